// The counter-based generator of the deterministic samplers (RANSAC hypotheses: dc_planes.hip; mesh sampling: dc_meshdist.hip;
// restated in Python by segmentation.splitmix64).  Host and device.
#pragma once
#include "dc_common.h"

namespace dc {

DC_HD uint64_t splitmix64(uint64_t x) {
  uint64_t z = x + 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

}  // namespace dc
