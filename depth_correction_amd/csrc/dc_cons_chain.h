// Chained steps: the Adam update and the final sums of one evaluation inside the launch of the next (StepChain, the leading blocks,
// the published weights and the wait for them), and the step kernel's per-block header (StepHdr).  A part of dc_consistency.hip, included
// after dc_cons_basis.h; dc_blocktab.hip includes it for StepHdr's layout (it needs dc_device.h only).
#pragma once

namespace dc {

// torch.optim.Adam (single-tensor path, no amsgrad) for one fp64 parameter; grad is scaled first.
struct AdamArgs {
  double* p; double* m; double* v;     // parameters, exp_avg, exp_avg_sq (p == nullptr: no update)
  int n;
  double grad_scale, lr, b1, b2, eps, weight_decay, bias1, bias2_sqrt;
};
// (p0, m0, v0: the parameter's state, loaded by the caller -- early, so the trip hides behind its own work)
__device__ __forceinline__ void adam_apply(const AdamArgs& a, int i, double grad, double p0, double m0, double v0) {
  double g = grad * a.grad_scale;
  if (a.weight_decay != 0.0) g += a.weight_decay * p0;
  const double mi = m0 + (g - m0) * (1.0 - a.b1);                   // exp_avg.lerp_(grad, 1 - beta1)
  const double vi = v0 * a.b2 + (1.0 - a.b2) * g * g;               // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, 1 - beta2)
  a.m[i] = mi; a.v[i] = vi;
  const double denom = sqrt(vi) / a.bias2_sqrt + a.eps;
  a.p[i] = p0 + (-(a.lr / a.bias1)) * (mi / denom);
}
__device__ __forceinline__ void adam_update(const AdamArgs& a, int i, double grad) { adam_apply(a, i, grad, a.p[i], a.m[i], a.v[i]); }

// ---- chained steps: the previous evaluation's final sums inside the next evaluation's launch -----------------------------
// A dependent reduction launch after a kernel that filled every L2 costs ~9 us, an eighth of a C2 step.  In a chain
// of steps the launch of step t + 1 therefore starts with `n_front` leading blocks that finish step t: block a < 2 + P sums
// column a of step t's partial rows (one per BLOCK in this mode: 7.8 k rows, one trip for 256 lanes), writes out_prev[a],
// takes weight (a - 2)'s Adam step and raises ready[parity]; the other blocks fetch everything that does not depend on the
// weights, then wait for ready[parity] == P.  The leading blocks are dispatched first and need nothing from the waiting ones,
// so they always finish; the wait is bounded all the same (a grid must drain).  parity alternates per launch: this launch
// clears the other flag and writes its own partial rows to the other buffer.  The last step of a chain is finished by the
// ordinary reduction launch (flush).
struct StepChain {
  int32_t* ready;            // 64 bytes, zero before the first launch of a chain (the published weights, chain_publish); nullptr: ordinary
                             // launch (per-wavefront rows)
  uint32_t stamp;            // this launch's number: what marks a published word as belonging to it
  int parity, has_prev, n_front, n_out;
  int reverse;               // this launch walks every XCD's share of the blocks backwards (chain_block_of)
  const double* prev;        // the previous launch's rows [(2 + P)][prev_rows]
  int64_t prev_rows;
  const double* grad_sum;    // or: the previous evaluation's dL/dw already summed (over the ranks: an all-reduce ran in between);
                             // the leading blocks then only take the Adam update (out_prev is not written)
  double* out_prev;          // [n_out] <- sums of the previous evaluation (slots beyond 2 + P: 0)
  double* w_prev_out;        // [P] or nullptr <- the weights the previous evaluation used (a training log records them: train.py)
  int32_t* status;           // bit 0: a point left the q32 extent (read); bit 1: a wait for the weights ran out (raised here)
  int spin_limit;            // polls a waiting block makes before it gives up (dc_set_option(5, n); 0: gives up at once)
  const double* w_now;       // the caller's weights (what a launch with nothing to finish publishes)
  const int32_t* prev_status;  // linked chains: the status word of the sequence whose rows are finished (nullptr: `status`)
  const double* acc_in;      // [2 + P] or nullptr: added to the previous launch's sums (the sequences of ONE loss evaluated launch after
                             // launch: the running sums of the step's earlier sequences)
  AdamArgs adam;             // the update the previous evaluation's gradient feeds (bias corrections of ITS step)
  const uint8_t* blk_skip;   // [blocks] or nullptr: blocks none of whose centres is inside the loss mask (dcSequenceDesc.blk_skip): they add
                             // nothing to the loss, the count or dL/dw and are treated like the padding blocks of the last round
};
// What a block of consistency_step_q32_kernel needs before it can fetch anything, as ONE 64-byte record per 256-point block
// (dcSequenceDesc.step_hdr, built by dc_step_header_build in dc_blocktab.hip, which includes this file for the layout): the
// block's entries of slot_ptr, blk_ptr, own_base and blk_skip and its 256 mask bytes were five arrays and six dependent trips;
// the first 32 bytes are one scalar load, a wavefront's in_mask word a second, issued together.
struct alignas(64) StepHdr {
  int32_t s0, nslots;        // slot_ptr[blk], slot_ptr[blk + 1] - slot_ptr[blk]
  int32_t base, nd;          // blk_ptr[blk], blk_ptr[blk + 1] - blk_ptr[blk]
  int32_t own;               // own_base[blk], or -1 (no own_base: a table for a compact centre list)
  int32_t flags;             // bit 0 (kStepHdrSkip): no centre of the block is inside the loss mask (blk_skip[blk])
  int32_t n_live;            // min(256, n - 256 blk)
  int32_t reserved;
  uint64_t in_mask[4];       // bit l of word w: lane 64 w + l is live and inside the mask (no mask: live)
};
static_assert(sizeof(StepHdr) == 64, "one record per cache-line half: a block's header never straddles two");
constexpr int32_t kStepHdrSkip = 1;
constexpr int32_t kStatusChainTimeout = 2;    // (bit 0: q32 overflow, raised by quantize())
constexpr int kChainFront = 8;             // leading blocks of a chained launch (a multiple of the XCD count)

// The logical block of this workgroup (xcd_block_of); -1: padding.  Every other launch of a chain of fixed-K steps walks its XCD's
// share of the blocks BACKWARDS: the basis rows are the same in every step, an XCD's 4 MB of L2 still holds the rows of the last
// ~260 blocks it finished, and a launch's first round -- 1 536 blocks that all start by fetching rows -- is its slowest
// (profiles/r04_block_trace.md: 12 us per block against 7.7 later on).  Walking back, the first round finds its rows in L2:
// C2 step 42.8 -> 41.4 us.  Block -> row of the partial sums is by grid position either way, so the order of the final
// additions differs between the two directions by rounding only (deterministic: the direction is the launch's parity).
__device__ __forceinline__ int64_t chain_block_of(const StepChain& ch, bool chained, int64_t nblocks) {
  const int64_t b = (int64_t)blockIdx.x - (chained ? ch.n_front : 0);
  if (!(chained && ch.reverse)) return xcd_block_of(b, nblocks);
  const int64_t per = (nblocks + kXcds - 1) / kXcds;
  const int64_t logical = (b % kXcds) * per + (per - 1 - b / kXcds);
  return logical < nblocks ? logical : -1;
}

// Weight k of a chained launch, published by the leading block that finished it and picked up by every other block in ONE
// memory trip: the double travels as two 64-bit words {low half | stamp}, {high half | stamp} (8-byte accesses are single-copy
// atomic), the stamp being the launch's number -- a word carrying it can only be this launch's.  (Rounds 2-4: a counter raised
// after a fence, polled, and then the weights loaded: two dependent trips through the fabric in front of every block's staging.)
__device__ __forceinline__ void chain_publish(const StepChain& ch, int k, double w) {
  unsigned long long* pub = reinterpret_cast<unsigned long long*>(ch.ready);
  const unsigned long long st = (unsigned long long)ch.stamp << 32;
  __hip_atomic_store(pub + 2 * k, st | (unsigned)__double2loint(w), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_store(pub + 2 * k + 1, st | (unsigned)__double2hiint(w), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// lane `l`'s value of v, the same for every lane of the wavefront (all of them active)
__device__ __forceinline__ double lane_value_f64(double v, int l) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l), __builtin_amdgcn_readlane(__double2loint(v), l));
}

template <int P>
__device__ __forceinline__ void chain_front_block(const StepChain& ch, double* lds /* [kBlock / kWave] in LDS */) {
  const int a = blockIdx.x;
  if (a == 0 && ch.has_prev && !ch.grad_sum)
    for (int z = 2 + P + threadIdx.x; z < ch.n_out; z += kBlock) ch.out_prev[z] = 0.0;
  if (a >= 2 + P) return;
  if (ch.grad_sum) {                     // the sums exist already: weight a - 2's update, then publish
    if (a >= 2 && threadIdx.x == 0) {
      if (ch.has_prev && ch.adam.p) adam_update(ch.adam, a - 2, ch.grad_sum[a - 2]);
      const double wk = ch.adam.p ? ch.adam.p[a - 2] : ch.w_now[a - 2];
      chain_publish(ch, a - 2, wk);
      if (ch.w_prev_out) ch.w_prev_out[a - 2] = wk;      // (this form records the weights THIS evaluation uses: its sums are current)
    }
    return;
  }
  const bool step_blk = ch.has_prev && ch.adam.p && a >= 2;
  const bool step = step_blk && threadIdx.x == 0;
  const int32_t* st_prev = ch.prev_status ? ch.prev_status : ch.status;
  const bool flagged = ch.has_prev && a == 0 && threadIdx.x == 0 && st_prev &&
                       __hip_atomic_load(st_prev, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0;
  // the parameter's state {p, m, v} is loaded by lanes 0, 1, 2 -- ONE register pair beside the 32 doubles in flight below, not
  // three in lane 0 (the block shares the step kernels' register allocation) -- and handed to lane 0 after the sum
  double st = 0.0;
  if (step_blk && threadIdx.x < 3) {
    const double* src = threadIdx.x == 0 ? ch.adam.p : threadIdx.x == 1 ? ch.adam.m : ch.adam.v;
    st = src[a - 2];
    if (threadIdx.x == 0 && ch.w_prev_out) ch.w_prev_out[a - 2] = st;
  }
  double s = 0.0;
  if (ch.has_prev) {
    constexpr int U = 32;
    const int64_t rows = ch.prev_rows;
    const uint32_t tid = threadIdx.x;
    // (the trip's first row and what is left of the column are the same for the whole block: scalar; a lane adds 32-bit offsets)
    for (int64_t b0 = 0; b0 < rows; b0 += (int64_t)U * kBlock) {
      const double* p = ch.prev + (int64_t)a * rows + b0;
      const uint32_t left = rows - b0 < (int64_t)U * kBlock ? (uint32_t)(rows - b0) : (uint32_t)(U * kBlock);
      double v[U];
#pragma unroll
      for (int u_ = 0; u_ < U; ++u_) v[u_] = (tid + (uint32_t)(u_ * kBlock) < left) ? p[tid + (uint32_t)(u_ * kBlock)] : 0.0;
#pragma unroll
      for (int w_ = U / 2; w_ > 0; w_ >>= 1) {
#pragma unroll
        for (int u_ = 0; u_ < w_; ++u_) v[u_] += v[u_ + w_];
      }
      s += v[0];
    }
    s = wave_sum(s);
  }
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  if (lane == 0) lds[wave] = s;
  __syncthreads();
  const double p0 = lane_value_f64(st, 0), m0 = lane_value_f64(st, 1), v0 = lane_value_f64(st, 2);     // (wavefront 0's are the state)
  if (threadIdx.x == 0) {
    if (ch.has_prev) {
      double t = 0.0;
      for (int wv = 0; wv < kBlock / kWave; ++wv) t += lds[wv];
      if (ch.acc_in) t += ch.acc_in[a];                      // (read before out_prev is written: the two may be one buffer)
      if (flagged) t = __longlong_as_double(0x7ff8000000000000ll);
      ch.out_prev[a] = t;
      if (step) adam_apply(ch.adam, a - 2, t, p0, m0, v0);
    }
    // weight a - 2 is final for this launch (the value just stored, or the caller's when there was nothing to finish)
    if (a >= 2) chain_publish(ch, a - 2, step ? ch.adam.p[a - 2] : ch.w_now[a - 2]);
  }
}

// chain_front_block on its own: finishes the last launch of a linked chain (dc_sequence_chain_flush_linked)
template <int P>
__global__ __launch_bounds__(kBlock) void chain_front_only_kernel(StepChain ch) {
  __shared__ double s_front[kBlock / kWave];
  chain_front_block<P>(ch, s_front);
}

// s_w[k] <- w_k * w_scale of this launch for the lanes of the block, as soon as its leading blocks have published them
// (bounded wait); *s_ok <- 0 when a wait ran out.  Every thread of the block calls it; the caller's barrier follows.
template <int P>
__device__ __forceinline__ void chain_weights(const StepChain& ch, double w_scale, double* s_w, int* s_ok) {
  const int tid = threadIdx.x;
  if (tid == 0) *s_ok = 1;
  if (tid < 2 * P) {
    const unsigned long long* pub = reinterpret_cast<const unsigned long long*>(ch.ready) + tid;
    unsigned long long word = 0;
    bool ok = false;
    for (int spin = 0; spin < ch.spin_limit; ++spin) {
      // (relaxed: an agent-scope acquire would invalidate this XCD's L2 on every poll -- nothing else is read through it)
      word = __hip_atomic_load(pub, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if ((uint32_t)(word >> 32) == ch.stamp) { ok = true; break; }
      __builtin_amdgcn_s_sleep(2);
    }
    const int half = (int)(uint32_t)word;
    const int other = __shfl_xor(half, 1, kWave);                       // lanes 2k / 2k + 1: low / high half of weight k
    if ((tid & 1) == 0) s_w[tid >> 1] = (ok ? __hiloint2double(other, half) : __longlong_as_double(0x7ff8000000000000ll)) * w_scale;
    // a wait that ran out poisons this launch's sums (NaN) AND says so: the status word tells it apart from a q32 overflow
    if (!ok) {
      *s_ok = 0;
      if (ch.status) atomicOr(ch.status, kStatusChainTimeout);
    }
  }
}

}  // namespace dc
