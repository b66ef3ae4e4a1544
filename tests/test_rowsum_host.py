"""The fixed-order row reducer every finish kernel shares (csrc/dc_rowsum.h) through its host build (dc_host_rows_sum in
libdc_hostcheck.so, the header the kernels include), against a numpy fp64 emulation of the documented order: lane l of LANES adds the
rows l, l + LANES, ... in order starting from 0.0, then the LANES sums are added in lane order starting from 0.0.  Bit equality, not
a tolerance: an fp64 addition is one IEEE operation on the host as on the device, so the order is all there is to check."""
import ctypes

import numpy as np
import pytest


@pytest.fixture(scope='module')
def lib():
    """libdc_hostcheck.so with dc_host_rows_sum (rebuilt when the library at hand predates it)."""
    from helpers import hostcheck_lib
    lib = hostcheck_lib()
    if not hasattr(lib, 'dc_host_rows_sum'):
        import __graft_entry__ as ge
        ge.build()
        lib = hostcheck_lib()
    lib.dc_host_rows_sum.restype = ctypes.c_double
    lib.dc_host_rows_sum.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_int]
    return lib


def emulate(rows, q, lanes, lane_stride=None, lane_order=None):
    """The documented order in numpy fp64 scalars; lane_stride / lane_order let a test state a WRONG order."""
    lane_stride = lanes if lane_stride is None else lane_stride
    tot = np.float64(0.0)
    for l in (range(lanes) if lane_order is None else lane_order):
        s = np.float64(0.0)
        for r in range(l, rows.shape[0], lane_stride):
            s = s + rows[r, q]
        tot = tot + s
    return tot


def mixed_rows(n_rows, stride, seed):
    """Values of both signs over 60 binades: almost every addition rounds, so another order gives other bits."""
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n_rows, stride)) * np.exp2(rng.integers(-30, 31, size=(n_rows, stride)).astype(np.float64))


def row_counts(lanes):
    # the sizes at which the eight-rows-at-a-time loop is entered, left and re-entered
    return [0, 1, lanes - 1, lanes, lanes + 1, 8 * lanes - 1, 8 * lanes, 8 * lanes + 1, 16 * lanes + 3]


@pytest.mark.parametrize('stride', [17, 30, 93])
@pytest.mark.parametrize('lanes', [4, 8])
def test_rows_sum_order_is_bit_exact(lib, lanes, stride):
    for n_rows in row_counts(lanes):
        rows = mixed_rows(n_rows, stride, 1000 * lanes + 10 * stride + n_rows)
        for q in range(stride):
            got = lib.dc_host_rows_sum(rows.ctypes.data, n_rows, stride, q, lanes)
            want = emulate(rows, q, lanes)
            assert np.float64(got).tobytes() == want.tobytes(), (lanes, stride, n_rows, q, got, want)


@pytest.mark.parametrize('lanes', [4, 8])
def test_another_lane_stride_or_lane_order_gives_other_bits(lib, lanes):
    """The test above has teeth: on the same inputs a lane stride of LANES + 1 rows, or the lane sums added from the
    last lane down, differ from the library (in some column: a reversed sum of four terms often rounds alike)."""
    stride, n_rows = 30, 16 * lanes + 3
    rows = mixed_rows(n_rows, stride, 7 + lanes)
    got = [np.float64(lib.dc_host_rows_sum(rows.ctypes.data, n_rows, stride, q, lanes)).tobytes() for q in range(stride)]
    for wrong in (dict(lane_stride=lanes + 1), dict(lane_order=range(lanes - 1, -1, -1))):
        differ = sum(got[q] != emulate(rows, q, lanes, **wrong).tobytes() for q in range(stride))
        assert differ > 0, wrong


def test_other_lane_counts_are_refused(lib):
    rows = np.ones((4, 17))
    assert np.isnan(lib.dc_host_rows_sum(rows.ctypes.data, 4, 17, 0, 5))
