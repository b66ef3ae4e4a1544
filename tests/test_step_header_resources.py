"""The step header's builder is in the built library, and the C2 step kernel that reads the header -- one 64-byte scalar load per
block where it read slot_ptr, blk_ptr, own_base, blk_skip and the mask bytes -- still fits the residency it is built for: the
limits are those of tests/test_step_kernel_resources.py, applied by its own test functions to every default instantiation and to
the six-block builds (no GPU: the code object's notes only)."""
import pytest

from test_step_kernel_resources import (SLOT_COUNTS, WEIGHTS, _code_objects, _kernels, step_kernels,  # noqa: F401 (fixture)
                                        test_default_step_kernel_fits_its_residency as _default_fits,
                                        test_six_block_build_of_the_ab_switch as _six_fits)


def test_header_builder_is_built():
    import __graft_entry__ as ge
    ge.build()
    from depth_correction_amd import _native
    import ctypes
    assert 'dc_step_header_build' in _native._SIGNATURES
    getattr(ctypes.CDLL(_native.lib_path()), 'dc_step_header_build')
    blob = open(_native.lib_path(), 'rb').read()
    names = [k['.name'] for elf in _code_objects(blob) for k in _kernels(elf)]
    assert any('bt_step_header_kernel' in n for n in names), 'no header builder kernel in the gfx950 code objects'


def test_step_kernel_takes_the_header(step_kernels):
    """Every instantiation's mangled name carries the header's type where own_base was, and no mask pointer."""
    for key, k in step_kernels.items():
        assert 'PKNS_7StepHdrE' in k['.name'], (key, k['.name'])


@pytest.mark.parametrize('p', WEIGHTS)
@pytest.mark.parametrize('ns', SLOT_COUNTS)
def test_default_instantiations_keep_their_limits(step_kernels, ns, p):
    _default_fits(step_kernels, ns, p)


@pytest.mark.parametrize('p', (1, 2))
@pytest.mark.parametrize('ns', SLOT_COUNTS)
def test_six_block_builds_keep_their_limits(step_kernels, ns, p):
    _six_fits(step_kernels, ns, p)
