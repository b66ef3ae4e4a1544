"""Registers, scratch and LDS of the C2 step kernel, read from the notes of the built library's gfx950 code object (no GPU, no
instructions: metadata only).

consistency_step_q32_kernel<NS, P, 512> is built for SEVEN resident 256-thread blocks per CU where seven tiles fit the LDS (one or
two weights: 16.6 KB each).  Seven blocks per CU are 7 wavefronts per SIMD, and the hardware admits them only if
  * vgpr_count <= 72: 512 registers per SIMD lane / 7, rounded down to the allocation granule of 8;
  * sgpr_count <= 96: 256-thread blocks are admitted up to floor(800 / (ceil(sgpr / 16) * 16 + 16)) per CU -- 7 at 81..96, 6 at 97..112;
  * 7 * group_segment_fixed_size <= 160 KiB;
and nothing may live in scratch (private_segment_fixed_size == 0): a spill in the hot loop costs more than a wavefront buys.
Three weights stage a third 8 KB piece per tile: 7 * 24.9 KB exceeds the 160 KiB whatever the registers are, so those
instantiations (like the 768-row ones) are built for six and held to six's limits: vgpr_count <= 80 (512 / 6 -> 80),
sgpr_count <= 112, 6 tiles in the LDS, no scratch.  The same limits hold for the six-block builds dc_set_option(9, 1) selects."""
import os
import re
import struct

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS_BYTES = 160 * 1024
SLOT_COUNTS, WEIGHTS = (4, 8, 10, 16), (1, 2, 3)


def _unpack(b, i=0):
    """One MessagePack value at b[i:] -> (value, next index): the subset the AMDGPU metadata note uses."""
    t = b[i]
    if t <= 0x7f:
        return t, i + 1
    if t >= 0xe0:
        return t - 0x100, i + 1
    if 0x80 <= t <= 0x8f or t in (0xde, 0xdf):
        n, i = (t & 0x0f, i + 1) if t <= 0x8f else (struct.unpack_from('>H', b, i + 1)[0], i + 3) if t == 0xde else (struct.unpack_from('>I', b, i + 1)[0], i + 5)
        out = {}
        for _ in range(n):
            k, i = _unpack(b, i)
            out[k], i = _unpack(b, i)
        return out, i
    if 0x90 <= t <= 0x9f or t in (0xdc, 0xdd):
        n, i = (t & 0x0f, i + 1) if t <= 0x9f else (struct.unpack_from('>H', b, i + 1)[0], i + 3) if t == 0xdc else (struct.unpack_from('>I', b, i + 1)[0], i + 5)
        out = []
        for _ in range(n):
            v, i = _unpack(b, i)
            out.append(v)
        return out, i
    if 0xa0 <= t <= 0xbf:
        n = t & 0x1f
        return b[i + 1:i + 1 + n].decode(), i + 1 + n
    if t in (0xd9, 0xda, 0xdb, 0xc4, 0xc5, 0xc6):
        w = {0xd9: 1, 0xda: 2, 0xdb: 4, 0xc4: 1, 0xc5: 2, 0xc6: 4}[t]
        n = int.from_bytes(b[i + 1:i + 1 + w], 'big')
        s = b[i + 1 + w:i + 1 + w + n]
        return (s.decode() if t >= 0xd9 else bytes(s)), i + 1 + w + n
    if t == 0xc0:
        return None, i + 1
    if t in (0xc2, 0xc3):
        return t == 0xc3, i + 1
    if t in (0xcc, 0xcd, 0xce, 0xcf):
        w = 1 << (t - 0xcc)
        return int.from_bytes(b[i + 1:i + 1 + w], 'big'), i + 1 + w
    if t in (0xd0, 0xd1, 0xd2, 0xd3):
        w = 1 << (t - 0xd0)
        return int.from_bytes(b[i + 1:i + 1 + w], 'big', signed=True), i + 1 + w
    if t == 0xca:
        return struct.unpack_from('>f', b, i + 1)[0], i + 5
    if t == 0xcb:
        return struct.unpack_from('>d', b, i + 1)[0], i + 9
    raise AssertionError('MessagePack type 0x%02x' % t)


def _code_objects(blob):
    """The gfx950 ELF images of every offload bundle in the library (one per translation unit), found as tests/test_abi.py finds the
    target: by the bundle entries' triple."""
    magic = b'__CLANG_OFFLOAD_BUNDLE__'
    at = blob.find(magic)
    while at >= 0:
        n, = struct.unpack_from('<Q', blob, at + len(magic))
        i = at + len(magic) + 8
        for _ in range(n):
            off, size, tlen = struct.unpack_from('<QQQ', blob, i)
            triple = blob[i + 24:i + 24 + tlen]
            i += 24 + tlen
            if re.fullmatch(rb'hipv4-amdgcn-amd-amdhsa--gfx950', triple) and size:
                yield blob[at + off:at + off + size]
        at = blob.find(magic, at + len(magic))


def _kernels(elf):
    """[{'.name': .., '.vgpr_count': .., ...}] from the NT_AMDGPU_METADATA note of an ELF64 code object."""
    assert elf[:6] == b'\x7fELF\x02\x01', 'a little-endian ELF64 image'
    shoff, = struct.unpack_from('<Q', elf, 0x28)
    shentsize, shnum = struct.unpack_from('<HH', elf, 0x3a)
    out = []
    for s in range(shnum):
        stype, = struct.unpack_from('<I', elf, shoff + s * shentsize + 4)
        off, size = struct.unpack_from('<QQ', elf, shoff + s * shentsize + 0x18)
        if stype != 7:                                       # SHT_NOTE
            continue
        i = off
        while i + 12 <= off + size:
            namesz, descsz, ntype = struct.unpack_from('<III', elf, i)
            name = elf[i + 12:i + 12 + namesz]
            d0 = i + 12 + (namesz + 3) // 4 * 4
            if name.rstrip(b'\0') == b'AMDGPU' and ntype == 32:
                out += _unpack(elf[d0:d0 + descsz])[0].get('amdhsa.kernels', [])
            i = d0 + (descsz + 3) // 4 * 4
    return out


@pytest.fixture(scope='module')
def step_kernels():
    """{(NS, P, CAP, BLOCKS): notes} of every consistency_step_q32_kernel instantiation in the built library."""
    import __graft_entry__ as ge
    ge.build()
    from depth_correction_amd import _native
    blob = open(_native.lib_path(), 'rb').read()
    found = {}
    for elf in _code_objects(blob):
        for k in _kernels(elf):
            m = re.match(r'_ZN2dc27consistency_step_q32_kernelILi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)EEE', k['.name'])
            if m:
                found[tuple(int(v) for v in m.groups())] = k
    assert found, 'no consistency_step_q32_kernel in the code object'
    return found


def _default_blocks(p):
    """What the launch ladder's default instantiation is built for (step_q32_blocks<P, 512>, csrc/dc_cons_step.h)."""
    return 7 if p <= 2 else 6


@pytest.mark.parametrize('p', WEIGHTS)
@pytest.mark.parametrize('ns', SLOT_COUNTS)
def test_default_step_kernel_fits_its_residency(step_kernels, ns, p):
    blocks = _default_blocks(p)
    k = step_kernels.get((ns, p, 512, blocks))
    assert k is not None, 'consistency_step_q32_kernel<%d, %d, 512> built for %d blocks per CU is missing: %s' % (ns, p, blocks, sorted(step_kernels))
    print('consistency_step_q32_kernel<%d, %d, 512> (%d blocks): vgpr %d sgpr %d scratch %d lds %d' % (
        ns, p, blocks, k['.vgpr_count'], k['.sgpr_count'], k['.private_segment_fixed_size'], k['.group_segment_fixed_size']))
    assert k['.private_segment_fixed_size'] == 0
    if blocks == 7:
        assert k['.vgpr_count'] <= 72
        assert k['.sgpr_count'] <= 96
        assert 7 * k['.group_segment_fixed_size'] <= LDS_BYTES
    else:
        assert 7 * k['.group_segment_fixed_size'] > LDS_BYTES, 'seven tiles fit the LDS: this instantiation should be built for seven'
        assert k['.vgpr_count'] <= 80
        assert k['.sgpr_count'] <= 112
        assert 6 * k['.group_segment_fixed_size'] <= LDS_BYTES


@pytest.mark.parametrize('p', (1, 2))
@pytest.mark.parametrize('ns', SLOT_COUNTS)
def test_six_block_build_of_the_ab_switch(step_kernels, ns, p):
    """dc_set_option(9, 1): the same body under __launch_bounds__(256, 6) -- no scratch either, six's registers."""
    k = step_kernels.get((ns, p, 512, 6))
    assert k is not None, sorted(step_kernels)
    assert k['.private_segment_fixed_size'] == 0
    assert k['.vgpr_count'] <= 80
    assert k['.sgpr_count'] <= 112
    assert k['.group_segment_fixed_size'] == step_kernels[(ns, p, 512, 7)]['.group_segment_fixed_size']
