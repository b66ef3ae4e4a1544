#!/usr/bin/env python3
"""Are the device code objects of two builds of libdc_hip.so the same?  For a change that must not touch device code (a host-side
refactor): dumps .hip_fatbin of both libraries (llvm-objcopy), finds every gfx950 ELF in it and compares the defined function symbols --
the set of names (no instantiation added or dropped), each symbol's size and the SHA-256 of its code bytes.  Exit status 1 on a difference.

    python3 tools/compare_code_objects.py parent/libdc_hip.so depth_correction_amd/lib/libdc_hip.so"""
import hashlib
import os
import struct
import subprocess
import sys
import tempfile


def fatbin(path):
    with tempfile.NamedTemporaryFile() as f:
        subprocess.run([os.path.join(os.environ.get('ROCM_PATH', '/opt/rocm'), 'lib/llvm/bin/llvm-objcopy'), '--dump-section', '.hip_fatbin=' + f.name, path, '/dev/null'], check=True)
        return open(f.name, 'rb').read()


def elves(blob):
    pos = 0
    while True:
        pos = blob.find(b'\x7fELF\x02\x01\x01', pos)
        if pos < 0:
            return
        e_shoff, = struct.unpack_from('<Q', blob, pos + 0x28)
        e_shentsize, e_shnum = struct.unpack_from('<HH', blob, pos + 0x3A)
        size = e_shoff + e_shentsize * e_shnum
        yield blob[pos:pos + size]
        pos += size


def functions(elf):
    e_shoff, = struct.unpack_from('<Q', elf, 0x28)
    e_shentsize, e_shnum, e_shstrndx = struct.unpack_from('<HHH', elf, 0x3A)
    secs = []
    for i in range(e_shnum):
        name, typ, flags, addr, off, size, link, info, align, entsize = struct.unpack_from('<IIQQQQIIQQ', elf, e_shoff + i * e_shentsize)
        secs.append(dict(name=name, type=typ, addr=addr, off=off, size=size, link=link, entsize=entsize))
    out = {}
    for s in secs:
        if s['type'] != 2:       # SHT_SYMTAB
            continue
        strtab = secs[s['link']]
        for j in range(s['size'] // 24):
            st_name, st_info, st_other, st_shndx, st_value, st_size = struct.unpack_from('<IBBHQQ', elf, s['off'] + j * 24)
            if (st_info & 0xF) != 2 or st_shndx == 0 or st_shndx >= e_shnum:       # STT_FUNC, defined
                continue
            end = elf.index(b'\0', strtab['off'] + st_name)
            nm = elf[strtab['off'] + st_name:end].decode()
            sec = secs[st_shndx]
            code = elf[sec['off'] + st_value - sec['addr']: sec['off'] + st_value - sec['addr'] + st_size]
            out[nm] = (st_size, hashlib.sha256(code).hexdigest())
    return out


def all_functions(path):
    out = {}
    n = 0
    for elf in elves(fatbin(path)):
        n += 1
        for nm, v in functions(elf).items():
            out.setdefault(nm, []).append(v)
    return n, out


na, a = all_functions(sys.argv[1])
nb, b = all_functions(sys.argv[2])
print('code objects: %d vs %d; function symbols: %d vs %d' % (na, nb, len(a), len(b)))
print('only in first:', sorted(set(a) - set(b)))
print('only in second:', sorted(set(b) - set(a)))
diff = [nm for nm in a if nm in b and sorted(a[nm]) != sorted(b[nm])]
print('same name, different size or bytes: %d' % len(diff))
for nm in diff[:20]:
    print('  ', nm, a[nm], b[nm])
sys.exit(1 if (diff or set(a) != set(b) or na != nb) else 0)
