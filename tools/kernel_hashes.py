"""Per-kernel code hashes of librsp.so's gfx950 code objects (bench provenance).

usage: kernel_hashes.py LIBRSP.so OUT.json
       kernel_hashes.py LIB_OR_OBJECT --instantiations

The HIP fat binary in the .so holds one clang offload bundle per device translation unit; its
gfx950 entry is an AMDGPU ELF.  For every kernel symbol (STT_FUNC with a `.kd` descriptor) the
bytes of its code are hashed; kernels are keyed by their short name (the identifier before the
template arguments, as tools/pmc_traffic.py keys its counters), all instantiations of a name
hashed together in mangled-name order.  bench.py compares these with the hashes a PMC traffic
file recorded when it was measured: a kernel whose code changed since has no measured traffic.

--instantiations prints one `hash mangled-name` line per kernel function instead, sorted by name,
for a library or a single object file (build/rsp_k2.hip.o): two builds whose lists are equal
run the same machine code in every template instantiation.

The frame chain's kernels are spread over one translation unit per stage (rsp_k1.hip, rsp_k2.hip,
rsp_k3.hip, rsp_frame_aux.hip, rsp_stage3.hip, rsp_vcfar.hip, rsp_xcfar.hip, rsp_dbf.hip, rsp_mtd.hip, rsp_detect.hip) plus rsp_music.hip, so a library has
several code objects.  A kernel's mangled name found in two of them is an error (merge), and the
Makefile's hash step fails.
"""
import hashlib
import json
import re
import struct
import sys

MAGIC = b'__CLANG_OFFLOAD_BUNDLE__'


def code_objects(blob):
    i = blob.find(MAGIC)
    while i >= 0:
        n = struct.unpack_from('<Q', blob, i + 24)[0]
        p = i + 32
        for _ in range(n):
            off, size, tl = struct.unpack_from('<QQQ', blob, p)
            triple = blob[p + 24:p + 24 + tl].decode()
            p += 24 + tl
            if 'amdgcn' in triple and size:
                yield triple, blob[i + off:i + off + size]
        i = blob.find(MAGIC, i + 1)


def kernel_code(elf):
    """{mangled kernel name: bytes of its code} from one AMDGPU ELF (64-bit little endian)."""
    assert elf[:4] == b'\x7fELF' and elf[4] == 2 and elf[5] == 1
    shoff, = struct.unpack_from('<Q', elf, 0x28)
    shentsize, shnum, shstrndx = struct.unpack_from('<HHH', elf, 0x3A)
    secs = [struct.unpack_from('<IIQQQQIIQQ', elf, shoff + k * shentsize) for k in range(shnum)]
    out = {}
    for s in secs:
        if s[1] != 2:   # SHT_SYMTAB
            continue
        strtab = secs[s[6]]
        for k in range(s[5] // s[9]):
            name_off, info, other, shndx, value, size = struct.unpack_from('<IBBHQQ', elf, s[4] + k * s[9])
            if info & 0xF != 2 or size == 0 or shndx >= len(secs):   # STT_FUNC with code
                continue
            nm = elf[strtab[4] + name_off:elf.index(b'\0', strtab[4] + name_off)].decode()
            sec = secs[shndx]
            out[nm] = elf[sec[4] + (value - sec[3]):sec[4] + (value - sec[3]) + size]
    return out


def short_name(mangled):
    """The kernel's identifier: the first source name of the mangled name that is not the
    anonymous namespace (`_ZN12_GLOBAL__N_110k1_dbf_mtdI...` -> k1_dbf_mtd)."""
    if not mangled.startswith('_Z'):
        return mangled
    p = 3 if mangled.startswith('_ZN') else 2
    while True:
        m = re.match(r'(\d+)', mangled[p:])
        if not m:
            return mangled
        n = int(m.group(1))
        name = mangled[p + len(m.group(1)):p + len(m.group(1)) + n]
        p += len(m.group(1)) + n
        if not name.startswith('_GLOBAL__N'):
            return name


def merge(into, more):
    """Add one code object's kernels to `into`.  A mangled name that is there already is an error: two
    translation units define the same kernel, and a plain dict.update would hide one of them."""
    dup = sorted(set(into) & set(more))
    if dup:
        raise SystemExit('kernel defined in two code objects: ' + ', '.join(dup))
    into.update(more)
    return into


def kernels(path):
    """{mangled name: code bytes} of every kernel in the gfx950 code objects of a library or object."""
    blob = open(path, 'rb').read()
    out = {}
    for _, elf in code_objects(blob):   # kernels = functions that have a kernel descriptor
        kd = {n.decode()[:-3] for n in re.findall(rb'([_A-Za-z0-9]+\.kd)\0', elf)}
        merge(out, {nm: code for nm, code in kernel_code(elf).items() if nm in kd})
    return out


def main():
    if '--instantiations' in sys.argv[1:]:
        path, = [a for a in sys.argv[1:] if a != '--instantiations']
        funcs = kernels(path)
        for nm in sorted(funcs):
            print(hashlib.sha256(funcs[nm]).hexdigest()[:16], nm)
        return
    lib, out = sys.argv[1:3]
    funcs = kernels(lib)
    groups = {}
    for nm in sorted(funcs):
        groups.setdefault(short_name(nm), []).append(nm)
    res = {}
    for sn, names in sorted(groups.items()):
        h = hashlib.sha256()
        for nm in names:
            h.update(nm.encode() + b'\0' + funcs[nm])
        res[sn] = h.hexdigest()[:16]
    json.dump(res, open(out, 'w'), indent=1, sort_keys=True)


if __name__ == '__main__':
    main()
