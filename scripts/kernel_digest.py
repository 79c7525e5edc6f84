#!/usr/bin/env python3
"""One line per gfx950 kernel of the build: what the compiler made of it, as a hash and its resource numbers.

    python scripts/kernel_digest.py [object directory, default deepdish_amd/csrc/_obj] > digest.txt

For every object it takes the device code object out (llvm-objcopy --dump-section .hip_fatbin, clang-offload-bundler
--unbundle), reads the symbol table and the metadata note (llvm-readelf -sW / --notes) and prints, tab-separated and sorted:

    source  demangled name  code bytes  sha256 of the code  vgpr  agpr  sgpr  lds bytes  scratch bytes  vgpr spills  sgpr spills

Two builds compute the same thing on the device where their lines are equal (diff the two outputs).  It only hashes and
tabulates: no instruction is looked at.  LLVM's tools are taken from $ROCM_LLVM_BIN (default /opt/rocm/llvm/bin)."""
import hashlib
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.environ.get('ROCM_LLVM_BIN', '/opt/rocm/llvm/bin')
TARGET = 'hipv4-amdgcn-amd-amdhsa--gfx950'
NOTE_KEYS = ('.vgpr_count', '.agpr_count', '.sgpr_count', '.group_segment_fixed_size', '.private_segment_fixed_size',
             '.vgpr_spill_count', '.sgpr_spill_count')


def tool(name, *args):
    return subprocess.run([os.path.join(BIN, name)] + list(args), check=True, capture_output=True, text=True).stdout


def code_object(obj, tmp):
    """The gfx950 code object inside a host object, or None (a .cpp source has no device code)."""
    fat, co = os.path.join(tmp, 'fatbin'), os.path.join(tmp, 'co')
    if '.hip_fatbin' not in tool('llvm-readelf', '-SW', obj):
        return None
    tool('llvm-objcopy', '--dump-section', '.hip_fatbin=' + fat, obj)
    tool('clang-offload-bundler', '--unbundle', '--type=o', '--targets=' + TARGET, '--input=' + fat, '--output=' + co)
    return co


def sections(co):
    """index -> (address, file offset)"""
    out = {}
    for m in re.finditer(r'^\s*\[\s*(\d+)\]\s+\S*\s+\S+\s+([0-9a-f]{16})\s+([0-9a-f]+)\s', tool('llvm-readelf', '-SW', co), re.M):
        out[int(m.group(1))] = (int(m.group(2), 16), int(m.group(3), 16))
    return out


def functions(co, demangle):
    """.symtab's FUNC symbols in table order: (value, size, section index, name)"""
    text = tool('llvm-readelf', '-sW', *(['-C'] if demangle else []), co)
    text = text[text.index("'.symtab'"):]
    syms = []
    for line in text.splitlines():
        f = line.split(None, 7)
        if len(f) == 8 and f[3] == 'FUNC' and f[6].isdigit():
            syms.append((int(f[1], 16), int(f[2]), int(f[6]), f[7]))
    return syms


def metadata(co):
    """mangled kernel name -> the NOTE_KEYS numbers, from the amdhsa.kernels list of the metadata note"""
    out, cur = {}, {}
    for line in tool('llvm-readelf', '--notes', co).splitlines():
        m = re.match(r'^ {2}(- | {2})(\.[a-z_]+):\s+(\S+)\s*$', line)               # a kernel's own keys: its arguments' lie deeper
        if not m:
            continue
        if m.group(1) == '- ' and cur.get('.name'):                                 # the list's next kernel
            out[cur['.name']] = cur
            cur = {}
        cur[m.group(2)] = m.group(3)
    if cur.get('.name'):
        out[cur['.name']] = cur
    return out


def digest(obj_dir):
    lines = []
    for name in sorted(os.listdir(obj_dir)):
        if not name.endswith('.o'):
            continue
        with tempfile.TemporaryDirectory() as tmp:
            co = code_object(os.path.join(obj_dir, name), tmp)
            if co is None:
                continue
            secs, meta = sections(co), metadata(co)
            with open(co, 'rb') as f:
                blob = f.read()
            for (value, size, ndx, mangled), (_, _, _, plain) in zip(functions(co, False), functions(co, True)):
                addr, off = secs[ndx]
                code = blob[value - addr + off:value - addr + off + size]
                assert len(code) == size, (name, mangled)
                k = meta.get(mangled, {})                        # a device function that is no kernel has no metadata
                lines.append('\t'.join([name[:-2], plain, str(size), hashlib.sha256(code).hexdigest()] + [k.get(key, '-') for key in NOTE_KEYS]))
    return sorted(lines)


if __name__ == '__main__':
    print('\n'.join(digest(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'deepdish_amd', 'csrc', '_obj'))))
