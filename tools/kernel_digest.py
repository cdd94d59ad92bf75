#!/usr/bin/env python3
"""One line per gfx950 kernel of a built library: a digest of its instructions and its kernel descriptor.

Two runs compared with `diff` show whether a change to the sources or to the build moved any kernel: a kernel compiled to the same
instructions with the same descriptor (register counts, LDS size, scratch, ...) prints the same line wherever its code object
ends up in the library.  A kernel symbol that occurs in more than one code object (a template instantiated in two translation
units: twice the compile time, and the runtime picks one copy per module) is reported and fails the run.

Per kernel, sorted by demangled name:
    <sha256[:16] of the instruction words> <the 64 descriptor bytes, entry offset zeroed> <size in bytes> <demangled name>
The instruction words are the hex encodings `llvm-objdump -d` prints (addresses and symbolised branch targets are not hashed:
branches are pc-relative, so the words do not depend on where the kernel lies; the literal of the s_add_u32 / s_addc_u32 pair
behind an s_getpc_b64, the pc-relative address of a device variable, does, and is hashed as zero).  The descriptor is the kernel's `.kd` object; its
bytes 16-23 (kernel_code_entry_byte_offset) depend on the layout of the code object only and are zeroed.

usage: kernel_digest.py [--duplicates-only] lib.so | obj.o [obj.o ...]
"""
import hashlib
import re
import shutil
import subprocess
import sys
import tempfile
from collections import defaultdict
from pathlib import Path

LLVM_BIN = Path("/opt/rocm/lib/llvm/bin")
SYM = re.compile(r"^\s*\d+:\s+([0-9a-f]+)\s+(\d+)\s+(FUNC|OBJECT)\s+\S+\s+\S+\s+(\d+)\s+(\S+)$")
LABEL = re.compile(r"^[0-9a-f]+ <(.+)>:$")
WORDS = re.compile(r"//\s*([0-9A-Fa-f]+):((?:\s+[0-9A-Fa-f]{8})+)")


def llvm_tool(name):
    """path of an LLVM binutil of the ROCm toolchain (or of PATH), None where there is none"""
    p = LLVM_BIN / name
    return str(p) if p.exists() else shutil.which(name)


def code_objects(binary: Path, tmp: Path):
    """every gfx950 code object embedded in a hipcc host object or shared library (llvm-objdump --offloading writes them next to
    its input), in the order of the fat binary"""
    local = tmp / binary.name
    local.write_bytes(binary.read_bytes())
    subprocess.run([llvm_tool("llvm-objdump"), "--offloading", str(local)], check=True, stdout=subprocess.DEVNULL,
                   stderr=subprocess.DEVNULL)
    cos = [p for p in tmp.glob(binary.name + ".*gfx950*")]
    return sorted(cos, key=lambda p: int(p.name[len(binary.name) + 1:].split(".")[0]))


def kernels(co: Path):
    """{mangled kernel name: (instruction digest, descriptor hex, code size)} of one code object"""
    data = co.read_bytes()
    readelf = llvm_tool("llvm-readelf")
    sections = {}                                      # index -> (address, file offset)
    for line in subprocess.run([readelf, "-SW", str(co)], check=True, capture_output=True, text=True).stdout.splitlines():
        m = re.match(r"^\s*\[\s*(\d+)\]\s+\S+\s+\S+\s+([0-9a-f]+)\s+([0-9a-f]+)\s", line)
        if m:
            sections[int(m.group(1))] = (int(m.group(2), 16), int(m.group(3), 16))
    funcs, kds = {}, {}
    symtab = subprocess.run([readelf, "-sW", str(co)], check=True, capture_output=True, text=True).stdout
    for line in symtab.splitlines():
        m = SYM.match(line)
        if not m:
            continue
        value, size, kind, ndx, name = int(m.group(1), 16), int(m.group(2)), m.group(3), int(m.group(4)), m.group(5)
        if kind == "OBJECT" and name.endswith(".kd") and size == 64:
            addr, off = sections[ndx]
            kd = bytearray(data[off + value - addr: off + value - addr + 64])
            kd[16:24] = bytes(8)                       # kernel_code_entry_byte_offset
            kds[name[:-3]] = kd.hex()
        elif kind == "FUNC":
            funcs[name] = (value, size)
    hashes, cur, end, pcrel = {}, None, 0, 0
    asm = subprocess.run([llvm_tool("llvm-objdump"), "-d", str(co)], check=True, capture_output=True, text=True).stdout
    for line in asm.splitlines():
        m = LABEL.match(line)
        if m:
            cur = hashes.setdefault(m.group(1), hashlib.sha256()) if m.group(1) in kds else None
            end = sum(funcs[m.group(1)]) if cur is not None else 0
            continue
        if cur is not None:
            w = WORDS.search(line)
            if w and int(w.group(1), 16) < end:        # the disassembly runs on into the padding behind the symbol's last instruction
                words, op = w.group(2).split(), line.split()[0]
                if pcrel and op in ("s_add_u32", "s_addc_u32") and len(words) == 2:
                    words[1], pcrel = "00000000", pcrel - 1
                else:
                    pcrel = 2 if op == "s_getpc_b64" else 0
                cur.update(" ".join(words).upper().encode() + b"\n")
    return {name: (hashes[name].hexdigest()[:16], kds[name], funcs[name][1]) for name in kds}


def digest(binaries):
    """(lines, duplicates): lines sorted by demangled name; duplicates = {mangled name: [code objects]} for the kernel symbols
    found in more than one code object"""
    found = defaultdict(list)                          # mangled name -> [(code object label, record)]
    with tempfile.TemporaryDirectory() as d:
        for i, b in enumerate(binaries):
            sub = Path(d) / str(i)
            sub.mkdir()
            for co in code_objects(Path(b), sub):
                label = f"{Path(b).name}#{co.name[len(Path(b).name) + 1:].split('.')[0]}"
                for name, rec in kernels(co).items():
                    found[name].append((label, rec))
    names = sorted(found)
    filt = shutil.which("c++filt") or llvm_tool("llvm-cxxfilt")
    plain = subprocess.run([filt], input="\n".join(names), capture_output=True, text=True, check=True).stdout.splitlines() if filt and names else names
    lines = [f"{rec[0]} {rec[1]} {rec[2]:6d} {dem}" for dem, name in sorted(zip(plain, names)) for _, rec in found[name]]
    return lines, {n: [lab for lab, _ in v] for n, v in found.items() if len(v) > 1}


def main():
    args = sys.argv[1:]
    binaries = [a for a in args if not a.startswith("--")]
    if not binaries:
        raise SystemExit(__doc__)
    lines, dups = digest(binaries)
    if "--duplicates-only" not in args:
        print("\n".join(lines))
    if dups:
        for n, where in sorted(dups.items()):
            print(f"kernel_digest: {n} occurs in {len(where)} code objects: {', '.join(where)}", file=sys.stderr)
        raise SystemExit(f"kernel_digest: {len(dups)} kernel symbol(s) in more than one code object")


if __name__ == "__main__":
    main()
