#!/usr/bin/env python3
"""Per-symbol comparison of the gfx950 device code of two builds: tools/disasm_diff.py DIR_A DIR_B

For every *.o present in both directories (csrc/obj or csrc/obj_probes of two checkouts built by csrc/build.sh) the gfx950 code object is
unbundled as tools/disasm.sh does and disassembled with llvm-objdump -d; the listings are split per symbol and compared as instruction text,
without the address / encoding columns.  One line per differing symbol (object, name, differing lines, symbol length), then
"N of M symbols identical".  Exit status 1 if a symbol differs or a symbol or object exists on one side only."""
import difflib
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin")
_SYMBOL = re.compile(r"^[0-9a-f]+ <(.+)>:\s*$")
_COLUMNS = re.compile(r"^\s*[0-9a-f]+:\s+(?:[0-9a-f]{2}\s)+\s*|\s*//.*$")      # "addr: bytes" in front, "// addr: encoding" behind


def split_symbols(listing):
    """{symbol: [instruction text, ...]} of an llvm-objdump -d listing, address / encoding columns dropped."""
    syms, cur = {}, None
    for line in listing.splitlines():
        m = _SYMBOL.match(line)
        if m:
            cur = syms.setdefault(m.group(1), [])
        elif cur is not None and line.strip():
            cur.append(_COLUMNS.sub("", line).strip())
    return syms


def compare(listing_a, listing_b):
    """(rows, identical, total): rows = [(symbol, differing lines or None if on one side only, symbol length)] of the symbols that differ."""
    a, b = split_symbols(listing_a), split_symbols(listing_b)
    rows = []
    for name in sorted(set(a) | set(b)):
        if name not in a or name not in b:
            rows.append((name, None, len(a.get(name, b.get(name)))))
        elif a[name] != b[name]:
            ops = difflib.SequenceMatcher(None, a[name], b[name], autojunk=False).get_opcodes()
            rows.append((name, sum(max(i2 - i1, j2 - j1) for tag, i1, i2, j1, j2 in ops if tag != "equal"), max(len(a[name]), len(b[name]))))
    total = len(set(a) | set(b))
    return rows, total - len(rows), total


def disassemble(obj, tmp):
    fat, dev = os.path.join(tmp, "fat.bin"), os.path.join(tmp, "dev.co")
    r = subprocess.run([os.path.join(LLVM, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, obj, os.path.join(tmp, "copy.o")], capture_output=True)
    if r.returncode != 0 or not os.path.isfile(fat):      # a translation unit without device code (host glue only), as tools/kernel_resources.py reads it
        return ""
    subprocess.check_call([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                           "--input=" + fat, "--output=" + dev])
    return subprocess.check_output([os.path.join(LLVM, "llvm-objdump"), "-d", dev], text=True)


def main(dir_a, dir_b):
    objs = [sorted(f for f in os.listdir(d) if f.endswith(".o")) for d in (dir_a, dir_b)]
    one_sided = sorted(set(objs[0]) ^ set(objs[1]))
    for f in one_sided:
        print("%s: object on one side only" % f)
    identical = total = 0
    for f in sorted(set(objs[0]) & set(objs[1])):
        with tempfile.TemporaryDirectory() as ta, tempfile.TemporaryDirectory() as tb:
            rows, same, n = compare(disassemble(os.path.join(dir_a, f), ta), disassemble(os.path.join(dir_b, f), tb))
        for name, diff, length in rows:
            print("%s: %s: %s" % (f, name, "symbol on one side only (%d lines)" % length if diff is None else "%d of %d lines differ" % (diff, length)))
        identical, total = identical + same, total + n
    print("%d of %d symbols identical" % (identical, total))
    return 0 if identical == total and not one_sided else 1


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
