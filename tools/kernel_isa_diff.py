#!/usr/bin/env python3
"""Compares the gfx950 kernels of two builds instruction by instruction (no GPU needed).

Usage: python tools/kernel_isa_diff.py OBJ_DIR_A OBJ_DIR_B [--rename OLD=NEW ...] [--filter TEXT]

For every kernel in the objects (*.o) of either directory: the kernel's disassembly (ROCm
llvm-objdump -d) with addresses and encodings stripped and branch targets made kernel-relative,
and its code-object note fields (kernel_resources.FIELDS).  A kernel is `identical` when both
the text and the fields match; kernels are matched by symbol name whichever object holds them,
so a kernel that moved between translation units still meets its counterpart.  --rename maps a
substring of A's symbol names before matching (a kernel whose template list changed).

Two builds side by side: AG_RS_OBJ_DIR / AG_RS_LIB_NAME (alpenglow_amd/build.py).  The tool
compares text and nothing else.  Exit status 1 if any kernel differs or has no counterpart.
"""
import argparse
import difflib
import glob
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from kernel_resources import FIELDS, LLVM, kernel_notes, unbundle  # noqa: E402

LABEL = re.compile(r"^[0-9a-f]+ <(\S+)>:$")
TARGET = re.compile(r"<([^>+]+)(?:\+(0x[0-9a-f]+))?>\s*$")


def kernels_of(obj, d):
    """{kernel symbol: (normalised instruction text, note fields)} of one host object."""
    if b".hip_fatbin" not in subprocess.run([f"{LLVM}/llvm-readelf", "-S", obj], check=True,
                                            capture_output=True).stdout:
        return {}
    co = os.path.join(d, "k.co")
    unbundle(obj, co)
    notes = kernel_notes(co)
    dis = subprocess.run([f"{LLVM}/llvm-objdump", "-d", co], check=True, capture_output=True, text=True).stdout
    text, cur = {}, None
    for line in dis.splitlines():
        m = LABEL.match(line)
        if m:
            cur = m.group(1)
            text[cur] = []
            continue
        if cur is None or not line.strip():
            continue
        ins, _, comment = line.partition("//")
        ins = " ".join(ins.split())
        t = TARGET.search(comment)
        if t:  # a branch: its target as an offset from its own kernel's start
            where = t.group(2) or "0x0"
            ins = ins.rsplit(" ", 1)[0] + (f" <+{where}>" if t.group(1) == cur else f" <{t.group(1)}+{where}>")
        text[cur].append(ins)
    for ins in text.values():  # the padding behind a kernel's last instruction depends on what follows it
        while ins and ins[-1] in ("s_nop 0", "s_code_end", "..."):
            ins.pop()
    return {k: ("\n".join(text.get(k, [])), notes[k]) for k in notes}


def build_of(objdir, d):
    out = {}
    for obj in sorted(glob.glob(os.path.join(objdir, "*.o"))):
        for k, v in kernels_of(obj, d).items():
            out[k] = (*v, os.path.basename(obj)[:-2])
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("dir_a")
    ap.add_argument("dir_b")
    ap.add_argument("--rename", action="append", default=[], metavar="OLD=NEW")
    ap.add_argument("--filter", default="", help="only kernels whose symbol contains this text")
    ap.add_argument("--diff", type=int, default=0, metavar="N", help="show the first N lines of each difference")
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as d:
        a, b = build_of(args.dir_a, d), build_of(args.dir_b, d)
    for r in args.rename:
        old, new = r.split("=", 1)
        a = {k.replace(old, new): v for k, v in a.items()}
    same = diff = alone = 0
    for k in sorted(set(a) | set(b)):
        if args.filter not in k:
            continue
        if k not in a or k not in b:
            alone += 1
            print(f"only in {'A' if k in a else 'B'}  {(a.get(k) or b.get(k))[2]:24s} {k}")
            continue
        (ta, na, fa), (tb, nb, fb) = a[k], b[k]
        where = fa if fa == fb else f"{fa} -> {fb}"
        fields = " ".join(f"{f}={na[f]}" if na[f] == nb[f] else f"{f}={na[f]}->{nb[f]}" for f in FIELDS)
        if ta == tb and na == nb:
            same += 1
            print(f"identical  {where:40s} {ta.count(chr(10)) + 1:6d} insts  {fields}  {k}")
        else:
            diff += 1
            la, lb = ta.split("\n"), tb.split("\n")
            first = next((i for i, (x, y) in enumerate(zip(la, lb)) if x != y), min(len(la), len(lb)))
            print(f"DIFFERENT  {where:40s} {len(la):6d} -> {len(lb)} insts, first at {first}  {fields}  {k}")
            if args.diff:
                for line in list(difflib.unified_diff(la, lb, "A", "B", n=2, lineterm=""))[:args.diff]:
                    print("    " + line)
    print(f"{same} identical, {diff} different, {alone} without counterpart")
    return 1 if diff or alone else 0


if __name__ == "__main__":
    sys.exit(main())
