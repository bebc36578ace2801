#!/usr/bin/env python3
"""Compare two device-assembly listings kernel by kernel.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -I include --cuda-device-only -S csrc/X.hip -o new/X.s
    python tools/isa_diff.py old/X.s new/X.s [--map OLD_SYMBOL=NEW_SYMBOL ...] [--context N]

For every function symbol of the OLD listing it prints one line: `same` (the instruction stream and the
.amdhsa_ directives are equal), `DIFF` (followed by the first differing lines) or `GONE` (no such symbol in
the new listing), with the kernel's register, LDS and scratch directives. Symbols only the new listing has
are reported as `NEW`. Exit status 1 if anything is DIFF.

It compares text only. Before comparing it drops comments and normalises the compiler's local label
numbers (.LBB<n>_<m>, .Ltmp<n>, .Lfunc_end<n>, ...), which depend on a function's position in the file,
not on its code. `--map` names a kernel whose mangled name changed (a template parameter dropped): the
old symbol is compared with the new one.
"""
from __future__ import annotations

import argparse
import re
import sys

_FUNC_TYPE = re.compile(r"^\s*\.type\s+(\S+),@function")
_LABEL = re.compile(r"^([A-Za-z_.$][\w.$]*):")
_LBB = re.compile(r"\.LBB\d+_(\d+)")
_LNUM = re.compile(r"\.L(tmp|func_begin|func_end|JTI|CPI|BB_END)(\d+)(_\d+)?")
# section switches inside a function (a template instance sits in a comdat section of its own name, a plain
# kernel in .text): where the code is placed, not what it is
_SECTION = re.compile(r"^\s*\.(section|text)\b")
# what the summary line shows (every .amdhsa_ directive is compared)
_SHOWN = ("next_free_vgpr", "next_free_sgpr", "accum_offset", "group_segment_fixed_size",
          "private_segment_fixed_size", "kernarg_size")


def _strip(line: str) -> str:
    return line.split(";", 1)[0].rstrip()


def _normalise(body):
    """Local labels renumbered by first appearance within the function."""
    seen: dict = {}

    def num(m):
        key = (m.group(1), m.group(2))
        if key not in seen:
            seen[key] = len([k for k in seen if k[0] == m.group(1)])
        return f".L{m.group(1)}#{seen[key]}{m.group(3) or ''}"

    out = []
    for line in body:
        line = _LBB.sub(r".LBB#_\1", line)
        out.append(_LNUM.sub(num, line))
    return out


def parse(path: str):
    """-> ({symbol: [normalised body lines]}, {symbol: {directive: value}}), symbols in file order."""
    with open(path) as fh:
        lines = [_strip(l) for l in fh]
    funcs = [m.group(1) for m in map(_FUNC_TYPE.match, lines) if m]
    bodies: dict = {}
    meta: dict = {}
    cur = None
    kd = None
    for line in lines:
        if not line.strip():
            continue
        if kd is not None:
            if line.strip() == ".end_amdhsa_kernel":
                kd = None
            else:
                parts = line.split()
                meta[kd][parts[0].replace(".amdhsa_", "")] = " ".join(parts[1:])
            continue
        m = re.match(r"^\s*\.amdhsa_kernel\s+(\S+)", line)
        if m:
            kd = m.group(1)
            meta[kd] = {}
            continue
        if cur is None:
            m = _LABEL.match(line)
            if m and m.group(1) in funcs and m.group(1) not in bodies:
                cur = m.group(1)
                bodies[cur] = []
            continue
        if re.match(r"^\.Lfunc_end\d+:", line):
            bodies[cur] = _normalise(bodies[cur])
            cur = None
            continue
        if not _SECTION.match(line):
            bodies[cur].append(line)
    return bodies, meta


def _summary(md) -> str:
    return " ".join(f"{k}={md[k]}" for k in _SHOWN if k in md) if md else "(no kernel descriptor)"


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--map", action="append", default=[], metavar="OLD=NEW",
                    help="a symbol whose name changed (repeatable)")
    ap.add_argument("--context", type=int, default=6, help="differing lines shown per DIFF (default 6)")
    args = ap.parse_args()
    names = dict(m.split("=", 1) for m in args.map)
    old_b, old_m = parse(args.old)
    new_b, new_m = parse(args.new)
    print(f"# {args.old} -> {args.new}")
    status = 0
    matched = set()
    for sym, body in old_b.items():
        tgt = names.get(sym, sym)
        tag = sym if tgt == sym else f"{sym} -> {tgt}"
        if tgt not in new_b:
            print(f"GONE  {tag}\n      {_summary(old_m.get(sym))}")
            continue
        matched.add(tgt)
        nbody = [l.replace(tgt, sym) for l in new_b[tgt]] if tgt != sym else new_b[tgt]
        omd, nmd = old_m.get(sym, {}), new_m.get(tgt, {})
        dirs = [f"      .amdhsa_{k}: {omd.get(k)} -> {nmd.get(k)}" for k in sorted(set(omd) | set(nmd))
                if omd.get(k) != nmd.get(k)]
        if body == nbody and not dirs:
            print(f"same  {tag}\n      {_summary(nmd)} ({len(body)} lines)")
            continue
        status = 1
        print(f"DIFF  {tag}\n      old {_summary(omd)} ({len(body)} lines)\n      new {_summary(nmd)} ({len(nbody)} lines)")
        for d in dirs:
            print(d)
        shown = 0
        for i in range(max(len(body), len(nbody))):
            a = body[i] if i < len(body) else "<end>"
            b = nbody[i] if i < len(nbody) else "<end>"
            if a != b:
                print(f"      line {i + 1}:\n        - {a.strip()}\n        + {b.strip()}")
                shown += 1
                if shown >= args.context:
                    break
    for sym in new_b:
        if sym not in matched:
            print(f"NEW   {sym}\n      {_summary(new_m.get(sym))}")
    return status


if __name__ == "__main__":
    sys.exit(main())
