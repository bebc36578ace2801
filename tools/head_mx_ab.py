"""Measurement only: the server's work for one (client, micro-batch) part of dist.WideHub with an MX codec, as today's
four launches (slk_cutmx_decode, slk_wide_head's two kernels, slk_cutmx_encode) against slk_wide_head_mx's two, ONE
process, B = 4096, HIP events; prints one JSON line (stored as profiles/head_mx_ab.txt). The method is
tools/cutmx_ab.py's: every side sits between its own pair of events, behind a device-to-device copy that moves as many
bytes as that side reads plus writes (counted as in the README section: Wf, which stays in L2, is left out), the sides
are interleaved launch by launch, and each repeat reports new / old. Before timing, the two sides' outputs are compared
bit for bit at this size.

Pass 1 has two forms (csrc/slk_wide_head_mx.hip, SLK_HEAD_MX_STAGED): direct loads, and a wave-private LDS tile filled
by 16-byte loads. The product library holds the first; given a variant library built with the other,

  tools/build_variant.sh head_mx_staged "-DSLK_HEAD_MX_STAGED=1" && python tools/head_mx_ab.py build_abl/head_mx_staged.so

the variant's entry is a third side of every case, interleaved with the other two and compared with them bit for bit.

Not measured here: any multi-GPU time (the hub's links and the clients' waiting cannot be timed on one card), hardware
counters, other batch sizes.

usage: python tools/head_mx_ab.py [variant.so] [--repeats 7] [--launches 50]"""
import argparse
import ctypes
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "split-learning-k8s_amd"), ROOT]
from eval_bench import stats, time_each  # noqa: E402
from splitcnn import _lib  # noqa: E402
from splitcnn.codec import CUTMX_RECORD  # noqa: E402
from splitcnn.wide import KEEP_SCALE, KEEP_THRESHOLD  # noqa: E402

B, DENSE, KBITS = 4096, 32768, 2048
CASES = ((0, 0), (1, 1), (0, -1))
WIDTH = {0: CUTMX_RECORD["e2m1"], 1: CUTMX_RECORD["e4m3"], -1: DENSE}


def variant_entry(path):
    """slk_wide_head_mx of another build of the library, with the product binding's argument types."""
    fn = ctypes.CDLL(path).slk_wide_head_mx
    fn.argtypes, fn.restype = _lib._SIGS["slk_wide_head_mx"], ctypes.c_int
    return fn


def sides(dev, fin, fout, other=None):
    """(old, new, new of the variant build or None, bytes_old, bytes_new, outputs): callables on their own buffers."""
    s = torch.cuda.current_stream().cuda_stream
    g = torch.Generator().manual_seed(0)
    x = torch.randn(B, 16384, generator=g).relu_().to(torch.bfloat16).to(dev)
    rec = torch.empty((B, WIDTH[fin]), dtype=torch.uint8, device=dev)
    _lib.call("slk_cutmx_encode", x.data_ptr(), B, fin, rec.data_ptr(), s)
    wf8 = (torch.randn(163840, generator=g) * 0.02).to(dev)
    bf = torch.zeros(10, device=dev)
    y = torch.randint(0, 10, (B,), generator=g).to(dev)
    step = torch.zeros(1, dtype=torch.int32, device=dev)
    nslab = _lib.query("slk_wide_head_nslab", B)

    def outs(nwork):
        o = {k: torch.empty(shape, device=dev) for k, shape in
             (("logits", (B, 10)), ("loss", (B,)), ("dl", (B, 10)), ("slabs", (nslab, 163850)), ("work", (nwork,)))}
        o["out"] = (torch.empty((B, 16384), dtype=torch.bfloat16, device=dev) if fout < 0 else
                    torch.empty((B, WIDTH[fout]), dtype=torch.uint8, device=dev))
        o["flags"] = torch.zeros(2, dtype=torch.int32, device=dev)
        return o

    a, n = outs(_lib.query("slk_wide_head_work", B)), outs(_lib.query("slk_wide_head_mx_work", B))
    v = outs(_lib.query("slk_wide_head_mx_work", B)) if other else None
    cut = torch.empty_like(x)
    dcut = a["out"] if fout < 0 else torch.empty_like(x)
    head = lambda o: (step.data_ptr(), 0, KEEP_THRESHOLD, KEEP_SCALE, 1.0 / B, o["logits"].data_ptr(),  # noqa: E731
                      o["loss"].data_ptr(), o["dl"].data_ptr())

    def old():
        _lib.call("slk_cutmx_decode", rec.data_ptr(), B, fin, cut.data_ptr(), a["flags"][1:].data_ptr(), s)
        _lib.call("slk_wide_head", cut.data_ptr(), wf8.data_ptr(), bf.data_ptr(), y.data_ptr(), *head(a), dcut.data_ptr(),
                  a["slabs"].data_ptr(), a["work"].data_ptr(), a["flags"].data_ptr(), 0, B, s)
        if fout >= 0:
            _lib.call("slk_cutmx_encode", dcut.data_ptr(), B, fout, a["out"].data_ptr(), s)

    def mx_args(o):
        return (rec.data_ptr(), fin, wf8.data_ptr(), bf.data_ptr(), y.data_ptr(), *head(o), o["out"].data_ptr(), fout,
                o["slabs"].data_ptr(), o["work"].data_ptr(), o["flags"].data_ptr(), o["flags"][1:].data_ptr(), 0, B, s)

    def new():
        _lib.call("slk_wide_head_mx", *mx_args(n))

    def new_other():
        assert other(*mx_args(v)) == 0

    b_old = B * ((WIDTH[fin] + DENSE) + (2 * DENSE + KBITS) + (DENSE + KBITS) + (DENSE + WIDTH[fout] if fout >= 0 else 0))
    b_new = B * ((WIDTH[fin] + WIDTH[fout] + KBITS) + (WIDTH[fin] + KBITS))
    return old, new, new_other if other else None, b_old, b_new, (a, n, v)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("variant", nargs="?", help="a library built with the other pass-1 form (tools/build_variant.sh)")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--launches", type=int, default=50)
    args = ap.parse_args()
    R, N = max(args.repeats, 3), max(args.launches, 20)
    dev = torch.device("cuda:0")
    other = variant_entry(args.variant) if args.variant else None
    form = lambda staged: "LDS tile (staged)" if staged else "direct loads"  # noqa: E731
    defines = open(os.path.splitext(args.variant)[0] + ".defines").read().split() if args.variant else []
    staged = "-DSLK_HEAD_MX_STAGED=1" in defines
    out = {"tool": "head_mx_ab", "B": B, "repeats": R, "launches_per_repeat": N,
           "pass1_form_of_new": form(not staged) if other else "the product library's",
           "pass1_form_of_new_variant": form(staged) if other else "no variant given: not measured",
           "multi_gpu": "not measured (one card)"}
    fns, meta = {}, {}
    for fin, fout in CASES:
        tag = f"in{fin}_out{fout}"
        old, new, new_other, b_old, b_new, (a, n, v) = sides(dev, fin, fout, other)
        old(), new()
        if other:
            new_other()
        torch.cuda.synchronize()
        meta[tag] = {"bytes_old": b_old, "bytes_new": b_new, "bytes_new_over_old": round(b_new / b_old, 4),
                     "outputs_bitwise_equal": all(torch.equal(a[k].view(torch.uint8), n[k].view(torch.uint8))
                                                  for k in ("logits", "loss", "dl", "slabs", "out", "flags"))}
        if other:
            meta[tag]["variant_outputs_bitwise_equal"] = all(
                torch.equal(v[k].view(torch.uint8), n[k].view(torch.uint8)) for k in (*a, ) if k != "work")
        for name, fn, nbytes in (("old", old, b_old), ("new", new, b_new), ("new_variant", new_other, b_new)):
            if fn is None:
                continue
            src = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev)
            dst = torch.empty_like(src)
            fns[f"{tag}_{name}_copy"] = lambda src=src, dst=dst: dst.copy_(src)
            fns[f"{tag}_{name}"] = fn
    for fn in fns.values():
        for _ in range(3):
            fn()
    reps = [time_each(fns, N) for _ in range(R)]
    for tag, m in meta.items():
        ratios = [r[tag + "_new"] / r[tag + "_old"] for r in reps]
        olds = stats([r[tag + "_old"] for r in reps])
        news = stats([r[tag + "_new"] for r in reps])
        m.update({"old_four_launches": olds, "new_two_launches": news,
                  "old_copy_of_the_same_bytes": stats([r[tag + "_old_copy"] for r in reps]),
                  "new_copy_of_the_same_bytes": stats([r[tag + "_new_copy"] for r in reps]),
                  "new_over_old_per_repeat": [round(v, 4) for v in ratios],
                  "new_over_old_median": round(sorted(ratios)[len(ratios) // 2], 4),
                  "new_leaves_the_old_repeat_range": news["max_ms"] < olds["min_ms"] or news["min_ms"] > olds["max_ms"]})
        if other:
            vr = [r[tag + "_new_variant"] / r[tag + "_new"] for r in reps]
            m.update({"new_variant_two_launches": stats([r[tag + "_new_variant"] for r in reps]),
                      "variant_over_new_per_repeat": [round(x, 4) for x in vr],
                      "variant_over_new_median": round(sorted(vr)[len(vr) // 2], 4)})
    out["cases"] = meta
    print(json.dumps(out))


if __name__ == "__main__":
    main()
