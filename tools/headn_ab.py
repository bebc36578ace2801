"""Measurement only: the n-class K5 head (csrc/slk_wide_headn.hip) at nc = 100 and at nc = 10, next to the 10-class
head (slk_wide_head), ONE process, B = 4096, HIP events; prints one JSON line (stored as profiles/headn_ab.txt). The
method is tools/head_mx_ab.py's: every entry sits between its own pair of events, behind a device-to-device copy that
moves as many bytes as that entry reads plus writes (each operand counted once: re-reads of wq and dlq that stay in L2
are left out), all sides are interleaved launch by launch, and each repeat reports its own means. Before timing, the
n-class head at nc = 10 is compared with the 10-class head on the same operands (not bit for bit: it reads bf16
weights and bf16 dlogits; the largest differences are reported).

The entries are the granularity: slk_wide_headn_fwd is two kernels (split-K logits, cross-entropy) and
slk_wide_headn_bwd three (bf16 dlogits, cut gradient, weight gradient); the kernels of one entry cannot be launched
apart from outside, so which KERNEL of an entry dominates is not measured here. Not measured: other batch sizes,
hardware counters, the step with the client in it.

usage: python tools/headn_ab.py [--repeats 7] [--launches 30]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "split-learning-k8s_amd"), ROOT]
from eval_bench import stats, time_each  # noqa: E402
from splitcnn import _lib, ops  # noqa: E402
from splitcnn.wide import KEEP_SCALE, KEEP_THRESHOLD  # noqa: E402

B, CUTB, WQB = 4096, 32768, 2 * 128 * 16384 * 2
DROP = (0, KEEP_THRESHOLD, KEEP_SCALE)


def operands(dev, nc):
    g = torch.Generator().manual_seed(nc)
    cut = torch.randn(B, 16384, generator=g).relu_().to(torch.bfloat16).to(dev)
    wf = (torch.randn(nc * 16384, generator=g) * 0.02).to(dev)
    return cut, wf, torch.zeros(nc, device=dev), torch.randint(0, nc, (B,), generator=g).to(dev)


def headn_sides(dev, nc):
    """{name: (callable, bytes)} of the n-class head's three entries, and its outputs."""
    cut, wf, bf, y = operands(dev, nc)
    step, err = torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    wq = torch.empty(ops.HEADN_WQ_ELEMS, dtype=torch.bfloat16, device=dev)
    nslab, width = ops.wide_headn_nslab(B), nc * 16384 + nc
    o = {"logits": torch.empty((B, nc), device=dev), "loss": torch.empty(B, device=dev),
         "dl": torch.empty((B, nc), device=dev), "dcut": torch.empty_like(cut),
         "slabs": torch.empty((nslab, width), device=dev)}
    work = torch.empty(ops.wide_headn_work(B), device=dev)
    sides = {
        "shadow": (lambda: ops.wide_fcn_shadow(wf, nc, wq), 4 * nc * 16384 + WQB),
        "fwd": (lambda: ops.wide_headn_fwd(cut, wq, bf, nc, y, step, *DROP, 1.0 / B, o["logits"], work, loss_i=o["loss"],
                                           dlogits=o["dl"], err_flag=err), B * CUTB + WQB // 2 + 2 * B * 4096 + 8 * B * nc),
        "bwd": (lambda: ops.wide_headn_bwd(cut, wq, o["dl"], nc, step, *DROP, o["dcut"], o["slabs"], work),
                2 * B * CUTB + WQB // 2 + 4 * B * nc + 4 * nslab * width),
    }
    return sides, o, (cut, wf, bf, y)


def head10_sides(dev, ops10):
    cut, wf, bf, y = ops10
    s = torch.cuda.current_stream().cuda_stream
    step, err = torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    wf8 = torch.empty(163840, device=dev)
    nslab = _lib.query("slk_wide_head_nslab", B)
    o = {"logits": torch.empty((B, 10), device=dev), "loss": torch.empty(B, device=dev), "dl": torch.empty((B, 10), device=dev),
         "dcut": torch.empty_like(cut), "slabs": torch.empty((nslab, 163850), device=dev)}
    work = torch.empty(_lib.query("slk_wide_head_work", B), device=dev)
    sides = {
        "shadow": (lambda: _lib.call("slk_wide_fc_shadow", wf.data_ptr(), wf8.data_ptr(), s), 2 * 4 * 163840),
        "head": (lambda: _lib.call("slk_wide_head", cut.data_ptr(), wf8.data_ptr(), bf.data_ptr(), y.data_ptr(),
                                   step.data_ptr(), *DROP, 1.0 / B, o["logits"].data_ptr(), o["loss"].data_ptr(),
                                   o["dl"].data_ptr(), o["dcut"].data_ptr(), o["slabs"].data_ptr(), work.data_ptr(),
                                   err.data_ptr(), 0, B, s), 3 * B * CUTB + 2 * B * 2048 + 4 * nslab * 163850),
    }
    return sides, o


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--launches", type=int, default=30)
    args = ap.parse_args()
    R, N = max(args.repeats, 3), max(args.launches, 10)
    dev = torch.device("cuda:0")
    groups = {}
    groups["headn_nc100"], _, _ = headn_sides(dev, 100)
    groups["headn_nc10"], on, ops10 = headn_sides(dev, 10)
    groups["head10"], oo = head10_sides(dev, ops10)
    fns, nbytes = {}, {}
    for gname, sides in groups.items():
        for name, (fn, nb) in sides.items():
            src = torch.empty(nb // 2, dtype=torch.uint8, device=dev)
            dst = torch.empty_like(src)
            fns[f"{gname}_{name}_copy"] = lambda src=src, dst=dst: dst.copy_(src)
            fns[f"{gname}_{name}"] = fn
            nbytes[f"{gname}_{name}"] = nb
    for fn in fns.values():   # in order: a shadow before its head, a fwd before its bwd
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    red = lambda t: ops.reduce_slabs(t).double()  # noqa: E731
    out = {"tool": "headn_ab", "B": B, "repeats": R, "launches_per_repeat": N,
           "headn_nc10_vs_head10_max_abs_difference": {
               "logits": float((on["logits"] - oo["logits"]).abs().max()), "loss": float((on["loss"] - oo["loss"]).abs().max()),
               "dcut": float((on["dcut"].float() - oo["dcut"].float()).abs().max()),
               "grad": float((red(on["slabs"]) - red(oo["slabs"])).abs().max()),
               "grad_max_abs": float(red(oo["slabs"]).abs().max())},
           "slabs": {"headn": ops.wide_headn_nslab(B), "head10": _lib.query("slk_wide_head_nslab", B)}}
    reps = [time_each(fns, N) for _ in range(R)]
    entries = {}
    for k, nb in nbytes.items():
        t, c = stats([r[k] for r in reps]), stats([r[k + "_copy"] for r in reps])
        entries[k] = {"bytes": nb, "entry": t, "copy_of_the_same_bytes": c,
                      "entry_over_copy_median": round(t["median_ms"] / c["median_ms"], 3)}
    out["entries"] = entries
    tot = lambda g: [sum(r[f"{g}_{n}"] for n in groups[g]) for r in reps]  # noqa: E731
    out["totals_ms"] = {g: stats(tot(g)) for g in groups}
    for g in ("headn_nc100", "headn_nc10"):
        ratios = [a / b for a, b in zip(tot(g), tot("head10"))]
        out[f"{g}_over_head10_per_repeat"] = [round(v, 3) for v in ratios]
        out[f"{g}_dominant_entry"] = max(groups[g], key=lambda n: entries[f"{g}_{n}"]["entry"]["median_ms"])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
