#!/usr/bin/env python3
"""The NoPeek term (privacy.DcorLoss, slk_dcor_grad) measured on one device in one process.

    python tools/nopeek_ab.py [--batch 4096] [--repeats 7] [--out profiles/nopeek_ab.txt]

Three measurements, the forms of each alternating over the repeats, every call between its own HIP events:
  * the graphed K5 step with and without leak_loss (two trainers from the same seed);
  * slk_dcor_grad on a seeded batch and the seeded model's step-0 cut, in nested forms instead of per launch (the entry
    has no way to stop early): the metric alone (launches 1-3), the entry at alpha = 0 (launches 1-5 and the product's
    epilogue, its K loop skipped) and the entry at alpha > 0 (all six);
  * the same term from torch autograd over two cdist calls, as the yardstick: time and peak extra memory.
Reported: medians and ranges in ms, and the product kernel's executed FLOPs (2 Np^2 dz) over the time its K loop adds
(the entry at alpha > 0 minus at alpha = 0) against the bf16 MFMA peak. No counters are read, so which resource bounds
the product is not determined here."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "split-learning-k8s_amd"))
BF16_PEAK = 2.5e15   # dense bf16 MFMA FLOP/s of one MI355X (vendor figure)


def torch_term(x, z, dcut, alpha):
    """dcut + alpha * d dCor^2 / d z by autograd through two cdist matrices (no resolution rule)."""
    z = z.detach().requires_grad_(True)
    a, b = torch.cdist(x, x), torch.cdist(z, z)
    n = x.shape[0]

    def dcov2(p, q):
        return (p * q).sum() / n ** 2 - 2 * (p.sum(1) * q.sum(1)).sum() / n ** 3 + p.sum() * q.sum() / n ** 4
    r2 = dcov2(a, b) / (dcov2(a, a) * dcov2(b, b)).sqrt()
    (g,) = torch.autograd.grad(alpha * r2, z)
    return (dcut.float() + g).to(torch.bfloat16)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def stat(name, ts, extra=""):
    return f"{name:<34s} median {statistics.median(ts):8.3f}  range {min(ts):8.3f} .. {max(ts):8.3f}{extra}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--alpha", type=float, default=1.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "nopeek_ab.py needs a ROCm GPU"
    from splitcnn import privacy
    from splitcnn.wide import WideTrainer, init_wide_models
    B = args.batch
    g = torch.Generator().manual_seed(0)
    x = torch.randn(B, 3, 32, 32, generator=g).cuda()
    y = torch.randint(0, 10, (B,), generator=g).cuda()
    plain = WideTrainer(*init_wide_models(seed=0), device="cuda", graph=True)
    leak = WideTrainer(*init_wide_models(seed=0), device="cuda", graph=True, leak_loss=privacy.DcorLoss(args.alpha))
    xs, ys = plain.static_inputs(B)
    xl, yl = leak.static_inputs(B)
    for t in (xs, xl):
        t.copy_(x)
    for t in (ys, yl):
        t.copy_(y)
    z = plain.client.forward(x, tag="eval").clone()
    dcut = (torch.randn(z.shape, generator=torch.Generator().manual_seed(1)) * 1e-3).to(torch.bfloat16).cuda()
    xf, zf = x.view(B, -1), z.view(B, -1).float()
    on, off, out = privacy.DcorLoss(args.alpha), privacy.DcorLoss(0.0), torch.empty_like(dcut)
    for _ in range(2):   # warm every form
        plain.step(xs, ys)
        leak.step(xl, yl)
        privacy.distance_correlation(x, z)
        on.add_grad(x, z, dcut, out=out)
        off.add_grad(x, z, dcut, out=out)
        torch_term(xf, zf, dcut.view(B, -1), args.alpha)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    t = {k: [] for k in ("plain", "leak", "metric", "off", "on", "torch")}
    for _ in range(args.repeats):
        t["plain"].append(timed(lambda: plain.step(xs, ys))[0])
        t["leak"].append(timed(lambda: leak.step(xl, yl))[0])
        t["metric"].append(timed(lambda: privacy.distance_correlation(x, z))[0])
        t["off"].append(timed(lambda: off.add_grad(x, z, dcut, out=out))[0])
        t["on"].append(timed(lambda: on.add_grad(x, z, dcut, out=out))[0])
        t["torch"].append(timed(lambda: torch_term(xf, zf, dcut.view(B, -1), args.alpha))[0])
    peak = torch.cuda.max_memory_allocated() - base
    Np = (B + 127) // 128 * 128
    flops = 2 * Np * Np * zf.shape[1]
    loop = statistics.median(t["on"]) - statistics.median(t["off"])
    lines = [
        f"NoPeek term at B = {B}, dx = {xf.shape[1]}, dz = {zf.shape[1]}, alpha = {args.alpha}; {args.repeats} "
        "interleaved repeats, ms",
        stat("graphed K5 step, leak_loss=None", t["plain"]),
        stat("graphed K5 step, leak_loss", t["leak"]),
        stat("slk_dcor (launches 1-3)", t["metric"]),
        stat("slk_dcor_grad, alpha = 0", t["off"], "   (launches 1-5 and the product's epilogue)"),
        stat("slk_dcor_grad, alpha > 0", t["on"], "   (all six launches)"),
        stat("torch autograd over two cdist", t["torch"], f"   peak extra memory {peak / 2 ** 20:.1f} MiB"),
        f"slk_dcor_grad workspace {privacy.ops.dcor_grad_workspace_bytes(B) / 2 ** 20:.2f} MiB "
        f"(U {2 * Np * Np / 2 ** 20:.0f} MiB)",
        f"product K loop: {flops / 1e9:.1f} GFLOP executed over the {loop:.3f} ms it adds = "
        f"{flops / (loop * 1e-3) / 1e12:.1f} TFLOP/s, {100 * flops / (loop * 1e-3) / BF16_PEAK:.1f} % of the "
        f"{BF16_PEAK / 1e12:.0f} TFLOP/s bf16 peak; which resource bounds it was not determined (no counters read)",
        f"last step's leak_stats: {leak.leak_stats()}",
    ]
    print("\n".join(lines))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
