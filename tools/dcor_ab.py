#!/usr/bin/env python3
"""privacy.distance_correlation against the same statistic built from torch.cdist, on one device in one process.

    python tools/dcor_ab.py [--batch 4096] [--repeats 7] [--out profiles/dcor_ab.txt]

The inputs are a seeded batch and the seeded K5 model's step-0 cut of it. The two forms alternate, every launch between
its own HIP events; the torch form gets the bf16 cut upcast to float32 (the upcast is not timed). Reported: the medians
and ranges, torch's peak extra memory, both results, and the z loop's executed bf16 FLOPs over the WHOLE metric's time
as a fraction of the bf16 MFMA peak (a lower bound of the loop's own fraction: no counters are read)."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "split-learning-k8s_amd"))
BF16_PEAK = 2.5e15   # dense bf16 MFMA FLOP/s of one MI355X (vendor figure)


def torch_dcor(x, z):
    """The biased statistic from two cdist matrices (no resolution rule)."""
    a, b = torch.cdist(x, x), torch.cdist(z, z)
    n = x.shape[0]

    def dcov2(p, q):
        return (p * q).sum() / n ** 2 - 2 * (p.sum(1) * q.sum(1)).sum() / n ** 3 + p.sum() * q.sum() / n ** 4
    cov, vx, vz = dcov2(a, b), dcov2(a, a), dcov2(b, b)
    return torch.stack([(cov.clamp(min=0) / (vx * vz).sqrt()).sqrt(), cov, vx, vz])


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "dcor_ab.py needs a ROCm GPU"
    from splitcnn import privacy
    from splitcnn.wide import WideTrainer, init_wide_models
    B = args.batch
    x = torch.randn(B, 3, 32, 32, generator=torch.Generator().manual_seed(0)).cuda()
    tr = WideTrainer(*init_wide_models(seed=0), device="cuda", graph=False)
    tr.cut_leakage(x)
    z = tr.eval_cut.clone()
    xf, zf = x.view(B, -1), z.view(B, -1).float()
    for _ in range(2):   # warm both forms
        ours, theirs = privacy.distance_correlation(x, z).values.clone(), torch_dcor(xf, zf)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    t_ours, t_torch = [], []
    for _ in range(args.repeats):
        t_ours.append(timed(lambda: privacy.distance_correlation(x, z))[0])
        t_torch.append(timed(lambda: torch_dcor(xf, zf))[0])
    peak = torch.cuda.max_memory_allocated() - base
    T = (B + 127) // 128
    z_flops = T * (T + 1) // 2 * 128 * 128 * zf.shape[1] * 2
    m_ours, m_torch = statistics.median(t_ours), statistics.median(t_torch)
    lines = [
        f"distance correlation at B = {B}, dx = {xf.shape[1]}, dz = {zf.shape[1]}; {args.repeats} interleaved repeats, ms",
        f"slk_dcor      median {m_ours:.3f}  range {min(t_ours):.3f} .. {max(t_ours):.3f}",
        f"torch.cdist   median {m_torch:.3f}  range {min(t_torch):.3f} .. {max(t_torch):.3f}   "
        f"peak extra memory {peak / 2 ** 20:.1f} MiB",
        f"slk_dcor workspace {privacy.ops.dcor_workspace_bytes(B) / 2 ** 20:.2f} MiB",
        f"results (dcor, dcov2, dvar_x, dvar_z): slk_dcor {ours.tolist()}  torch {theirs.tolist()}",
        f"z loop: {z_flops / 1e9:.1f} GFLOP executed; over the whole metric's median time that is "
        f"{z_flops / (m_ours * 1e-3) / 1e12:.1f} TFLOP/s, {100 * z_flops / (m_ours * 1e-3) / BF16_PEAK:.1f} % of the "
        f"{BF16_PEAK / 1e12:.0f} TFLOP/s bf16 peak (lower bound of the loop's own fraction)",
    ]
    print("\n".join(lines))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
