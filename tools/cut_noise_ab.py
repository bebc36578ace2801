"""Measurement only: what privacy.CutNoise costs on one GPU, ONE process, B = 4096, HIP events; prints one JSON line
(stored as profiles/cut_noise_ab.txt).

  launches: slk_cut_noise over 4096 samples — clip + Laplace, clip + Gaussian, Laplace without a clip, the clip alone
            (evaluation) — and slk_cut_scale_rows, eager, each between its own pair of HIP events and each behind a
            device-to-device copy that moves as many bytes as the launch reads plus writes (copy_(n) moves n bytes in
            and n out: the copy's tensor holds half the launch's bytes), next to slk_cut8_roundtrip (e4m3) of the same
            repeat as a second yardstick: the same bytes and the same one-block-per-sample skeleton. Reported per repeat
            as launch / copy and launch / roundtrip;
  step:     the graphed K5 step (default Adam) plain and with cut_noise=CutNoise("laplace", 0.1, clip=30) on registered
            input buffers, interleaved repeat by repeat, with a second plain trainer as the control: the noised step is
            reported against the plain step of the same process and that step's own repeat range.

Not measured here: accuracy on real CIFAR-10, any attack's success, any multi-GPU time.

usage: python tools/cut_noise_ab.py [--repeats 7] [--steps 100] [--launches 50]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "split-learning-k8s_amd"), ROOT]
from eval_bench import stats, time_each, time_loop  # noqa: E402
from splitcnn.codec import Fp8Cut  # noqa: E402
from splitcnn.privacy import NOISE_SAMPLE, CutNoise  # noqa: E402

B = 4096


def launch_times(dev, R, N):
    g = torch.Generator().manual_seed(0)
    x = torch.randn(B, 32, 8, 8, 8, generator=g).relu_().to(torch.bfloat16).to(dev)   # a ReLU cut's shape of data
    out = torch.empty_like(x)
    st = torch.empty(B, 2, device=dev)
    ctr = torch.full((1,), 3, dtype=torch.int32, device=dev)
    moved = 2 * B * NOISE_SAMPLE * 2        # every launch reads the rows once and writes them once
    lap, gau = CutNoise("laplace", 0.1, clip=30.0, seed=1), CutNoise("gaussian", 0.1, clip=30.0, seed=1)
    bare, codec = CutNoise("laplace", 0.1, seed=1), Fp8Cut()
    lap.apply(x, out, ctr, stats=st)        # st holds the coefficients slk_cut_scale_rows reads
    src = torch.empty(moved // 2, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    fns = {"clip_laplace": lambda: lap.apply(x, out, ctr, stats=st),
           "clip_gaussian": lambda: gau.apply(x, out, ctr, stats=st),
           "laplace_no_clip": lambda: bare.apply(x, out, ctr),
           "clip_only": lambda: lap.apply(x, out, noise=False, stats=st),
           "scale_rows": lambda: lap.scale_rows(x, st, out),
           "cut8_roundtrip": lambda: codec.roundtrip(x, out, "fwd"),
           "copy": lambda: dst.copy_(src)}
    for fn in fns.values():
        for _ in range(3):
            fn()
    reps = [time_each(fns, N) for _ in range(R)]
    res = {"bytes_read_plus_written": moved}
    for name in fns:
        res[name] = stats([r[name] for r in reps])
        if name not in ("copy", "cut8_roundtrip"):
            res[name + "_over_copy_per_repeat"] = [round(r[name] / r["copy"], 3) for r in reps]
            res[name + "_over_roundtrip_per_repeat"] = [round(r[name] / r["cut8_roundtrip"], 3) for r in reps]
    res["cut8_roundtrip_over_copy_per_repeat"] = [round(r["cut8_roundtrip"] / r["copy"], 3) for r in reps]
    return res


def step_times(dev, R, N):
    from splitcnn.wide import SyntheticCIFAR, WideTrainer, init_wide_models
    data = SyntheticCIFAR(42)
    xs, ys = zip(*(data.batch(B) for _ in range(2)))
    X, Y = torch.stack(xs).to(dev), torch.stack(ys).to(dev)
    mk = lambda q: WideTrainer(*init_wide_models(seed=0), device=dev, graph=True, cut_noise=q)  # noqa: E731
    trs = [mk(None), mk(CutNoise("laplace", 0.1, clip=30.0, seed=1)), mk(None)]
    for tr in trs:
        for i in range(2):
            tr.register_inputs(X[i], Y[i])
        for i in range(4):
            tr.step(X[i % 2], Y[i % 2])
    plain, noised, control = trs
    d, n, c = [], [], []
    for _ in range(R):
        d.append(time_loop(lambda i: plain.step(X[i % 2], Y[i % 2]), N))
        n.append(time_loop(lambda i: noised.step(X[i % 2], Y[i % 2]), N))
        c.append(time_loop(lambda i: control.step(X[i % 2], Y[i % 2]), N))
    sd, sn, sc = stats(d), stats(n), stats(c)
    coef = noised.cut_stats()[:, 1]
    return {"config": "default Adam(1e-3); noised " + repr(noised.cut_noise),
            "plain_step": sd, "noised_step": sn, "control_plain_step": sc,
            "plain_repeat_range_ms": round(sd["max_ms"] - sd["min_ms"], 4),
            "noised_minus_plain_median_ms": round(sn["median_ms"] - sd["median_ms"], 4),
            "control_minus_plain_median_ms": round(sc["median_ms"] - sd["median_ms"], 4),
            "noised_over_plain_per_repeat": [round(b / a, 4) for a, b in zip(d, n)],
            "control_over_plain_per_repeat": [round(b / a, 4) for a, b in zip(d, c)],
            "launches_added": ["slk_cut_noise", "slk_cut_scale_rows"],
            "last_step_fraction_of_rows_clipped": round(float((coef < 1).float().mean()), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--launches", type=int, default=50)
    args = ap.parse_args()
    R, N, L = max(args.repeats, 3), max(args.steps, 20), max(args.launches, 20)
    dev = torch.device("cuda:0")
    out = {"tool": "cut_noise_ab", "B": B, "repeats": R, "steps_per_repeat": N, "launches_per_repeat": L}
    out["launch_ms"] = launch_times(dev, R, L)
    out["k5_step"] = step_times(dev, R, N)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
