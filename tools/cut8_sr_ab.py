"""Measurement only: what stochastic rounding adds to codec.Fp8Cut on one GPU, ONE process, B = 4096, HIP events; prints
one JSON line (stored as profiles/cut8_sr_ab.txt).

  launches: slk_cut8_encode_sr / slk_cut8_roundtrip_sr over 4096 samples, per format, eager, next to their nearest twins
            slk_cut8_encode / slk_cut8_roundtrip, each between its own pair of HIP events and each behind a
            device-to-device copy that moves as many bytes as the launch reads plus writes (copy_(n) moves n bytes in
            and n out: the copy's tensor holds half the launch's bytes); reported per repeat as sr / nearest and
            launch / copy;
  step:     the graphed K5 step (default Adam) with cut_codec=Fp8Cut() and with Fp8Cut(rounding={"bwd": "stochastic"})
            on registered input buffers, interleaved repeat by repeat, with a second Fp8Cut() trainer as the control:
            the stochastic step is reported against the nearest step of the same process and that step's own repeat
            range.

Not measured here: accuracy on real CIFAR-10, any multi-GPU time.

usage: python tools/cut8_sr_ab.py [--repeats 7] [--steps 100] [--launches 50]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "split-learning-k8s_amd"), ROOT]
from eval_bench import stats, time_each, time_loop  # noqa: E402
from splitcnn.codec import CUT8_RECORD, CUT8_SAMPLE, Fp8Cut  # noqa: E402

B = 4096


def launch_times(dev, R, N):
    g = torch.Generator().manual_seed(0)
    x = torch.randn(B, 32, 8, 8, 8, generator=g).relu_().to(torch.bfloat16).to(dev)   # a ReLU cut's shape of data
    out = torch.empty_like(x)
    ctr = torch.full((1,), 3, dtype=torch.int32, device=dev)
    res = {}
    dense, recb = B * CUT8_SAMPLE * 2, B * CUT8_RECORD
    moved = {"encode": dense + recb, "roundtrip": 2 * dense}
    near, sr = Fp8Cut(), Fp8Cut(rounding="stochastic", seed=1)
    for fmt, d in (("e4m3", "fwd"), ("e5m2", "bwd")):
        rec = near.records("ab", B, dev)
        fns = {}
        for name, q, kw in (("encode", near, {}), ("encode_sr", sr, {"step": ctr}),
                            ("roundtrip", near, {}), ("roundtrip_sr", sr, {"step": ctr})):
            src = torch.empty(moved[name.replace("_sr", "")] // 2, dtype=torch.uint8, device=dev)
            dst = torch.empty_like(src)
            if name.startswith("encode"):
                fns[name] = lambda q=q, kw=kw: q.encode(x, rec, d, **kw)
            else:
                fns[name] = lambda q=q, kw=kw: q.roundtrip(x, out, d, **kw)
            fns[f"{name}_copy"] = lambda src=src, dst=dst: dst.copy_(src)
        for fn in fns.values():
            for _ in range(3):
                fn()
        reps = [time_each(fns, N) for _ in range(R)]
        res[fmt] = {}
        for name in ("encode", "roundtrip"):
            res[fmt][name] = {"bytes_read_plus_written": moved[name],
                              "nearest": stats([r[name] for r in reps]),
                              "stochastic": stats([r[name + "_sr"] for r in reps]),
                              "copy_of_the_same_bytes": stats([r[name + "_copy"] for r in reps]),
                              "stochastic_over_nearest_per_repeat": [round(r[name + "_sr"] / r[name], 3) for r in reps],
                              "nearest_over_copy_per_repeat": [round(r[name] / r[name + "_copy"], 3) for r in reps],
                              "stochastic_over_copy_per_repeat": [round(r[name + "_sr"] / r[name + "_sr_copy"], 3) for r in reps]}
    return res


def step_times(dev, R, N):
    from splitcnn.wide import SyntheticCIFAR, WideTrainer, init_wide_models
    data = SyntheticCIFAR(42)
    xs, ys = zip(*(data.batch(B) for _ in range(2)))
    X, Y = torch.stack(xs).to(dev), torch.stack(ys).to(dev)
    mk = lambda q: WideTrainer(*init_wide_models(seed=0), device=dev, graph=True, cut_codec=q)  # noqa: E731
    trs = [mk(Fp8Cut()), mk(Fp8Cut(rounding={"bwd": "stochastic"})), mk(Fp8Cut())]
    for tr in trs:
        for i in range(2):
            tr.register_inputs(X[i], Y[i])
        for i in range(4):
            tr.step(X[i % 2], Y[i % 2])
    near, sr, control = trs
    d, n, c = [], [], []
    for _ in range(R):
        d.append(time_loop(lambda i: near.step(X[i % 2], Y[i % 2]), N))
        n.append(time_loop(lambda i: sr.step(X[i % 2], Y[i % 2]), N))
        c.append(time_loop(lambda i: control.step(X[i % 2], Y[i % 2]), N))
    sd, sn, sc = stats(d), stats(n), stats(c)
    return {"config": "default Adam(1e-3); nearest " + repr(near.cut_codec) + "; stochastic " + repr(sr.cut_codec),
            "nearest_codec_step": sd, "stochastic_bwd_step": sn, "control_nearest_codec_step": sc,
            "nearest_repeat_range_ms": round(sd["max_ms"] - sd["min_ms"], 4),
            "stochastic_minus_nearest_median_ms": round(sn["median_ms"] - sd["median_ms"], 4),
            "control_minus_nearest_median_ms": round(sc["median_ms"] - sd["median_ms"], 4),
            "stochastic_over_nearest_per_repeat": [round(b / a, 4) for a, b in zip(d, n)],
            "control_over_nearest_per_repeat": [round(b / a, 4) for a, b in zip(d, c)]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--launches", type=int, default=50)
    args = ap.parse_args()
    R, N, L = max(args.repeats, 3), max(args.steps, 20), max(args.launches, 20)
    dev = torch.device("cuda:0")
    out = {"tool": "cut8_sr_ab", "B": B, "repeats": R, "steps_per_repeat": N, "launches_per_repeat": L}
    out["launch_ms"] = launch_times(dev, R, L)
    out["k5_step"] = step_times(dev, R, N)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
