"""Measurement only: what codec.Fp8Cut costs on one GPU, ONE process, B = 4096, HIP events; prints one JSON line (stored
as profiles/cut8_ab.txt).

  launches: slk_cut8_encode / slk_cut8_decode / slk_cut8_roundtrip over 4096 samples, per format, eager, each between
            its own pair of HIP events and each behind a device-to-device copy that moves as many bytes as the launch
            reads plus writes (copy_(n) moves n bytes in and n out: the copy's tensor holds half the launch's bytes);
            reported per repeat as launch / copy;
  step:     the graphed K5 step (default Adam) without and with cut_codec=Fp8Cut() on registered input buffers,
            interleaved repeat by repeat, with a second plain trainer as the control: the step with the codec is
            reported against the plain step of the same process and that step's own repeat range.

Not measured here: accuracy on real CIFAR-10, any multi-GPU time, whether the K5 exchange is link-bound at all.

usage: python tools/cut8_ab.py [--repeats 7] [--steps 100] [--launches 50]"""
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
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    res = {}
    dense, recb = B * CUT8_SAMPLE * 2, B * CUT8_RECORD
    moved = {"encode": dense + recb, "decode": recb + dense, "roundtrip": 2 * dense}
    for fmt, d in (("e4m3", "fwd"), ("e5m2", "bwd")):
        q = Fp8Cut(fwd="e4m3", bwd="e5m2")
        rec = q.records("ab", B, dev)
        q.encode(x, rec, d)
        fns = {}
        for name, fn in (("encode", lambda q=q, d=d, rec=rec: q.encode(x, rec, d)),
                         ("decode", lambda q=q, d=d, rec=rec: q.decode(rec, out, err, d)),
                         ("roundtrip", lambda q=q, d=d: q.roundtrip(x, out, d))):
            src = torch.empty(moved[name] // 2, dtype=torch.uint8, device=dev)
            dst = torch.empty_like(src)
            fns[name] = fn
            fns[f"{name}_copy"] = lambda src=src, dst=dst: dst.copy_(src)
        for fn in fns.values():
            for _ in range(3):
                fn()
        reps = [time_each(fns, N) for _ in range(R)]
        res[fmt] = {}
        for name in ("encode", "decode", "roundtrip"):
            res[fmt][name] = {"bytes_read_plus_written": moved[name],
                              "launch": stats([r[name] for r in reps]),
                              "copy_of_the_same_bytes": stats([r[name + "_copy"] for r in reps]),
                              "launch_over_copy_per_repeat": [round(r[name] / r[name + "_copy"], 3) for r in reps]}
        assert int(err.item()) == 0
    return res


def step_times(dev, R, N):
    from splitcnn.wide import SyntheticCIFAR, WideTrainer, init_wide_models
    data = SyntheticCIFAR(42)
    xs, ys = zip(*(data.batch(B) for _ in range(2)))
    X, Y = torch.stack(xs).to(dev), torch.stack(ys).to(dev)
    mk = lambda **kw: WideTrainer(*init_wide_models(seed=0), device=dev, graph=True, **kw)  # noqa: E731
    trs = [mk(), mk(cut_codec=Fp8Cut()), mk()]
    for tr in trs:
        for i in range(2):
            tr.register_inputs(X[i], Y[i])
        for i in range(4):
            tr.step(X[i % 2], Y[i % 2])
    plain, coded, control = trs
    d, n, c = [], [], []
    for _ in range(R):
        d.append(time_loop(lambda i: plain.step(X[i % 2], Y[i % 2]), N))
        n.append(time_loop(lambda i: coded.step(X[i % 2], Y[i % 2]), N))
        c.append(time_loop(lambda i: control.step(X[i % 2], Y[i % 2]), N))
    sd, sn, sc = stats(d), stats(n), stats(c)
    return {"config": "default Adam(1e-3), " + repr(coded.cut_codec),
            "plain_step": sd, "cut_codec_step": sn, "control_plain_step": sc,
            "plain_repeat_range_ms": round(sd["max_ms"] - sd["min_ms"], 4),
            "codec_minus_plain_median_ms": round(sn["median_ms"] - sd["median_ms"], 4),
            "control_minus_plain_median_ms": round(sc["median_ms"] - sd["median_ms"], 4),
            "codec_over_plain_per_repeat": [round(b / a, 4) for a, b in zip(d, n)],
            "control_over_plain_per_repeat": [round(b / a, 4) for a, b in zip(d, c)],
            "plain_samples_per_s": round(B / (sd["median_ms"] * 1e-3)),
            "codec_samples_per_s": round(B / (sn["median_ms"] * 1e-3))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--launches", type=int, default=50)
    args = ap.parse_args()
    R, N, L = max(args.repeats, 3), max(args.steps, 20), max(args.launches, 20)
    dev = torch.device("cuda:0")
    out = {"tool": "cut8_ab", "B": B, "repeats": R, "steps_per_repeat": N, "launches_per_repeat": L,
           "bytes_per_sample_and_direction": {"fp8_record": CUT8_RECORD, "dense_bf16": 2 * CUT8_SAMPLE}}
    out["launch_ms"] = launch_times(dev, R, L)
    out["k5_step"] = step_times(dev, R, N)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
