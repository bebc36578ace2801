"""Measurement only: what codec.MxCut costs on one GPU next to codec.Fp8Cut, ONE process, B = 4096, HIP events; prints one
JSON line (stored as profiles/cutmx_ab.txt). The method is tools/cut8_ab.py's.

  launches: slk_cutmx_encode / _decode / _roundtrip in both formats and slk_cut8_encode / _decode / _roundtrip in both
            of theirs over 4096 samples, eager, each between its own pair of HIP events and each behind a
            device-to-device copy that moves as many bytes as the launch reads plus writes (copy_(n) moves n bytes in
            and n out: the copy's tensor holds half the launch's bytes); reported per repeat as launch / copy. The
            yardsticks are the copy and the FP8 launch, never the MX kernel itself;
  step:     the graphed K5 step (default Adam) plain, with cut_codec=Fp8Cut() and with cut_codec=MxCut() on registered
            input buffers, interleaved repeat by repeat, with a second plain trainer as the control;
  error:    the relative L2 error |x - roundtrip(x)| / |x| of each format on the seeded model's step-0 cut and cut
            gradient (B = 4096, synthetic CIFAR batch) — for information only: no claim and no threshold.

Not measured here: accuracy on real CIFAR-10, any multi-GPU time, hardware counters, other batch sizes.

usage: python tools/cutmx_ab.py [--repeats 7] [--steps 100] [--launches 50]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "split-learning-k8s_amd"), ROOT]
from eval_bench import stats, time_each, time_loop  # noqa: E402
from splitcnn.codec import CUT8_RECORD, CUT8_SAMPLE, CUTMX_RECORD, Fp8Cut, MxCut  # noqa: E402

B = 4096
CODECS = (("mx_e2m1", lambda: MxCut("e2m1", None), "fwd"), ("mx_e4m3", lambda: MxCut("e4m3", None), "fwd"),
          ("fp8_e4m3", lambda: Fp8Cut("e4m3", None), "fwd"), ("fp8_e5m2", lambda: Fp8Cut(None, "e5m2"), "bwd"))


def launch_times(dev, R, N):
    g = torch.Generator().manual_seed(0)
    x = torch.randn(B, 32, 8, 8, 8, generator=g).relu_().to(torch.bfloat16).to(dev)   # a ReLU cut's shape of data
    out = torch.empty_like(x)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    dense = B * CUT8_SAMPLE * 2
    fns, moved = {}, {}
    for tag, make, d in CODECS:
        q = make()
        recb = B * q.record_bytes(d)
        rec = q.records("ab", B, dev, direction=d)
        q.encode(x, rec, d)
        for name, fn, nbytes in (("encode", lambda q=q, d=d, rec=rec: q.encode(x, rec, d), dense + recb),
                                 ("decode", lambda q=q, d=d, rec=rec: q.decode(rec, out, err, d), recb + dense),
                                 ("roundtrip", lambda q=q, d=d: q.roundtrip(x, out, d), 2 * dense)):
            src = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev)
            dst = torch.empty_like(src)
            fns[f"{tag}_{name}"] = fn
            fns[f"{tag}_{name}_copy"] = lambda src=src, dst=dst: dst.copy_(src)
            moved[f"{tag}_{name}"] = nbytes
    for fn in fns.values():
        for _ in range(3):
            fn()
    reps = [time_each(fns, N) for _ in range(R)]
    assert int(err.item()) == 0
    res = {}
    for key, nbytes in moved.items():
        ratios = [r[key] / r[key + "_copy"] for r in reps]
        res[key] = {"bytes_read_plus_written": nbytes, "launch": stats([r[key] for r in reps]),
                    "copy_of_the_same_bytes": stats([r[key + "_copy"] for r in reps]),
                    "launch_over_copy_per_repeat": [round(v, 3) for v in ratios],
                    "launch_over_copy_median": round(sorted(ratios)[len(ratios) // 2], 3)}
    return res


def step_times(dev, R, N):
    from splitcnn.wide import SyntheticCIFAR, WideTrainer, init_wide_models
    data = SyntheticCIFAR(42)
    xs, ys = zip(*(data.batch(B) for _ in range(2)))
    X, Y = torch.stack(xs).to(dev), torch.stack(ys).to(dev)
    mk = lambda **kw: WideTrainer(*init_wide_models(seed=0), device=dev, graph=True, **kw)  # noqa: E731
    trs = {"plain": mk(), "fp8": mk(cut_codec=Fp8Cut()), "mx": mk(cut_codec=MxCut()), "control": mk()}
    for tr in trs.values():
        for i in range(2):
            tr.register_inputs(X[i], Y[i])
        for i in range(4):
            tr.step(X[i % 2], Y[i % 2])
    t = {k: [] for k in trs}
    for _ in range(R):
        for k, tr in trs.items():
            t[k].append(time_loop(lambda i, tr=tr: tr.step(X[i % 2], Y[i % 2]), N))
    s = {k: stats(v) for k, v in t.items()}
    out = {"config": f"default Adam(1e-3); {trs['fp8'].cut_codec!r}; {trs['mx'].cut_codec!r}",
           "plain_repeat_range_ms": round(s["plain"]["max_ms"] - s["plain"]["min_ms"], 4)}
    for k in trs:
        out[k + "_step"] = s[k]
        out[k + "_samples_per_s"] = round(B / (s[k]["median_ms"] * 1e-3))
        if k != "plain":
            out[k + "_minus_plain_median_ms"] = round(s[k]["median_ms"] - s["plain"]["median_ms"], 4)
            out[k + "_over_plain_per_repeat"] = [round(b / a, 4) for a, b in zip(t["plain"], t[k])]
    return out


def quantisation_error(dev):
    from splitcnn.wide import SyntheticCIFAR, WideClientStage, WideServerStage, init_wide_models
    a, b = init_wide_models(seed=0)
    c, s = WideClientStage(a, device=dev), WideServerStage(b, device=dev, seed=0)
    x, y = (t.to(dev) for t in SyntheticCIFAR(42).batch(B))
    cut = c.forward(x).clone()
    dcut = s.step_request(cut, y)[0].clone()
    res = {}
    for tag, make, d in CODECS:
        q = make()
        for name, t in (("cut", cut), ("cut_gradient", dcut)):
            r = q.roundtrip(t, torch.empty_like(t), d).double()
            res[f"{tag}_{name}"] = float(((r - t.double()).norm() / t.double().norm()).item())
    res["zero_fraction"] = {"cut": float((cut == 0).float().mean().item()),
                            "cut_gradient": float((dcut == 0).float().mean().item())}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--launches", type=int, default=50)
    args = ap.parse_args()
    R, N, L = max(args.repeats, 3), max(args.steps, 20), max(args.launches, 20)
    dev = torch.device("cuda:0")
    out = {"tool": "cutmx_ab", "B": B, "repeats": R, "steps_per_repeat": N, "launches_per_repeat": L,
           "bytes_per_sample_and_direction": {"mx_e2m1_record": CUTMX_RECORD["e2m1"], "mx_e4m3_record": CUTMX_RECORD["e4m3"],
                                              "fp8_record": CUT8_RECORD, "dense_bf16": 2 * CUT8_SAMPLE}}
    out["launch_ms"] = launch_times(dev, R, L)
    out["k5_step"] = step_times(dev, R, N)
    out["relative_l2_error_of_roundtrip"] = quantisation_error(dev)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
