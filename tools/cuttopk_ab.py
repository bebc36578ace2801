"""Measurement only: what codec.TopKCut costs on one GPU, ONE process, B = 4096, HIP events; prints one JSON line
(stored as profiles/cuttopk_ab.txt). The method is tools/cutmx_ab.py's.

  launches: slk_cuttopk_encode / _decode / _roundtrip at k = 1024 and 2048 over the seeded model's step-0 cut (4096
            samples), eager, each between its own pair of HIP events and each behind a device-to-device copy that moves
            as many bytes as the launch reads plus writes (copy_(n) moves n bytes in and n out: the copy's tensor holds
            half the launch's bytes); reported per repeat as launch / copy. slk_cutmx_roundtrip (e2m1) and
            slk_cut8_roundtrip (e4m3) run in the same repeats on the same input: the yardsticks are the copy and those
            two launches, never the top-k kernel itself;
  step:     the graphed K5 step (default Adam) plain and with cut_codec=TopKCut(2048) on registered input buffers,
            interleaved repeat by repeat, with a second plain trainer as the control;
  error:    the relative L2 error |x - roundtrip(x)| / |x| at k = 1024 and 2048 on that cut and its cut gradient —
            for information only: no claim and no threshold.

Not measured here: accuracy on real CIFAR-10, any multi-GPU time, hardware counters, other batch sizes.

usage: python tools/cuttopk_ab.py [--repeats 7] [--steps 100] [--launches 50]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "split-learning-k8s_amd"), ROOT]
from eval_bench import stats, time_each, time_loop  # noqa: E402
from splitcnn.codec import CUT8_SAMPLE, Fp8Cut, MxCut, TopKCut  # noqa: E402

B = 4096
KS = (1024, 2048)


def step0(dev):
    """The seeded model's step-0 cut and cut gradient on a synthetic CIFAR batch."""
    from splitcnn.wide import SyntheticCIFAR, WideClientStage, WideServerStage, init_wide_models
    a, b = init_wide_models(seed=0)
    c, s = WideClientStage(a, device=dev), WideServerStage(b, device=dev, seed=0)
    x, y = (t.to(dev) for t in SyntheticCIFAR(42).batch(B))
    cut = c.forward(x).clone()
    return cut, s.step_request(cut, y)[0].clone()


def launch_times(dev, x, R, N):
    out = torch.empty_like(x)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    dense = B * CUT8_SAMPLE * 2
    fns, moved = {}, {}

    def add(key, fn, nbytes):
        src = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev)
        dst = torch.empty_like(src)
        fns[key], moved[key] = fn, nbytes
        fns[key + "_copy"] = lambda: dst.copy_(src)
    for k in KS:
        q = TopKCut(k, None)
        recb = B * q.record_bytes("fwd")
        rec = q.records("ab", B, dev, direction="fwd")
        q.encode(x, rec, "fwd")
        add(f"topk{k}_encode", lambda q=q, rec=rec: q.encode(x, rec, "fwd"), dense + recb)
        add(f"topk{k}_decode", lambda q=q, rec=rec: q.decode(rec, out, err, "fwd"), recb + dense)
        add(f"topk{k}_roundtrip", lambda q=q: q.roundtrip(x, out, "fwd"), 2 * dense)
    mx, f8 = MxCut("e2m1", None), Fp8Cut("e4m3", None)
    add("mx_e2m1_roundtrip", lambda: mx.roundtrip(x, out, "fwd"), 2 * dense)
    add("fp8_e4m3_roundtrip", lambda: f8.roundtrip(x, out, "fwd"), 2 * dense)
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
    trs = {"plain": mk(), "topk": mk(cut_codec=TopKCut(2048)), "control": mk()}
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
    out = {"config": f"default Adam(1e-3); {trs['topk'].cut_codec!r}",
           "plain_repeat_range_ms": round(s["plain"]["max_ms"] - s["plain"]["min_ms"], 4)}
    for k in trs:
        out[k + "_step"] = s[k]
        if k != "plain":
            out[k + "_minus_plain_median_ms"] = round(s[k]["median_ms"] - s["plain"]["median_ms"], 4)
            out[k + "_over_plain_per_repeat"] = [round(b / a, 4) for a, b in zip(t["plain"], t[k])]
    return out


def sparsification_error(cut, dcut):
    res = {}
    for k in KS:
        q = TopKCut(k, k)
        for name, t, d in (("cut", cut, "fwd"), ("cut_gradient", dcut, "bwd")):
            r = q.roundtrip(t, torch.empty_like(t), d).double()
            res[f"topk{k}_{name}"] = float(((r - t.double()).norm() / t.double().norm()).item())
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
    cut, dcut = step0(dev)
    out = {"tool": "cuttopk_ab", "B": B, "repeats": R, "steps_per_repeat": N, "launches_per_repeat": L,
           "bytes_per_sample_and_direction": {**{f"topk{k}_record": TopKCut(k).record_bytes("fwd") for k in KS},
                                              "dense_bf16": 2 * CUT8_SAMPLE}}
    out["launch_ms"] = launch_times(dev, cut, R, L)
    out["k5_step"] = step_times(dev, R, N)
    out["relative_l2_error_of_roundtrip"] = sparsification_error(cut, dcut)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
