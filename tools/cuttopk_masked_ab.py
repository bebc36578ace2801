"""Measurement only: what codec.TopKCut(k, "masked") costs on one GPU, ONE process, B = 4096, HIP events; prints one
JSON line (stored as profiles/cuttopk_masked_ab.txt). The method is tools/cuttopk_ab.py's.

  launches: slk_cuttopk_roundtrip_map / _mask / _gather / _scatter at k = 1024 and 2048 over the seeded model's step-0
            cut and cut gradient (4096 samples), eager, each between its own pair of HIP events and each behind a
            device-to-device copy that moves as many bytes as the launch reads plus writes (copy_(n) moves n bytes in
            and n out: the copy's tensor holds half the launch's bytes); reported per repeat as launch / copy.
            slk_cuttopk_roundtrip on the cut gradient runs in the same repeats: it is what the mask replaces;
  step:     the graphed K5 step (default Adam) plain, with TopKCut(2048, None), TopKCut(2048, 2048) and
            TopKCut(2048, "masked") on registered input buffers, interleaved repeat by repeat, with a second plain
            trainer as the control.

No pass ratio: the output says which medians differ by more than the repeats' ranges and claims nothing else.
Not measured here: accuracy (there is no dataset here), any multi-GPU time, hardware counters, other batch sizes.

usage: python tools/cuttopk_masked_ab.py [--repeats 7] [--steps 100] [--launches 50]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "split-learning-k8s_amd"), ROOT, os.path.join(ROOT, "tools")]
from cuttopk_ab import B, KS, step0  # noqa: E402
from eval_bench import stats, time_each, time_loop  # noqa: E402
from splitcnn.codec import CUT8_SAMPLE, CUTTOPK_MAP, TopKCut  # noqa: E402


def launch_times(dev, cut, dcut, R, N):
    out = torch.empty_like(cut)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    m = torch.empty(B, CUTTOPK_MAP, dtype=torch.uint8, device=dev)
    dense, mapb = B * CUT8_SAMPLE * 2, B * CUTTOPK_MAP
    fns, moved = {}, {}

    def add(key, fn, nbytes):
        src = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev)
        dst = torch.empty_like(src)
        fns[key], moved[key] = fn, nbytes
        fns[key + "_copy"] = lambda: dst.copy_(src)
    for k in KS:
        q = TopKCut(k, "masked")
        recb = B * q.record_bytes("bwd")
        rec = q.records("ab", B, dev, direction="bwd")
        mk = m.clone()
        q.roundtrip(cut, out, "fwd", map=mk)   # the map of this k, read by the three launches below
        q.encode(dcut, rec, "bwd", map=mk)
        scratch = torch.empty_like(m)
        add(f"k{k}_roundtrip_map", lambda q=q, s=scratch: q.roundtrip(cut, out, "fwd", map=s), 2 * dense + mapb)
        add(f"k{k}_mask", lambda q=q, mk=mk: q.roundtrip(dcut, out, "bwd", map=mk), 2 * dense + mapb)
        add(f"k{k}_gather", lambda q=q, mk=mk, rec=rec: q.encode(dcut, rec, "bwd", map=mk), dense + mapb + recb)
        add(f"k{k}_scatter", lambda q=q, mk=mk, rec=rec: q.decode(rec, out, err, "bwd", map=mk), recb + mapb + dense)
        t = TopKCut(k, k)
        add(f"k{k}_topk_roundtrip_of_dcut", lambda t=t: t.roundtrip(dcut, out, "bwd"), 2 * dense)
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
    mk = lambda q=None: WideTrainer(*init_wide_models(seed=0), device=dev, graph=True, cut_codec=q)  # noqa: E731
    trs = {"plain": mk(), "topk_fwd_only": mk(TopKCut(2048, None)), "topk_both": mk(TopKCut(2048, 2048)),
           "topk_masked": mk(TopKCut(2048, "masked")), "control": mk()}
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
    out = {"config": "default Adam(1e-3); " + "; ".join(repr(tr.cut_codec) for tr in trs.values() if tr.cut_codec)}
    for k in trs:
        out[k + "_step"] = s[k]
    # a difference of medians leaves the ranges where the two configurations' [min, max] do not overlap
    pairs = [("control", "plain"), ("topk_fwd_only", "plain"), ("topk_masked", "topk_fwd_only"),
             ("topk_both", "topk_masked"), ("topk_both", "topk_fwd_only")]
    out["differences"] = {f"{a}_minus_{b}": {
        "median_ms": round(s[a]["median_ms"] - s[b]["median_ms"], 4),
        "leaves_the_repeat_ranges": s[a]["min_ms"] > s[b]["max_ms"] or s[a]["max_ms"] < s[b]["min_ms"]}
        for a, b in pairs}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--launches", type=int, default=50)
    args = ap.parse_args()
    R, N, L = max(args.repeats, 3), max(args.steps, 20), max(args.launches, 20)
    dev = torch.device("cuda:0")
    cut, dcut = step0(dev)
    out = {"tool": "cuttopk_masked_ab", "B": B, "repeats": R, "steps_per_repeat": N, "launches_per_repeat": L,
           "bytes_per_sample": {**{f"masked_backward_k{k}": TopKCut(k, "masked").record_bytes("bwd") for k in KS},
                                **{f"topk_backward_k{k}": TopKCut(k, k).record_bytes("bwd") for k in KS},
                                "dense_bf16": 2 * CUT8_SAMPLE}}
    out["launch_ms"] = launch_times(dev, cut, dcut, R, L)
    out["k5_step"] = step_times(dev, R, N)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
