"""Measurement only: the evaluation path against the training forward, ONE process, B = 4096, seeded
synthetic inputs, HIP events; prints one JSON line (stored as profiles/eval_ab.txt).

  (i)  the code-less conv2 forward (slk_conv2_fwd_pool_x3p) against slk_conv2_fwd_pool_x3i: launches
       interleaved one for one, R repeats of N launches each, the per-launch mean of every repeat and the
       min / median over the repeats;
  (ii) the K2 and K5 evaluation graphs (ms per batch, samples/s) next to the same process's training step
       and, for K2, the three training forward launches (conv1_fwd, conv2_fwd_pool, the head) back to
       back — the pass evaluation replaces — and the evaluation's own launches one by one.

usage: python tools/eval_bench.py [--repeats 5] [--launches 50]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "split-learning-k8s_amd"), ROOT]
from bench import make_pool  # noqa: E402
from splitcnn import ops  # noqa: E402
from splitcnn.data import init_models  # noqa: E402
from splitcnn.engine import SplitTrainer  # noqa: E402
from splitcnn.metrics import EvalMetrics  # noqa: E402

B = 4096


def ev():
    return torch.cuda.Event(enable_timing=True)


def time_each(fns, n):
    """n rounds of the launches in `fns` (name -> callable), interleaved in order; mean ms per launch of each."""
    marks = {k: [] for k in fns}
    for _ in range(n):
        for k, fn in fns.items():
            s, e = ev(), ev()
            s.record()
            fn()
            e.record()
            marks[k].append((s, e))
    torch.cuda.synchronize()
    return {k: sum(s.elapsed_time(e) for s, e in v) / n for k, v in marks.items()}


def time_loop(fn, n):
    """ms per call of n back-to-back calls between one pair of events."""
    s, e = ev(), ev()
    s.record()
    for i in range(n):
        fn(i)
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / n


def stats(v):
    v = sorted(v)
    return {"min_ms": round(v[0], 4), "median_ms": round(v[len(v) // 2], 4), "max_ms": round(v[-1], 4),
            "per_repeat_ms": [round(t, 4) for t in v]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--launches", type=int, default=50)
    args = ap.parse_args()
    R, N = max(args.repeats, 3), max(args.launches, 50)
    dev = torch.device("cuda:0")
    X, Y = make_pool(B, 4, dev)
    out = {"tool": "eval_bench", "B": B, "repeats": R, "launches_per_repeat": N}

    # ---- K2
    tr = SplitTrainer(*init_models(seed=0), device=dev, graph=True)
    c, s = tr.client, tr.server
    W1, b1 = c.W1.detach(), c.b1.detach()
    m_ = s.model
    W2, b2, W3, b3 = (t.detach() for t in (m_.conv2.weight, m_.conv2.bias, m_.fc1.weight, m_.fc1.bias))
    x, y = X[0], Y[0]
    amax = torch.empty(B, device=dev)
    a16 = torch.empty(ops.conv2_act16_bytes(B), dtype=torch.uint8, device=dev)
    bitsb = ops.relu_bits_buffer(B, dev)
    pooled_i, pooled_p = (torch.empty(B, 64, 12, 12, device=dev) for _ in range(2))
    code = torch.empty(B, 64, 12, 12, dtype=torch.uint8, device=dev)
    logits, dlogits = (torch.empty(B, 10, device=dev) for _ in range(2))
    loss_i = torch.empty(B, device=dev)
    pred = torch.empty(B, dtype=torch.int64, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    met = EvalMetrics(dev)

    launches = {
        "train_conv1_fwd": lambda: ops.conv1_fwd_x3(x, W1, b1, amax, a16, relu_bits=bitsb),
        "train_conv2_fwd_pool_x3i": lambda: ops.conv2_fwd_pool_x3i(a16, amax, W2, b2, pooled=pooled_i, code=code),
        "train_fc_logits_xent": lambda: ops.fc_logits_xent(pooled_i, W3, b3, y, 1.0 / B, logits=logits, loss_i=loss_i,
                                                           dlogits=dlogits, err_flag=flag),
        "eval_conv1_fwd": lambda: ops.conv1_fwd_x3(x, W1, b1, amax, a16),
        "eval_conv2_fwd_pool_x3p": lambda: ops.conv2_fwd_pool_x3p(a16, amax, W2, b2, pooled=pooled_p),
        "eval_fc_eval": lambda: ops.fc_eval(pooled_p, W3, b3, y, logits=logits, loss_i=loss_i, pred=pred,
                                            err_flag=flag),
        "eval_accumulate": lambda: met.update(loss_i, pred, y),
    }
    for fn in launches.values():   # warm up every launch (code objects, buffers)
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    out["x3p_equals_x3i_bitwise"] = bool(torch.equal(pooled_p.view(torch.int32), pooled_i.view(torch.int32)))

    # (i) x3p against x3i, interleaved one for one
    ab = {"x3i": launches["train_conv2_fwd_pool_x3i"], "x3p": launches["eval_conv2_fwd_pool_x3p"]}
    reps = [time_each(ab, N) for _ in range(R)]
    out["conv2_ab"] = {k: stats([r[k] for r in reps]) for k in ab}
    out["conv2_ab"]["x3p_over_x3i_per_repeat"] = [round(r["x3p"] / r["x3i"], 4) for r in reps]

    # every launch on its own (the follow-up's baseline: head and conv2 times)
    reps = [time_each(launches, N) for _ in range(R)]
    out["launch_ms"] = {k: stats([r[k] for r in reps]) for k in launches}

    # (ii) back-to-back sequences and graphs
    t3 = ("train_conv1_fwd", "train_conv2_fwd_pool_x3i", "train_fc_logits_xent")
    e4 = ("eval_conv1_fwd", "eval_conv2_fwd_pool_x3p", "eval_fc_eval", "eval_accumulate")

    def seq(names):
        return lambda i: [launches[k]() for k in names]

    tr.eval_batch(x, y, met)       # captures the evaluation graph
    for i in range(4):
        tr.register_inputs(X[i], Y[i])
    for i in range(3):
        tr.step(X[i % 4], Y[i % 4])
    torch.cuda.synchronize()
    k2 = {"train_forward_3_launches": [], "eval_4_launches_eager": [], "eval_graph": [], "train_step_graph": []}
    for _ in range(R):             # the four interleaved, repeat by repeat
        k2["train_forward_3_launches"].append(time_loop(seq(t3), N))
        k2["eval_4_launches_eager"].append(time_loop(seq(e4), N))
        k2["eval_graph"].append(time_loop(lambda i: tr.eval_batch(X[i % 4], Y[i % 4], met), N))
        k2["train_step_graph"].append(time_loop(lambda i: tr.step(X[i % 4], Y[i % 4]), N))
    out["k2"] = {k: stats(v) for k, v in k2.items()}
    out["k2"]["eval_samples_per_s"] = round(B / (out["k2"]["eval_graph"]["median_ms"] * 1e-3))
    out["k2"]["train_samples_per_s"] = round(B / (out["k2"]["train_step_graph"]["median_ms"] * 1e-3))
    del tr

    # ---- K5
    from splitcnn.wide import SyntheticCIFAR, WideTrainer, init_wide_models
    data = SyntheticCIFAR(42)
    xs, ys = zip(*(data.batch(B) for _ in range(2)))
    XW, YW = torch.stack(xs).to(dev), torch.stack(ys).to(dev)
    tw = WideTrainer(*init_wide_models(seed=0), device=dev, graph=True)
    mw = EvalMetrics(dev)
    tw.eval_batch(XW[0], YW[0], mw)
    for i in range(2):
        tw.register_inputs(XW[i], YW[i])
    for i in range(3):
        tw.step(XW[i % 2], YW[i % 2])
    torch.cuda.synchronize()
    k5 = {"eval_graph": [], "train_step_graph": []}
    for _ in range(R):
        k5["eval_graph"].append(time_loop(lambda i: tw.eval_batch(XW[i % 2], YW[i % 2], mw), N))
        k5["train_step_graph"].append(time_loop(lambda i: tw.step(XW[i % 2], YW[i % 2]), N))
    out["k5"] = {k: stats(v) for k, v in k5.items()}
    out["k5"]["eval_samples_per_s"] = round(B / (out["k5"]["eval_graph"]["median_ms"] * 1e-3))
    out["k5"]["train_samples_per_s"] = round(B / (out["k5"]["train_step_graph"]["median_ms"] * 1e-3))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
