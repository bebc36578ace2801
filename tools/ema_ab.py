"""Measurement only: what optim.EMA costs, ONE process, B = 4096, HIP events; prints one JSON line (stored as
profiles/ema_ab.txt).

  K2: SGD(0.01, momentum=0.9, nesterov=True, weight_decay=5e-4) without and with ema= (one slk_ema_multi over both
      stages' blocks in front of the shared tick);
  K5: AdamW(1e-3, weight_decay=0.01) without and with ema= (one slk_ema_multi per stage in front of its tick).

The trainers of a model replay their captured graphs on registered input buffers, interleaved repeat by repeat, R
repeats of N steps; the step with the average is reported against the plain step of the same process, with that
step's own repeat range beside it and a second plain trainer as the control. Then the lone slk_ema_multi launches,
eager, HIP events around each (the K2 launch over both blocks; the K5 client's and server's), and one evaluation
batch on the averaged and on the live weights, timed the same way (graph replays on the passes' static inputs).

usage: python tools/ema_ab.py [--repeats 7] [--steps 100]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "split-learning-k8s_amd"), ROOT]
from bench import make_pool  # noqa: E402
from eval_bench import stats, time_each, time_loop  # noqa: E402
from splitcnn import ops, optim  # noqa: E402
from splitcnn.data import init_models  # noqa: E402
from splitcnn.engine import SplitTrainer  # noqa: E402

B = 4096


def ab(plain, averaged, control, R, N):
    """Interleaved repeats of N steps each; the step with the average (and the control: a second plain trainer)
    against the plain one of this process."""
    d, n, c = [], [], []
    for _ in range(R):
        d.append(time_loop(plain, N))
        n.append(time_loop(averaged, N))
        c.append(time_loop(control, N))
    sd, sn, sc = stats(d), stats(n), stats(c)
    return {"plain_step": sd, "ema_step": sn, "control_plain_step": sc,
            "plain_repeat_range_ms": round(sd["max_ms"] - sd["min_ms"], 4),
            "ema_minus_plain_median_ms": round(sn["median_ms"] - sd["median_ms"], 4),
            "control_minus_plain_median_ms": round(sc["median_ms"] - sd["median_ms"], 4),
            "ema_over_plain_per_repeat": [round(b / a, 4) for a, b in zip(d, n)],
            "control_over_plain_per_repeat": [round(b / a, 4) for a, b in zip(d, c)],
            "plain_samples_per_s": round(B / (sd["median_ms"] * 1e-3)),
            "ema_samples_per_s": round(B / (sn["median_ms"] * 1e-3))}


def launch_times(launches, R, N):
    for fn in launches.values():
        for _ in range(3):
            fn()
    reps = [time_each(launches, N) for _ in range(R)]
    return {name: stats([r[name] for r in reps]) for name in launches}


def ema_launch(stages):
    cfg = stages[0].ema_cfg
    step = torch.full((1,), 1000, dtype=torch.int32, device=stages[0].device)   # past any warm-up: d = decay
    segs = [(torch.zeros_like(st.ema), st.params) for st in stages]             # scratch blocks: the trainers' stay
    return lambda: ops.ema_multi(segs, cfg.value, step, cfg.start, cfg.warmup)


def eval_times(tr, x, y, R, N):
    """One evaluation batch on either set of weights: replays of the passes' graphs (no accumulator)."""
    return launch_times({"eval_batch(weights='live')": lambda: tr.eval_batch(x, y),
                         "eval_batch(weights='ema')": lambda: tr.eval_batch(x, y, weights="ema")}, R, N)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--steps", type=int, default=100)
    args = ap.parse_args()
    R, N = max(args.repeats, 3), max(args.steps, 20)
    dev = torch.device("cuda:0")
    out = {"tool": "ema_ab", "B": B, "repeats": R, "steps_per_repeat": N}

    # ---- K2
    X, Y = make_pool(B, 4, dev)
    cfg = optim.SGD(0.01, momentum=0.9, nesterov=True, weight_decay=5e-4)
    mk = lambda **kw: SplitTrainer(*init_models(seed=0), device=dev, graph=True, optim=cfg, **kw)  # noqa: E731
    trs = [mk(), mk(ema=optim.EMA(0.999, device=dev)), mk()]
    for tr in trs:
        for i in range(4):
            tr.register_inputs(X[i], Y[i])
        for i in range(4):
            tr.step(X[i], Y[i])
    td, tn, tc = trs
    out["k2"] = ab(lambda i: td.step(X[i % 4], Y[i % 4]), lambda i: tn.step(X[i % 4], Y[i % 4]),
                   lambda i: tc.step(X[i % 4], Y[i % 4]), R, N)
    out["k2"]["config"] = repr(cfg) + ", " + repr(tn.client.ema_cfg)
    out["k2"]["ema_floats"] = tn.client.ema.numel() + tn.server.ema.numel()
    out["k2"]["launch_ms"] = launch_times({"ema_multi (client + server blocks, one launch)":
                                           ema_launch([tn.client, tn.server])}, R, N)
    out["k2"]["eval_ms"] = eval_times(tn, X[0], Y[0], R, N)
    del trs, td, tn, tc

    # ---- K5
    from splitcnn.wide import SyntheticCIFAR, WideTrainer, init_wide_models
    data = SyntheticCIFAR(42)
    xs, ys = zip(*(data.batch(B) for _ in range(2)))
    XW, YW = torch.stack(xs).to(dev), torch.stack(ys).to(dev)
    cfg5 = optim.Adam(1e-3, weight_decay=0.01)
    mk5 = lambda **kw: WideTrainer(*init_wide_models(seed=0), device=dev, graph=True, optim=cfg5, **kw)  # noqa: E731
    tws = [mk5(), mk5(ema=optim.EMA(0.999, device=dev)), mk5()]
    for tw in tws:
        for i in range(2):
            tw.register_inputs(XW[i], YW[i])
        for i in range(4):
            tw.step(XW[i % 2], YW[i % 2])
    wd_, wn, wc = tws
    out["k5"] = ab(lambda i: wd_.step(XW[i % 2], YW[i % 2]), lambda i: wn.step(XW[i % 2], YW[i % 2]),
                   lambda i: wc.step(XW[i % 2], YW[i % 2]), R, N)
    out["k5"]["config"] = repr(cfg5) + ", " + repr(wn.client.ema_cfg)
    out["k5"]["ema_floats"] = wn.client.ema.numel() + wn.server.ema.numel()
    out["k5"]["launch_ms"] = launch_times({"ema_multi (client block)": ema_launch([wn.client]),
                                           "ema_multi (server block)": ema_launch([wn.server])}, R, N)
    out["k5"]["eval_ms"] = eval_times(wn, XW[0], YW[0], R, N)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
