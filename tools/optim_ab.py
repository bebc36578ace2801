"""Measurement only: what the optimizer configs of splitcnn.optim cost, ONE process, B = 4096, HIP events;
prints one JSON line (stored as profiles/optim_ab.txt).

  K2: the default step (optim.SGD(0.01) by value, slk_sgd_multi_from_slabs) against
      SGD(momentum=0.9, nesterov=True, weight_decay=5e-4) on a cosine table (slk_sgdm_multi_from_slabs + slk_tick);
  K5: the default step (Adam by value) against AdamW(weight_decay=0.01) on the same kind of table.

The trainers of a model replay their captured graphs on registered input buffers, interleaved repeat by
repeat, R repeats of N steps; the new step is reported against the default step of the same process, with the
default step's own repeat range beside it and a second default trainer as the control (what two trainers of
the same kind differ by). Then the optimizer launches one by one (HIP events around each, interleaved), on the
slabs the trainers' last step left: the default launches, the new launches, and the tick.

usage: python tools/optim_ab.py [--repeats 7] [--steps 100]"""
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


def buf(stage, name):
    """The stage's scratch buffer `name` (one batch size has run, so there is one)."""
    (t,) = [v for k, v in stage._buf._b.items() if k[0] == name]
    return t


def ab(default, new, control, R, N):
    """Interleaved repeats of N steps each; the new step (and the control: a second default trainer) against
    the default one of this process."""
    d, n, c = [], [], []
    for _ in range(R):
        d.append(time_loop(default, N))
        n.append(time_loop(new, N))
        c.append(time_loop(control, N))
    sd, sn, sc = stats(d), stats(n), stats(c)
    return {"default_step": sd, "new_step": sn, "control_default_step": sc,
            "default_repeat_range_ms": round(sd["max_ms"] - sd["min_ms"], 4),
            "new_minus_default_median_ms": round(sn["median_ms"] - sd["median_ms"], 4),
            "control_minus_default_median_ms": round(sc["median_ms"] - sd["median_ms"], 4),
            "new_over_default_per_repeat": [round(b / a, 4) for a, b in zip(d, n)],
            "control_over_default_per_repeat": [round(b / a, 4) for a, b in zip(d, c)],
            "default_samples_per_s": round(B / (sd["median_ms"] * 1e-3)),
            "new_samples_per_s": round(B / (sn["median_ms"] * 1e-3))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--steps", type=int, default=100)
    args = ap.parse_args()
    R, N = max(args.repeats, 3), max(args.steps, 20)
    dev = torch.device("cuda:0")
    out = {"tool": "optim_ab", "B": B, "repeats": R, "steps_per_repeat": N}
    T = R * N + 64   # a cosine table as long as the run

    # ---- K2
    X, Y = make_pool(B, 4, dev)
    cfg = optim.SGD(0.01, momentum=0.9, nesterov=True, weight_decay=5e-4)
    trs = [SplitTrainer(*init_models(seed=0), device=dev, graph=True),
           SplitTrainer(*init_models(seed=0), device=dev, graph=True, optim=cfg,
                        schedule=optim.LRSchedule.warmup_cosine(0.01, 16, T, device=dev)),
           SplitTrainer(*init_models(seed=0), device=dev, graph=True)]
    for tr in trs:
        for i in range(4):
            tr.register_inputs(X[i], Y[i])
        for i in range(4):
            tr.step(X[i], Y[i])
    torch.cuda.synchronize()
    td, tn, tc = trs
    out["k2"] = ab(lambda i: td.step(X[i % 4], Y[i % 4]), lambda i: tn.step(X[i % 4], Y[i % 4]),
                   lambda i: tc.step(X[i % 4], Y[i % 4]), R, N)
    out["k2"]["new_config"] = repr(cfg) + ", warmup_cosine table"

    k = ops.CONV2_SLAB
    loss_i = buf(td.server, "loss_i")
    ring, ctr = torch.zeros(4096, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    slabs = (buf(td.server, "s2"), buf(td.server, "s3"), buf(td.client, "c1w_slabs"))
    out["k2"]["slab_counts"] = {"conv2": slabs[0].shape[0], "fc": slabs[1].shape[0], "client": slabs[2].shape[0]}
    ps, pc = torch.zeros(ops.SERVER_NPARAM, device=dev), torch.zeros(ops.CLIENT_NPARAM, device=dev)
    gs, gc, bs, bc = (torch.zeros_like(t) for t in (ps, pc, ps, pc))
    step = torch.zeros(1, dtype=torch.int32, device=dev)
    loss = (loss_i, 1.0 / B, ring, ctr)
    kw = dict(lr_table=tn.server.schedule.table, step=step, **cfg.kernel_args())
    launches = {
        "sgd_multi (default)": lambda: ops.sgd_multi_from_slabs(
            [(ps[:k], gs[:k], slabs[0]), (ps[k:], gs[k:], slabs[1]), (pc, gc, slabs[2])], 0.0, loss=loss),
        "sgdm_multi (new)": lambda: ops.sgdm_multi_from_slabs(
            [(ps[:k], gs[:k], bs[:k], slabs[0]), (ps[k:], gs[k:], bs[k:], slabs[1]), (pc, gc, bc, slabs[2])],
            loss=loss, **kw),
        "tick (new)": lambda: ops.tick(step),
    }
    for fn in launches.values():
        for _ in range(3):
            fn()
    reps = [time_each(launches, N) for _ in range(R)]
    out["k2"]["launch_ms"] = {name: stats([r[name] for r in reps]) for name in launches}
    del trs, td, tn, tc

    # ---- K5
    from splitcnn.wide import SyntheticCIFAR, WideTrainer, init_wide_models
    data = SyntheticCIFAR(42)
    xs, ys = zip(*(data.batch(B) for _ in range(2)))
    XW, YW = torch.stack(xs).to(dev), torch.stack(ys).to(dev)
    cfg5 = optim.Adam(1e-3, weight_decay=0.01)
    tws = [WideTrainer(*init_wide_models(seed=0), device=dev, graph=True),
           WideTrainer(*init_wide_models(seed=0), device=dev, graph=True, optim=cfg5,
                       schedule=optim.LRSchedule.warmup_cosine(1e-3, 16, T, device=dev)),
           WideTrainer(*init_wide_models(seed=0), device=dev, graph=True)]
    for tw in tws:
        for i in range(2):
            tw.register_inputs(XW[i], YW[i])
        for i in range(4):
            tw.step(XW[i % 2], YW[i % 2])
    torch.cuda.synchronize()
    wd_, wn, wc = tws
    out["k5"] = ab(lambda i: wd_.step(XW[i % 2], YW[i % 2]), lambda i: wn.step(XW[i % 2], YW[i % 2]),
                   lambda i: wc.step(XW[i % 2], YW[i % 2]), R, N)
    out["k5"]["new_config"] = repr(cfg5) + ", warmup_cosine table"
    # each stage's optimizer launches of either kind, eager, on each trainer's own slabs (its Adam state moves on)
    s_def = [buf(wd_.client, n) for n in ("s1", "s2", "s3")]
    s_new = [buf(wn.client, n) for n in ("s1", "s2", "s3")]
    out["k5"]["slab_counts"] = {"conv1": s_def[0].shape[0], "conv2": s_def[1].shape[0], "conv3": s_def[2].shape[0]}
    f_def, f_new = buf(wd_.server, "sf"), buf(wn.server, "sf")
    out["k5"]["slab_counts"]["fc"] = f_def.shape[0]
    launches = {"client step_from_slabs (default: adam_multi + shadows + tick)": lambda: wd_.client.step_from_slabs(*s_def),
                "client step_from_slabs (new: adamw_multi + shadows + tick)": lambda: wn.client.step_from_slabs(*s_new),
                "server step_from_slabs (default: adam + fc shadow + tick)": lambda: wd_.server.step_from_slabs(f_def),
                "server step_from_slabs (new: adamw + fc shadow + tick)": lambda: wn.server.step_from_slabs(f_new)}
    for fn in launches.values():
        for _ in range(3):
            fn()
    reps = [time_each(launches, N) for _ in range(R)]
    out["k5"]["stage_sequence_ms"] = {name: stats([r[name] for r in reps]) for name in launches}
    del tws, wd_, wn, wc

    # every launch of the eager K5 step between its own pair of HIP events (engine.TIMER), default then new:
    # which launch the new step's time goes to
    from splitcnn.engine import TIMER
    per_launch = {}
    for name, kw in (("default", {}), ("new", {"optim": cfg5, "schedule": optim.LRSchedule.warmup_cosine(1e-3, 16, T, device=dev)})):
        tw = WideTrainer(*init_wide_models(seed=0), device=dev, graph=False, **kw)
        for i in range(4):
            tw.step(XW[i % 2], YW[i % 2])
        torch.cuda.synchronize()
        TIMER.reset()
        TIMER.enabled = True
        for i in range(N):
            tw.step(XW[i % 2], YW[i % 2])
        per_launch[name] = {k: {"per_step_ms": round(v["avg_ms"] * v["n"] / N, 4), "launches_per_step": v["n"] // N,
                                "min_ms": round(v["min_ms"], 4)} for k, v in TIMER.summary().items()}
        TIMER.enabled = False
        TIMER.reset()
        del tw
    opt_names = ("adam", "shadow", "tick")
    out["k5"]["eager_launch_ms"] = {
        name: {"optimizer_launches": {k: v for k, v in t.items() if any(s in k for s in opt_names)},
               "optimizer_per_step_ms": round(sum(v["per_step_ms"] for k, v in t.items()
                                                  if any(s in k for s in opt_names)), 4),
               "other_launches_per_step_ms": round(sum(v["per_step_ms"] for k, v in t.items()
                                                       if not any(s in k for s in opt_names)), 4)}
        for name, t in per_launch.items()}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
