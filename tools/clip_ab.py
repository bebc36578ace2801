"""Measurement only: what optim.ClipNorm costs, ONE process, B = 4096, HIP events; prints one JSON line (stored as
profiles/clip_ab.txt).

  K2: SGD(0.01, momentum=0.9, nesterov=True, weight_decay=5e-4) without clip (slk_sgdm_multi_from_slabs)
      against the same recipe with ClipNorm (slk_reduce_sqnorm_multi + slk_sgdm_clip_multi);
  K5: AdamW(weight_decay=0.01) without and with ClipNorm (per stage slk_reduce_sqnorm_multi + slk_adamw_clip_multi
      in place of slk_adamw_multi_from_slabs / slk_adamw_from_slabs).

The trainers of a model replay their captured graphs on registered input buffers, interleaved repeat by repeat,
R repeats of N steps; the clipped step is reported against the unclipped configured step of the same process, with
that step's own repeat range beside it and a second unclipped trainer as the control. Then the optimizer launches
one by one (HIP events around each, interleaved) on the slabs the trainers' last step left: the one launch, and the
two that replace it. The threshold is half the smaller stage norm of a measured step, so the clip is active.

usage: python tools/clip_ab.py [--repeats 7] [--steps 100]"""
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


def ab(plain, clipped, control, R, N):
    """Interleaved repeats of N steps each; the clipped step (and the control: a second unclipped trainer) against
    the unclipped one of this process."""
    d, n, c = [], [], []
    for _ in range(R):
        d.append(time_loop(plain, N))
        n.append(time_loop(clipped, N))
        c.append(time_loop(control, N))
    sd, sn, sc = stats(d), stats(n), stats(c)
    return {"unclipped_step": sd, "clipped_step": sn, "control_unclipped_step": sc,
            "unclipped_repeat_range_ms": round(sd["max_ms"] - sd["min_ms"], 4),
            "clipped_minus_unclipped_median_ms": round(sn["median_ms"] - sd["median_ms"], 4),
            "control_minus_unclipped_median_ms": round(sc["median_ms"] - sd["median_ms"], 4),
            "clipped_over_unclipped_per_repeat": [round(b / a, 4) for a, b in zip(d, n)],
            "control_over_unclipped_per_repeat": [round(b / a, 4) for a, b in zip(d, c)],
            "unclipped_samples_per_s": round(B / (sd["median_ms"] * 1e-3)),
            "clipped_samples_per_s": round(B / (sn["median_ms"] * 1e-3))}


def launch_times(launches, R, N):
    for fn in launches.values():
        for _ in range(3):
            fn()
    reps = [time_each(launches, N) for _ in range(R)]
    return {name: stats([r[name] for r in reps]) for name in launches}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--steps", type=int, default=100)
    args = ap.parse_args()
    R, N = max(args.repeats, 3), max(args.steps, 20)
    dev = torch.device("cuda:0")
    out = {"tool": "clip_ab", "B": B, "repeats": R, "steps_per_repeat": N}
    T = R * N + 64   # a cosine table as long as the run

    # ---- K2
    X, Y = make_pool(B, 4, dev)
    cfg = optim.SGD(0.01, momentum=0.9, nesterov=True, weight_decay=5e-4)
    clip = optim.ClipNorm(float("inf"), device=dev)
    mk = lambda **kw: SplitTrainer(*init_models(seed=0), device=dev, graph=True, optim=cfg,  # noqa: E731
                                   schedule=optim.LRSchedule.warmup_cosine(0.01, 16, T, device=dev), **kw)
    trs = [mk(), mk(clip=clip), mk()]
    for tr in trs:
        for i in range(4):
            tr.register_inputs(X[i], Y[i])
        for i in range(4):
            tr.step(X[i], Y[i])
    td, tn, tc = trs
    norms = tn.grad_norms()
    clip.set_max_norm(0.5 * min(v for v, _ in norms.values()))
    tn.step(X[0], Y[0])
    out["k2"] = {"norms_unclipped_step": norms, "max_norm": clip.max_norm, "norms_clipped_step": tn.grad_norms()}
    out["k2"].update(ab(lambda i: td.step(X[i % 4], Y[i % 4]), lambda i: tn.step(X[i % 4], Y[i % 4]),
                        lambda i: tc.step(X[i % 4], Y[i % 4]), R, N))
    out["k2"]["config"] = repr(cfg) + ", warmup_cosine table"
    out["k2"]["norms_last_step"] = tn.grad_norms()

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
    server = [(ps[:k], gs[:k], bs[:k], slabs[0]), (ps[k:], gs[k:], bs[k:], slabs[1])]
    client = [(pc, gc, bc, slabs[2])]
    groups = [(torch.zeros(ops.clip_partials_needed(server), device=dev), torch.zeros(2, device=dev), server),
              (torch.zeros(ops.clip_partials_needed(client), device=dev), torch.zeros(2, device=dev), client)]
    out["k2"]["partials"] = {"server": groups[0][0].numel(), "client": groups[1][0].numel()}
    out["k2"]["launch_ms"] = launch_times({
        "sgdm_multi (unclipped: reduce + step + loss log)":
            lambda: ops.sgdm_multi_from_slabs(server + client, loss=loss, **kw),
        "reduce_sqnorm_multi (clipped, pass 1 + loss log)": lambda: ops.reduce_sqnorm_multi(groups, loss=loss),
        "sgdm_clip_multi (clipped, pass 2)": lambda: ops.sgdm_clip_multi(groups, clip.value, **kw),
    }, R, N)
    del trs, td, tn, tc

    # ---- K5
    from splitcnn.wide import SyntheticCIFAR, WideTrainer, init_wide_models
    data = SyntheticCIFAR(42)
    xs, ys = zip(*(data.batch(B) for _ in range(2)))
    XW, YW = torch.stack(xs).to(dev), torch.stack(ys).to(dev)
    cfg5 = optim.Adam(1e-3, weight_decay=0.01)
    clip5 = optim.ClipNorm(float("inf"), device=dev)
    mk5 = lambda **kw: WideTrainer(*init_wide_models(seed=0), device=dev, graph=True, optim=cfg5,  # noqa: E731
                                   schedule=optim.LRSchedule.warmup_cosine(1e-3, 16, T, device=dev), **kw)
    tws = [mk5(), mk5(clip=clip5), mk5()]
    for tw in tws:
        for i in range(2):
            tw.register_inputs(XW[i], YW[i])
        for i in range(4):
            tw.step(XW[i % 2], YW[i % 2])
    wd_, wn, wc = tws
    norms = wn.grad_norms()
    clip5.set_max_norm(0.5 * min(v for v, _ in norms.values()))
    wn.step(XW[0], YW[0])
    out["k5"] = {"norms_unclipped_step": norms, "max_norm": clip5.max_norm, "norms_clipped_step": wn.grad_norms()}
    out["k5"].update(ab(lambda i: wd_.step(XW[i % 2], YW[i % 2]), lambda i: wn.step(XW[i % 2], YW[i % 2]),
                        lambda i: wc.step(XW[i % 2], YW[i % 2]), R, N))
    out["k5"]["config"] = repr(cfg5) + ", warmup_cosine table"
    out["k5"]["norms_last_step"] = wn.grad_norms()
    out["k5"]["partials"] = {"client": wn.client.clip_npart, "server": wn.server.clip_npart}
    # each stage's optimizer sequence of either kind, eager, on each trainer's own slabs (its Adam state moves on)
    s_def = [buf(wd_.client, n) for n in ("s1", "s2", "s3")]
    s_new = [buf(wn.client, n) for n in ("s1", "s2", "s3")]
    out["k5"]["slab_counts"] = {"conv1": s_def[0].shape[0], "conv2": s_def[1].shape[0], "conv3": s_def[2].shape[0]}
    f_def, f_new = buf(wd_.server, "sf"), buf(wn.server, "sf")
    out["k5"]["slab_counts"]["fc"] = f_def.shape[0]
    out["k5"]["stage_sequence_ms"] = launch_times({
        "client step_from_slabs (unclipped: adamw_multi + shadows + tick)": lambda: wd_.client.step_from_slabs(*s_def),
        "client step_from_slabs (clipped: reduce_sqnorm + adamw_clip + shadows + tick)":
            lambda: wn.client.step_from_slabs(*s_new),
        "server step_from_slabs (unclipped: adamw + fc shadow + tick)": lambda: wd_.server.step_from_slabs(f_def),
        "server step_from_slabs (clipped: reduce_sqnorm + adamw_clip + fc shadow + tick)":
            lambda: wn.server.step_from_slabs(f_new),
    }, R, N)
    # the launches alone, on scratch state
    c = wn.client
    segs = [tuple(torch.zeros(n, device=dev) for _ in range(4)) + (sl,) for n, sl in zip((1792, 73856, 295168), s_new)]
    grp = [(torch.zeros(ops.clip_partials_needed(segs), device=dev), torch.zeros(2, device=dev), segs)]
    step = torch.zeros(1, dtype=torch.int32, device=dev)
    kw5 = dict(lr_table=c.schedule.table, step=step, **cfg5.kernel_args())
    out["k5"]["client_launch_ms"] = launch_times({
        "adamw_multi (unclipped: reduce + step)": lambda: ops.adamw_multi_from_slabs(segs, **kw5),
        "reduce_sqnorm_multi (clipped, pass 1)": lambda: ops.reduce_sqnorm_multi(grp),
        "adamw_clip_multi (clipped, pass 2)": lambda: ops.adamw_clip_multi(grp, clip5.value, **kw5),
    }, R, N)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
