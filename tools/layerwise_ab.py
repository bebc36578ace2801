"""Measurement only: what optim.LARS and optim.LAMB cost, ONE process, B = 4096, HIP events; prints one JSON line
(stored as profiles/layerwise_ab.txt).

  K2: SGD(0.01, momentum=0.9, nesterov=True, weight_decay=5e-4) (slk_sgdm_multi_from_slabs) against LARS with the same
      momentum and decay (slk_reduce_tnorm_multi + slk_lars_multi) against the same SGD with ClipNorm
      (slk_reduce_sqnorm_multi + slk_sgdm_clip_multi);
  K5: AdamW(weight_decay=0.01) against LAMB (per stage slk_lamb_moments_multi + slk_lamb_multi) against AdamW with
      ClipNorm.

The yardstick of a layer-wise step is the clipped step of the same process: the same two-launch structure. The
trainers of a model replay their captured graphs on registered input buffers, interleaved repeat by repeat, R repeats
of N steps, a second unconfigured-recipe trainer as the control. Then the optimizer launches one by one (HIP events
around each, interleaved) on the slabs the trainers' last step left.

usage: python tools/layerwise_ab.py [--repeats 7] [--steps 100]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "split-learning-k8s_amd"), ROOT]
from bench import make_pool  # noqa: E402
from clip_ab import buf, launch_times  # noqa: E402
from eval_bench import stats, time_loop  # noqa: E402
from splitcnn import ops, optim  # noqa: E402
from splitcnn.data import init_models  # noqa: E402
from splitcnn.engine import SplitTrainer  # noqa: E402

B = 4096


def abc(plain, layer, clipped, control, R, N):
    """Interleaved repeats of N steps each: the layer-wise step against the plain and the clipped step."""
    t = {"plain": [], "layerwise": [], "clipped": [], "control_plain": []}
    for _ in range(R):
        for name, fn in zip(t, (plain, layer, clipped, control)):
            t[name].append(time_loop(fn, N))
    s = {k: stats(v) for k, v in t.items()}
    rng = lambda k: round(s[k]["max_ms"] - s[k]["min_ms"], 4)  # noqa: E731
    out = {f"{k}_step": v for k, v in s.items()}
    out.update({"plain_repeat_range_ms": rng("plain"), "clipped_repeat_range_ms": rng("clipped"),
                "layerwise_repeat_range_ms": rng("layerwise"),
                "layerwise_minus_clipped_median_ms": round(s["layerwise"]["median_ms"] - s["clipped"]["median_ms"], 4),
                "layerwise_minus_plain_median_ms": round(s["layerwise"]["median_ms"] - s["plain"]["median_ms"], 4),
                "control_minus_plain_median_ms": round(s["control_plain"]["median_ms"] - s["plain"]["median_ms"], 4),
                "layerwise_over_clipped_per_repeat": [round(b / a, 4) for a, b in zip(t["clipped"], t["layerwise"])],
                "layerwise_samples_per_s": round(B / (s["layerwise"]["median_ms"] * 1e-3)),
                "clipped_samples_per_s": round(B / (s["clipped"]["median_ms"] * 1e-3)),
                "plain_samples_per_s": round(B / (s["plain"]["median_ms"] * 1e-3))})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--steps", type=int, default=100)
    args = ap.parse_args()
    R, N = max(args.repeats, 3), max(args.steps, 20)
    dev = torch.device("cuda:0")
    out = {"tool": "layerwise_ab", "B": B, "repeats": R, "steps_per_repeat": N}
    T = R * N + 64   # a cosine table as long as the run

    # ---- K2
    X, Y = make_pool(B, 4, dev)
    sgd = optim.SGD(0.01, momentum=0.9, nesterov=True, weight_decay=5e-4)
    lars = optim.LARS(0.01, momentum=0.9, nesterov=True, weight_decay=5e-4)
    clip = optim.ClipNorm(float("inf"), device=dev)
    mk = lambda cfg, **kw: SplitTrainer(*init_models(seed=0), device=dev, graph=True, optim=cfg,  # noqa: E731
                                        schedule=optim.LRSchedule.warmup_cosine(0.01, 16, T, device=dev), **kw)
    trs = [mk(sgd), mk(lars), mk(sgd, clip=clip), mk(sgd)]
    for tr in trs:
        for i in range(4):
            tr.register_inputs(X[i], Y[i])
        for i in range(4):
            tr.step(X[i], Y[i])
    clip.set_max_norm(0.5 * min(v for v, _ in trs[2].grad_norms().values()))
    fns = [(lambda i, tr=tr: tr.step(X[i % 4], Y[i % 4])) for tr in trs]
    out["k2"] = {"config": repr(lars) + " / " + repr(sgd) + ", warmup_cosine table", "max_norm": clip.max_norm}
    out["k2"].update(abc(*fns, R, N))
    out["k2"]["trust_ratios_last_step"] = trs[1].trust_ratios()

    k = ops.CONV2_SLAB
    td = trs[0]
    loss_i = buf(td.server, "loss_i")
    ring, ctr = torch.zeros(4096, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    slabs = (buf(td.server, "s2"), buf(td.server, "s3"), buf(td.client, "c1w_slabs"))
    ps, pc = torch.randn(ops.SERVER_NPARAM, device=dev), torch.randn(ops.CLIENT_NPARAM, device=dev)
    gs, gc, bs, bc = (torch.zeros_like(t) for t in (ps, pc, ps, pc))
    step = torch.zeros(1, dtype=torch.int32, device=dev)
    loss = (loss_i, 1.0 / B, ring, ctr)
    kw = dict(lr_table=td.server.schedule.table, step=step)
    server = [(ps[:k], gs[:k], bs[:k], slabs[0]), (ps[k:], gs[k:], bs[k:], slabs[1])]
    client = [(pc, gc, bc, slabs[2])]
    cg = [(torch.zeros(ops.clip_partials_needed(server), device=dev), torch.zeros(2, device=dev), server),
          (torch.zeros(ops.clip_partials_needed(client), device=dev), torch.zeros(2, device=dev), client)]
    lserver = [s + (nw,) for s, nw in zip(server, (18432, 92160))]
    lclient = [client[0] + (288,)]
    lg = [(torch.zeros(ops.trust_partials_needed(lserver), device=dev), torch.zeros(4, 3, device=dev), lserver),
          (torch.zeros(ops.trust_partials_needed(lclient), device=dev), torch.zeros(2, 3, device=dev), lclient)]
    out["k2"]["launch_ms"] = launch_times({
        "sgdm_multi (plain: reduce + step + loss log)":
            lambda: ops.sgdm_multi_from_slabs(server + client, loss=loss, **kw, **sgd.kernel_args()),
        "reduce_sqnorm_multi (clipped, pass 1 + loss log)": lambda: ops.reduce_sqnorm_multi(cg, loss=loss),
        "sgdm_clip_multi (clipped, pass 2)": lambda: ops.sgdm_clip_multi(cg, clip.value, **kw, **sgd.kernel_args()),
        "reduce_tnorm_multi (LARS, pass 1 + loss log)": lambda: ops.reduce_tnorm_multi(lg, loss=loss),
        "lars_multi (LARS, pass 2)": lambda: ops.lars_multi(lg, **kw, **lars.kernel_args()),
    }, R, N)
    del trs, td, fns

    # ---- K5
    from splitcnn.wide import SyntheticCIFAR, WideTrainer, init_wide_models
    data = SyntheticCIFAR(42)
    xs, ys = zip(*(data.batch(B) for _ in range(2)))
    XW, YW = torch.stack(xs).to(dev), torch.stack(ys).to(dev)
    adamw, lamb = optim.Adam(1e-3, weight_decay=0.01), optim.LAMB(1e-3, weight_decay=0.01)
    clip5 = optim.ClipNorm(float("inf"), device=dev)
    mk5 = lambda cfg, **kw: WideTrainer(*init_wide_models(seed=0), device=dev, graph=True, optim=cfg,  # noqa: E731
                                        schedule=optim.LRSchedule.warmup_cosine(1e-3, 16, T, device=dev), **kw)
    tws = [mk5(adamw), mk5(lamb), mk5(adamw, clip=clip5), mk5(adamw)]
    for tw in tws:
        for i in range(2):
            tw.register_inputs(XW[i], YW[i])
        for i in range(4):
            tw.step(XW[i % 2], YW[i % 2])
    clip5.set_max_norm(0.5 * min(v for v, _ in tws[2].grad_norms().values()))
    fns = [(lambda i, tw=tw: tw.step(XW[i % 2], YW[i % 2])) for tw in tws]
    out["k5"] = {"config": repr(lamb) + " / " + repr(adamw) + ", warmup_cosine table", "max_norm": clip5.max_norm}
    out["k5"].update(abc(*fns, R, N))
    out["k5"]["trust_ratios_last_step"] = tws[1].trust_ratios()
    # the client's launches alone, on scratch state and the plain trainer's slabs
    c = tws[0].client
    sl = [buf(c, n) for n in ("s1", "s2", "s3")]
    out["k5"]["slab_counts"] = {"conv1": sl[0].shape[0], "conv2": sl[1].shape[0], "conv3": sl[2].shape[0]}
    segs = [(torch.randn(n, device=dev),) + tuple(torch.zeros(n, device=dev) for _ in range(3)) + (s,)
            for n, s in zip((1792, 73856, 295168), sl)]
    lsegs = [s + (nw,) for s, nw in zip(segs, (1728, 73728, 294912))]
    grp = [(torch.zeros(ops.clip_partials_needed(segs), device=dev), torch.zeros(2, device=dev), segs)]
    lgrp = [(torch.zeros(ops.trust_partials_needed(lsegs), device=dev), torch.zeros(6, 3, device=dev), lsegs)]
    step = torch.zeros(1, dtype=torch.int32, device=dev)
    kw5 = dict(lr_table=c.schedule.table, step=step)
    lk = lamb.kernel_args()
    out["k5"]["client_launch_ms"] = launch_times({
        "adamw_multi (plain: reduce + step)": lambda: ops.adamw_multi_from_slabs(segs, **kw5, **adamw.kernel_args()),
        "reduce_sqnorm_multi (clipped, pass 1)": lambda: ops.reduce_sqnorm_multi(grp),
        "adamw_clip_multi (clipped, pass 2)": lambda: ops.adamw_clip_multi(grp, clip5.value, **kw5, **adamw.kernel_args()),
        "lamb_moments_multi (LAMB, pass 1)": lambda: ops.lamb_moments_multi(lgrp, step, **lk),
        "lamb_multi (LAMB, pass 2)": lambda: ops.lamb_multi(lgrp, **kw5, **lk),
    }, R, N)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
