"""Measurement only: what CutMix in the batch kernel and the soft-target heads cost, ONE process, B = 4096, HIP
events; prints one JSON line (stored as profiles/mix_ab.txt).

  (i)  slk_image_batch_mix<3,32,32> (pad 4, flip, prob 1) against slk_image_batch<3,32,32> (pad 4, flip) on a seeded
       synthetic dataset of CIFAR-10's size resident in HBM, and in front of each a device-to-device copy of as many
       bytes as the launch writes (the bandwidth yardstick of this process), plus the mixed launch at prob 0 (all
       its hashes and both sources' address arithmetic, but no box, so no second source is loaded): the six launches
       interleaved one for one, R repeats of N rounds, every launch between its own pair of events; each round
       gathers another slice of one permutation (the partners are the slice rolled by one, as the loaders do it);
  (ii) the graphed K2 and K5 steps with loss=SoftCrossEntropy(0.1) on mixed labels against the default trainer on
       plain labels, with a second default trainer as the control and a loss=SoftCrossEntropy(0.0) trainer on the
       plain labels (the default's arithmetic through the soft kernels): registered input buffers, interleaved
       repeat by repeat, R repeats of N steps.

usage: python tools/mix_ab.py [--repeats 7] [--launches 48] [--steps 100]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "split-learning-k8s_amd"), ROOT]
from bench import make_pool  # noqa: E402
from eval_bench import stats, time_each, time_loop  # noqa: E402
from loader_bench import Synthetic  # noqa: E402
from splitcnn import ops  # noqa: E402
from splitcnn.cifar import CIFAR_MEAN, CIFAR_STD  # noqa: E402
from splitcnn.loss import SoftCrossEntropy, pack_mixed, unpack_mixed  # noqa: E402

B = 4096


def mixed_labels(y, seed):
    """Mixed labels over plain ones: the partner is the batch rolled by one, the weight uniform in [0, 1)."""
    g = torch.Generator().manual_seed(seed)
    return pack_mixed(y, y.roll(1), torch.rand(y.shape[0], generator=g).to(y.device))


def ab(plain, soft, control, soft0, R, N):
    """Interleaved repeats of N steps each: the soft step, the control (a second default trainer) and the soft
    kernels at smoothing 0 on the default trainer's plain labels (the default's arithmetic bit for bit, through the
    soft instantiation: what the kernel itself costs, apart from what other targets do to the values) against the
    default step of this process."""
    d, n, c, z = [], [], [], []
    for _ in range(R):
        d.append(time_loop(plain, N))
        n.append(time_loop(soft, N))
        c.append(time_loop(control, N))
        z.append(time_loop(soft0, N))
    sd, sn, sc, sz = stats(d), stats(n), stats(c), stats(z)
    return {"default_step": sd, "soft_step": sn, "control_default_step": sc, "soft_smoothing0_plain_labels_step": sz,
            "soft0_minus_default_median_ms": round(sz["median_ms"] - sd["median_ms"], 4),
            "soft0_over_default_per_repeat": [round(b / a, 4) for a, b in zip(d, z)],
            "default_repeat_range_ms": round(sd["max_ms"] - sd["min_ms"], 4),
            "soft_minus_default_median_ms": round(sn["median_ms"] - sd["median_ms"], 4),
            "control_minus_default_median_ms": round(sc["median_ms"] - sd["median_ms"], 4),
            "soft_over_default_per_repeat": [round(b / a, 4) for a, b in zip(d, n)],
            "control_over_default_per_repeat": [round(b / a, 4) for a, b in zip(d, c)],
            "default_samples_per_s": round(B / (sd["median_ms"] * 1e-3)),
            "soft_samples_per_s": round(B / (sn["median_ms"] * 1e-3))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--launches", type=int, default=48)
    ap.add_argument("--steps", type=int, default=100)
    args = ap.parse_args()
    R, NL, NS = max(args.repeats, 3), max(args.launches, 24), max(args.steps, 20)
    dev = torch.device("cuda:0")
    out = {"tool": "mix_ab", "B": B, "repeats": R, "launches_per_repeat": NL, "steps_per_repeat": NS}

    # ---- (i) the launches
    cf = Synthetic(50000, (3, 32, 32), 2)
    ci, cl = torch.from_numpy(cf.images).to(dev), torch.from_numpy(cf.labels).to(dev)
    perm = torch.randperm(50000, generator=torch.Generator().manual_seed(3)).to(dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    k = {"c": 0}

    slices = perm[:(50000 // B) * B].view(-1, B)
    partners = slices.roll(1, dims=1).contiguous()   # made once: only the launch itself sits between the events

    def cslice():
        k["c"] = (k["c"] + 1) % (50000 // B)
        return k["c"]

    aug = dict(mean=CIFAR_MEAN, std=CIFAR_STD, pad=4, flip=True, seed=0)

    def plain(x, y):
        c = cslice()
        ops.image_batch(ci, cl, slices[c], epoch=c, x=x, y=y, err_flag=err, **aug)

    def mix(x, y, prob=1.0):
        c = cslice()
        ops.image_batch_mix(ci, cl, slices[c], partners[c], prob=prob, epoch=c, x=x, y=y, err_flag=err, **aug)

    def mix_prob0(x, y):   # every hash and both sources' address arithmetic, but no box: only source i is loaded
        mix(x, y, prob=0.0)

    launches, outs = {}, {}
    for name, fn in (("image_batch_cifar_augment", plain), ("image_batch_mix_cifar_augment", mix),
                     ("image_batch_mix_cifar_augment_prob0", mix_prob0)):
        x, y = torch.empty((B, 3, 32, 32), device=dev), torch.empty(B, dtype=torch.int64, device=dev)
        src, dst = torch.randn_like(x), torch.empty_like(x)
        launches["copy_before_" + name] = lambda dst=dst, src=src: dst.copy_(src)
        launches[name] = lambda fn=fn, x=x, y=y: fn(x, y)
        outs[name] = y
    for fn in launches.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    reps = [time_each(launches, NL) for _ in range(R)]
    out["launch_ms"] = {name: stats([r[name] for r in reps]) for name in launches}
    pl, mx = "image_batch_cifar_augment", "image_batch_mix_cifar_augment"
    out["ratios_per_repeat"] = {
        "plain_over_its_copy": [round(r[pl] / r["copy_before_" + pl], 4) for r in reps],
        "mix_over_its_copy": [round(r[mx] / r["copy_before_" + mx], 4) for r in reps],
        "mix_over_plain": [round(r[mx] / r[pl], 4) for r in reps],
        "mix_prob0_over_plain": [round(r[mx + "_prob0"] / r[pl], 4) for r in reps]}
    sp, sm = out["launch_ms"][pl], out["launch_ms"][mx]
    out["plain_repeat_range_ms"] = round(sp["max_ms"] - sp["min_ms"], 4)
    out["mix_minus_plain_median_ms"] = round(sm["median_ms"] - sp["median_ms"], 4)
    wb = unpack_mixed(outs[mx])[2]
    out["last_mixed_batch"] = {"mean_wb": round(float(wb.mean()), 4), "empty_boxes": int((wb == 0).sum())}
    out["bytes"] = {"read_per_launch": B * 3072, "written_per_launch": B * 3072 * 4 + B * 8,
                    "copy_read_and_written": B * 3072 * 4}
    assert int(err.item()) == 0
    del ci, cl, launches

    # ---- (ii) the graphed steps
    soft = SoftCrossEntropy(0.1)
    from splitcnn.data import init_models
    from splitcnn.engine import SplitTrainer
    X, Y = make_pool(B, 4, dev)
    YM = torch.stack([mixed_labels(Y[i], i) for i in range(4)])
    soft0 = SoftCrossEntropy(0.0)
    trs = [SplitTrainer(*init_models(seed=0), device=dev, graph=True, **kw)
           for kw in ({}, {"loss": soft}, {}, {"loss": soft0})]
    for tr, labels in zip(trs, (Y, YM, Y, Y)):
        for i in range(4):
            tr.register_inputs(X[i], labels[i])
        for i in range(4):
            tr.step(X[i], labels[i])
    td, tn, tc, tz = trs
    out["k2"] = ab(lambda i: td.step(X[i % 4], Y[i % 4]), lambda i: tn.step(X[i % 4], YM[i % 4]),
                   lambda i: tc.step(X[i % 4], Y[i % 4]), lambda i: tz.step(X[i % 4], Y[i % 4]), R, NS)
    for tr in trs:
        tr.server.check_labels()
    del trs, td, tn, tc, tz

    from splitcnn.wide import SyntheticCIFAR, WideTrainer, init_wide_models
    data = SyntheticCIFAR(42)
    xs, ys = zip(*(data.batch(B) for _ in range(2)))
    XW, YW = torch.stack(xs).to(dev), torch.stack(ys).to(dev)
    YWM = torch.stack([mixed_labels(YW[i], 10 + i) for i in range(2)])
    tws = [WideTrainer(*init_wide_models(seed=0), device=dev, graph=True, **kw)
           for kw in ({}, {"loss": soft}, {}, {"loss": soft0})]
    for tw, labels in zip(tws, (YW, YWM, YW, YW)):
        for i in range(2):
            tw.register_inputs(XW[i], labels[i])
        for i in range(4):
            tw.step(XW[i % 2], labels[i % 2])
    wd_, wn, wc, wz = tws
    out["k5"] = ab(lambda i: wd_.step(XW[i % 2], YW[i % 2]), lambda i: wn.step(XW[i % 2], YWM[i % 2]),
                   lambda i: wc.step(XW[i % 2], YW[i % 2]), lambda i: wz.step(XW[i % 2], YW[i % 2]), R, NS)
    for tw in tws:
        tw.server.check_labels()
    out["label_smoothing"] = soft.label_smoothing
    print(json.dumps(out))


if __name__ == "__main__":
    main()
