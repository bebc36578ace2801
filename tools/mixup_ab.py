"""Measurement only: what slk_image_batch_blend costs, ONE process, B = 4096, HIP events; prints one JSON line (stored
as profiles/mixup_ab.txt).

  (i)  slk_image_batch_blend<3,32,32> (pad 4, flip) as MixUp at prob 1 (alpha 0.4), as the switch at prob 0.5 /
       switch 0.5 (alphas 1.0 / 0.4) and as table-CutMix at prob 1 (alpha 1.0), beside two yardsticks of the same
       process: slk_image_batch_mix at prob 1, and in front of each launch a device-to-device copy of as many bytes as
       it writes. The eight launches interleaved one for one, R repeats of N rounds, every launch between its own pair
       of events; each round gathers another slice of one permutation, partners the slice rolled by one.
       A MixUp sample reads both sources whole, 2 x 3072 B, where a launch writes 12288 B: (12288 + 6144) /
       (12288 + 3072) = 1.2 x the bytes of a CutMix sample (which reads about one source in all), so the MixUp launch
       is read against 1.2 x the CutMix launch of the same repeat.
  (ii) the graphed K5 step (loss=SoftCrossEntropy(0.1)) fed by a CifarLoader(mix=Mix()) against the same step fed by a
       CifarLoader(mix=CutMix()), and a second CutMix()-fed trainer as the control: whole epochs of 12 batches
       (drop_last) between one pair of events, interleaved repeat by repeat; ms per step, loader launch included.

usage: python tools/mixup_ab.py [--repeats 7] [--launches 48] [--epochs 4]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "split-learning-k8s_amd"), ROOT, os.path.join(ROOT, "tools")]
from eval_bench import ev, stats, time_each  # noqa: E402
from loader_bench import Synthetic  # noqa: E402
from splitcnn import ops  # noqa: E402
from splitcnn.cifar import CIFAR_MEAN, CIFAR_STD, Augment, CifarLoader  # noqa: E402
from splitcnn.loss import CutMix, Mix, MixUp, SoftCrossEntropy, mix_tables, unpack_mixed  # noqa: E402

B = 4096


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--launches", type=int, default=48)
    ap.add_argument("--epochs", type=int, default=4)
    args = ap.parse_args()
    R, NL, NE = max(args.repeats, 3), max(args.launches, 24), max(args.epochs, 1)
    dev = torch.device("cuda:0")
    out = {"tool": "mixup_ab", "B": B, "repeats": R, "launches_per_repeat": NL, "epochs_per_repeat": NE}

    # ---- (i) the launches
    cf = Synthetic(50000, (3, 32, 32), 2)
    ci, cl = torch.from_numpy(cf.images).to(dev), torch.from_numpy(cf.labels).to(dev)
    perm = torch.randperm(50000, generator=torch.Generator().manual_seed(3)).to(dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    slices = perm[:(50000 // B) * B].view(-1, B)
    partners = slices.roll(1, dims=1).contiguous()   # made once: only the launch itself sits between the events
    k = {"c": 0}

    def cslice():
        k["c"] = (k["c"] + 1) % (50000 // B)
        return k["c"]

    aug = dict(mean=CIFAR_MEAN, std=CIFAR_STD, pad=4, flip=True, seed=0)
    lam04 = mix_tables(MixUp(0.4), dev)[1]
    cut10, _ = mix_tables(Mix(1.0, 0.4), dev)

    def cutmix(x, y):
        c = cslice()
        ops.image_batch_mix(ci, cl, slices[c], partners[c], prob=1.0, epoch=c, x=x, y=y, err_flag=err, **aug)

    def blend(**tabs):
        def fn(x, y):
            c = cslice()
            ops.image_batch_blend(ci, cl, slices[c], partners[c], epoch=c, x=x, y=y, err_flag=err, **tabs, **aug)
        return fn

    launches, outs = {}, {}
    for name, fn in (("image_batch_mix_prob1", cutmix),
                     ("blend_mixup_prob1", blend(lam_table=lam04, prob=1.0)),
                     ("blend_switch_prob05_switch05", blend(cut_table=cut10, lam_table=lam04, prob=0.5, switch=0.5)),
                     ("blend_table_cutmix_prob1", blend(cut_table=cut10, prob=1.0))):
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
    names = [n for n in launches if not n.startswith("copy_before_")]
    cm, mu = "image_batch_mix_prob1", "blend_mixup_prob1"
    out["over_its_copy_per_repeat"] = {n: [round(r[n] / r["copy_before_" + n], 4) for r in reps] for n in names}
    out["over_image_batch_mix_per_repeat"] = {n: [round(r[n] / r[cm], 4) for r in reps] for n in names if n != cm}
    sc, sm = out["launch_ms"][cm], out["launch_ms"][mu]
    out["image_batch_mix_repeat_range_ms"] = round(sc["max_ms"] - sc["min_ms"], 4)
    out["mixup_bytes_over_cutmix_bytes"] = 1.2
    out["mixup_minus_1p2_x_image_batch_mix_median_ms"] = round(sm["median_ms"] - 1.2 * sc["median_ms"], 4)
    out["mixup_over_1p2_x_image_batch_mix_per_repeat"] = [round(r[mu] / (1.2 * r[cm]), 4) for r in reps]
    out["last_batches"] = {n: {"mean_wb": round(float(unpack_mixed(outs[n])[2].mean()), 4),
                               "plain_labels": int((outs[n] < 2 ** 32).sum())} for n in names}
    out["bytes"] = {"written_per_launch": B * 3072 * 4 + B * 8, "copy_read_and_written": B * 3072 * 4,
                    "read_per_launch_cutmix_about": B * 3072, "read_per_launch_mixup": 2 * B * 3072}
    assert int(err.item()) == 0
    del ci, cl, launches

    # ---- (ii) the graphed K5 step fed by a loader
    from splitcnn.wide import WideTrainer, init_wide_models
    soft = SoftCrossEntropy(0.1)

    def fed(mix):
        ld = CifarLoader(cf, batch_size=B, shuffle=True, seed=5, device=dev, drop_last=True, augment=Augment(), mix=mix)
        tr = WideTrainer(*init_wide_models(seed=0), device=dev, graph=True, loss=soft)
        for x, y in ld:       # one warm epoch: both buffer pairs get their graphs
            tr.step(x, y)
        torch.cuda.synchronize()
        return ld, tr

    def epochs(ld, tr):
        s, e = ev(), ev()
        n = 0
        s.record()
        for _ in range(NE):
            for x, y in ld:
                tr.step(x, y)
                n += 1
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e) / n

    runs = {"cutmix_fed_step": fed(CutMix()), "mix_fed_step": fed(Mix()), "control_cutmix_fed_step": fed(CutMix())}
    t = {name: [] for name in runs}
    for _ in range(R):
        for name, (ld, tr) in runs.items():
            t[name].append(epochs(ld, tr))
    for ld, tr in runs.values():
        tr.server.check_labels()
        assert int(ld.err.item()) == 0
    st = {name: stats(v) for name, v in t.items()}
    out["k5_step_ms"] = st
    out["k5"] = {"steps_per_epoch": len(runs["mix_fed_step"][0]),
                 "cutmix_fed_repeat_range_ms": round(st["cutmix_fed_step"]["max_ms"] - st["cutmix_fed_step"]["min_ms"], 4),
                 "mix_minus_cutmix_median_ms": round(st["mix_fed_step"]["median_ms"] - st["cutmix_fed_step"]["median_ms"], 4),
                 "control_minus_cutmix_median_ms": round(st["control_cutmix_fed_step"]["median_ms"]
                                                        - st["cutmix_fed_step"]["median_ms"], 4),
                 "mix_over_cutmix_per_repeat": [round(b / a, 4) for a, b in zip(t["cutmix_fed_step"], t["mix_fed_step"])],
                 "control_over_cutmix_per_repeat": [round(b / a, 4) for a, b in
                                                    zip(t["cutmix_fed_step"], t["control_cutmix_fed_step"])]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
