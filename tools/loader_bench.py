"""Measurement only: what the device-resident input path costs, ONE process, B = 4096, seeded synthetic
datasets of the real sizes (60,000 x 28 x 28 and 50,000 x 3 x 32 x 32 u8, resident in HBM), HIP events; prints one
JSON line (stored as profiles/loader_ab.txt).

  (i)  per-batch time of slk_mnist_batch, slk_image_batch<1,28,28> without augmentation, slk_image_batch<3,32,32>
       without and with augmentation (pad 4, flip), and in front of each a device-to-device copy of as many bytes
       as the launch writes (the bandwidth yardstick of this process; the copy also reads that many): the eight
       launches interleaved one for one, R repeats of N rounds, every launch between its own pair of events; each
       round gathers another slice of one permutation of the dataset into the kernel's own output buffers;
  (ii) the K5 graphed step fed by CifarLoader(augment=Augment()) against the same trainer stepping on two fixed
       preloaded buffers, and the loader iterated alone (its launches with no step between them), interleaved
       repeat by repeat, R repeats of N steps; then the host time of one epoch's permutation and its upload.

usage: python tools/loader_bench.py [--repeats 7] [--launches 48] [--launches-only]"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "split-learning-k8s_amd"), ROOT]
from eval_bench import ev, stats, time_each, time_loop  # noqa: E402
from splitcnn import ops  # noqa: E402
from splitcnn.cifar import CIFAR_MEAN, CIFAR_STD, Augment, CifarLoader  # noqa: E402

B = 4096


class Synthetic:
    """A dataset-shaped holder of seeded random u8 images and labels (what CifarBin / MnistIDX expose)."""

    def __init__(self, n, shape, seed):
        g = torch.Generator().manual_seed(seed)
        self.images = torch.randint(0, 256, (n,) + shape, dtype=torch.uint8, generator=g).numpy()
        self.labels = torch.randint(0, 10, (n,), dtype=torch.uint8, generator=g).numpy()

    def __len__(self):
        return len(self.images)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--launches", type=int, default=48)
    ap.add_argument("--launches-only", action="store_true", help="part (i) only")
    args = ap.parse_args()
    R, N = max(args.repeats, 3), max(args.launches, 24)
    dev = torch.device("cuda:0")
    out = {"tool": "loader_bench", "B": B, "repeats": R, "launches_per_repeat": N}

    # ---- (i) the launches
    mn, cf = Synthetic(60000, (28, 28), 1), Synthetic(50000, (3, 32, 32), 2)
    mi, ml = torch.from_numpy(mn.images).to(dev), torch.from_numpy(mn.labels).to(dev)
    ci, cl = torch.from_numpy(cf.images).to(dev), torch.from_numpy(cf.labels).to(dev)
    g = torch.Generator().manual_seed(3)
    mperm, cperm = torch.randperm(60000, generator=g).to(dev), torch.randperm(50000, generator=g).to(dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    k = {"m": 0, "c": 0}

    def mslice():
        k["m"] = (k["m"] + 1) % (60000 // B)
        return mperm[k["m"] * B:(k["m"] + 1) * B]

    def cslice():
        k["c"] = (k["c"] + 1) % (50000 // B)
        return cperm[k["c"] * B:(k["c"] + 1) * B]

    M1, S1 = (ops.MNIST_MEAN,), (ops.MNIST_STD,)
    kernels = {
        "mnist_batch": ((1, 28, 28), lambda x, y: ops.mnist_batch(mi, ml, mslice(), x=x, y=y, err_flag=err)),
        "image_batch_mnist_plain": ((1, 28, 28), lambda x, y: ops.image_batch(mi, ml, mslice(), mean=M1, std=S1, x=x, y=y,
                                                                               err_flag=err)),
        "image_batch_cifar_plain": ((3, 32, 32), lambda x, y: ops.image_batch(ci, cl, cslice(), mean=CIFAR_MEAN,
                                                                               std=CIFAR_STD, x=x, y=y, err_flag=err)),
        "image_batch_cifar_augment": ((3, 32, 32), lambda x, y: ops.image_batch(
            ci, cl, cslice(), mean=CIFAR_MEAN, std=CIFAR_STD, pad=4, flip=True, seed=0, epoch=k["c"], x=x, y=y,
            err_flag=err)),
    }
    # every kernel has its own output pair and, right in front of it, its own yardstick copy of as many bytes
    # (own source and destination): each launch then meets the caches as one round of all eight left them
    launches = {}

    def add(name, shape, fn):
        x, y = torch.empty((B,) + shape, device=dev), torch.empty(B, dtype=torch.int64, device=dev)
        src, dst = torch.randn_like(x), torch.empty_like(x)
        launches["copy_before_" + name] = lambda: dst.copy_(src)
        launches[name] = lambda: fn(x, y)

    for name, (shape, fn) in kernels.items():
        add(name, shape, fn)
    for fn in launches.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    reps = [time_each(launches, N) for _ in range(R)]
    out["launch_ms"] = {name: stats([r[name] for r in reps]) for name in launches}
    out["bytes"] = {"mnist_read": B * 784, "mnist_written": B * 784 * 4 + B * 8, "cifar_read": B * 3072,
                    "cifar_written": B * 3072 * 4 + B * 8, "copy_mnist_read_and_written": B * 784 * 4,
                    "copy_cifar_read_and_written": B * 3072 * 4}
    out["ratios_per_repeat"] = {f"{name}_over_its_copy": [round(r[name] / r["copy_before_" + name], 4) for r in reps]
                                for name in kernels}
    out["ratios_per_repeat"].update({
        "image_batch_mnist_plain_over_mnist_batch": [round(r["image_batch_mnist_plain"] / r["mnist_batch"], 4) for r in reps],
        "cifar_augment_over_cifar_plain": [round(r["image_batch_cifar_augment"] / r["image_batch_cifar_plain"], 4)
                                           for r in reps]})
    assert int(err.item()) == 0

    if args.launches_only:
        print(json.dumps(out))
        return

    # ---- (ii) the K5 step fed by the loader
    from splitcnn.wide import WideTrainer, init_wide_models
    ld = CifarLoader(cf, batch_size=B, seed=0, device=dev, drop_last=True, augment=Augment())
    tw = WideTrainer(*init_wide_models(seed=0), device=dev, graph=True)
    fixed = [(x.clone(), y.clone()) for (x, y), _ in zip(ld, range(2))]
    for x, y in fixed + [ld._buf(0, B), ld._buf(1, B)]:
        assert tw.register_inputs(x, y)
    nb = len(ld)

    def loader_loop(step):
        """ms per batch of N batches from the loader (whole epochs, their permutations included)."""
        s, e = ev(), ev()
        done = 0
        s.record()
        while done < N:
            for x, y in ld:
                if step:
                    tw.step(x, y)
                done += 1
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e) / done

    loader_loop(True)
    time_loop(lambda i: tw.step(*fixed[i % 2]), 8)
    k5 = {"step_fixed_buffers": [], "step_from_loader": [], "loader_alone": []}
    for _ in range(R):
        k5["step_fixed_buffers"].append(time_loop(lambda i: tw.step(*fixed[i % 2]), N))
        k5["step_from_loader"].append(loader_loop(True))
        k5["loader_alone"].append(loader_loop(False))
    out["k5"] = {name: stats(v) for name, v in k5.items()}
    # the once-per-epoch host work inside both loader loops: torch.randperm(n) and its blocking upload
    perm_ms = []
    for _ in range(R):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ld.order().to(dev)
        torch.cuda.synchronize()
        perm_ms.append((time.perf_counter() - t0) * 1e3)
    out["k5"]["epoch_permutation_host_ms"] = stats(perm_ms)
    out["k5"]["epoch_permutation_per_batch_ms"] = round(out["k5"]["epoch_permutation_host_ms"]["median_ms"] / nb, 4)
    sf, sl = out["k5"]["step_fixed_buffers"], out["k5"]["step_from_loader"]
    out["k5"].update({
        "batches_per_epoch": nb, "batches_per_repeat": -(-N // nb) * nb,
        "fixed_repeat_range_ms": round(sf["max_ms"] - sf["min_ms"], 4),
        "loader_minus_fixed_median_ms": round(sl["median_ms"] - sf["median_ms"], 4),
        "loader_over_fixed_per_repeat": [round(b / a, 4) for a, b in zip(k5["step_fixed_buffers"], k5["step_from_loader"])],
        "fixed_samples_per_s": round(B / (sf["median_ms"] * 1e-3)),
        "loader_samples_per_s": round(B / (sl["median_ms"] * 1e-3)),
        "caller_graphs": tw._n_caller_graphs(B)})
    assert int(ld.err.item()) == 0
    print(json.dumps(out))


if __name__ == "__main__":
    main()
