#!/usr/bin/env python
"""What DP-SGD costs on the K5 step: one process, B = 4096, graphed steps, 7 interleaved repeats of
(plain, dp, control) where control is a second plain trainer — its distance from plain is the noise floor of the
comparison. Then every slk_wide_grad_sqnorm layer between its own HIP events next to the sparse wgrad launch of the
same layer (the same GEMM shape over the whole batch: the yardstick). Prints a table; no ratio is a pass condition.

    python tools/dp_ab.py > profiles/dp_ab.txt"""
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "split-learning-k8s_amd"))

from splitcnn import ops  # noqa: E402
from splitcnn.privacy import DPSGD  # noqa: E402
from splitcnn.wide import (SyntheticCIFAR, WideTrainer, _k, client_backward_slab_shapes,  # noqa: E402
                           init_wide_models)

B, REPEATS, STEPS = 4096, 7, 20
dev = torch.device("cuda:0")


def timed(fn, n=1):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(n):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / n


def main():
    x, y = (t.to(dev) for t in SyntheticCIFAR(42).batch(B))
    trainers = {"plain": WideTrainer(*init_wide_models(0), device=dev),
                "dp": WideTrainer(*init_wide_models(0), device=dev, dp=DPSGD(1.0, 1.0)),
                "control": WideTrainer(*init_wide_models(0), device=dev)}
    ins = {}
    for k, tr in trainers.items():
        ins[k] = tr.static_inputs(B)
        ins[k][0].copy_(x)
        ins[k][1].copy_(y)
        for _ in range(5):
            tr.step(*ins[k])
    ms = {k: [] for k in trainers}
    for _ in range(REPEATS):
        for k, tr in trainers.items():
            ms[k].append(timed(lambda: tr.step(*ins[k]), STEPS))
    print(f"K5 step, B = {B}, graphed, {REPEATS} interleaved repeats of {STEPS} steps (ms per step: median, min, max)")
    for k, v in ms.items():
        print(f"  {k:8s} {statistics.median(v):8.3f} {min(v):8.3f} {max(v):8.3f}")
    med = {k: statistics.median(v) for k, v in ms.items()}
    print(f"  dp / plain = {med['dp'] / med['plain']:.3f}   control / plain = {med['control'] / med['plain']:.3f}")

    c = trainers["dp"].client
    dcut = trainers["dp"].server._b("dcut", (B, 32, 8, 8, 8), torch.bfloat16)
    args = (ins["dp"][0], c._da1m, c._a1, c._dp2, c._code2, c._p2, dcut, c._code3)
    work = torch.empty(B, 6, device=dev)
    slabs = [torch.empty(s, device=dev) for s in client_backward_slab_shapes(B)]
    st = torch.cuda.current_stream(dev).cuda_stream
    wgrads = (lambda: _k("wide_conv1_wgrad", args[0].data_ptr(), args[1].data_ptr(), slabs[0].data_ptr(), B, st),
              lambda: _k("wide_conv2_wgrad", args[3].data_ptr(), args[4].data_ptr(), args[2].data_ptr(),
                         slabs[1].data_ptr(), B, st),
              lambda: _k("wide_conv3_wgrad", args[6].data_ptr(), args[7].data_ptr(), args[5].data_ptr(),
                         slabs[2].data_ptr(), B, st))
    print("per layer, ms per launch (median of 7 interleaved): slk_wide_grad_sqnorm layer | sparse wgrad of the layer")
    for i, name in enumerate(("conv1", "conv2", "conv3")):
        a, b = [], []
        for _ in range(REPEATS):
            a.append(timed(lambda: ops.wide_grad_sqnorm(*args, work=work, layers=1 << i), 5))
            b.append(timed(wgrads[i], 5))
        print(f"  {name}: {statistics.median(a):8.3f} | {statistics.median(b):8.3f}   ratio {statistics.median(a) / statistics.median(b):.2f}")


if __name__ == "__main__":
    main()
