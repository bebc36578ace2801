#!/usr/bin/env python
"""Record the libslk.so launches of one training step for every optimizer recipe and stepping path.

The host layer between the trainers and the kernels (splitcnn/recipe.py and the stages' step methods) has one
output: the sequence of slk_* entry points it calls and the arguments it passes by value. This tool writes that
sequence to tests/golden/step_launches.json; tests/test_step_launches_gpu.py holds the tree to it. A change that
alters launches on purpose regenerates the file with this tool on its own tree and says so; a refactor records it
on its parent commit and must reproduce it.

    python tools/record_step_launches.py [--out tests/golden/step_launches.json] [--commit HASH]

Only public constructors and methods plus splitcnn._lib.call (and the argument types next to it) are used, so the
same file runs on older trees. Per configuration two eager steps run (graph=False) and the second is recorded: the
first differs by lazily allocated buffers. A record is [entry, arg, ...]: an argument passed by value is its
Python int or float, a pointer or host array is "p", None is null. K2 runs at B = 16, K5 at B = 8 (the sequence
does not depend on B).
"""
import argparse
import contextlib
import ctypes
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "split-learning-k8s_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import torch  # noqa: E402

from splitcnn import _lib, optim  # noqa: E402
from splitcnn.codec import Fp8Cut  # noqa: E402
from splitcnn.loss import SoftCrossEntropy  # noqa: E402

K2_B, K5_B = 16, 8
GOLDEN = os.path.join(ROOT, "tests", "golden", "step_launches.json")


@contextlib.contextmanager
def recording(out):
    """Append a record to `out` for every _lib.call inside the block; the call still goes through."""
    real = _lib.call

    def call(name, *args):
        types = _lib._SIGS[name]
        assert len(types) == len(args), name
        out.append([name] + [None if a is None else "p" if t is ctypes.c_void_p else
                             float(a) if t in (ctypes.c_float, ctypes.c_double) else int(a)
                             for t, a in zip(types, args)])
        real(name, *args)
    _lib.call = call
    try:
        yield out
    finally:
        _lib.call = real


# ---- the optimizer configs (fresh objects per trainer: a ClipNorm / EMA / LRSchedule owns device memory)
def _sgd():
    return optim.SGD(0.05, momentum=0.9, nesterov=True, weight_decay=5e-4)


def _adamw():
    return optim.Adam(1e-3, weight_decay=0.01)


def _clip(dev):
    return optim.ClipNorm(1.0, device=dev)


def _ema(dev):
    return optim.EMA(0.999, device=dev)


def k2_batch(dev, B=K2_B):
    from splitcnn.data import SyntheticMNIST
    return tuple(t.to(dev) for t in SyntheticMNIST(7).batch(B))


def k5_batch(dev, B=K5_B):
    from splitcnn.wide import SyntheticCIFAR
    return tuple(t.to(dev) for t in SyntheticCIFAR(9).batch(B))


def k2_trainer(dev, graph=False, fuse_optim=True, **kw):
    from splitcnn.data import init_models
    from splitcnn.engine import SplitTrainer
    tr = SplitTrainer(*init_models(seed=3), device=dev, graph=graph, **kw)
    tr.server.fuse_optim = fuse_optim
    return tr


def k5_trainer(dev, graph=False, fuse_adam=True, **kw):
    from splitcnn.wide import WideTrainer, init_wide_models
    tr = WideTrainer(*init_wide_models(seed=0), device=dev, graph=graph, **kw)
    tr.client.fuse_adam = fuse_adam
    return tr


# name -> keyword arguments of the trainer, given the device
K2_TRAINERS = {
    "k2/default": lambda d: {},
    "k2/sgd": lambda d: dict(optim=_sgd()),
    "k2/schedule": lambda d: dict(schedule=optim.LRSchedule.from_values([0.05, 0.1, 0.075, 0.025], d)),
    "k2/clip": lambda d: dict(clip=_clip(d)),
    "k2/sgd+clip": lambda d: dict(optim=_sgd(), clip=_clip(d)),
    "k2/lars": lambda d: dict(optim=optim.LARS(0.1)),
    "k2/sgd+ema": lambda d: dict(optim=_sgd(), ema=_ema(d)),
    "k2/clip+ema": lambda d: dict(clip=_clip(d), ema=_ema(d)),
    "k2/lars+ema": lambda d: dict(optim=optim.LARS(0.1), ema=_ema(d)),
    "k2/soft": lambda d: dict(loss=SoftCrossEntropy(0.1)),
    "k2/default,client-backward-apart": lambda d: dict(fuse_client_backward=False),
    "k2/sgd,client-backward-apart": lambda d: dict(optim=_sgd(), fuse_client_backward=False),
    "k2/default,optim-apart": lambda d: dict(fuse_optim=False),
    "k2/sgd,optim-apart": lambda d: dict(optim=_sgd(), fuse_optim=False),
}
K5_TRAINERS = {
    "k5/default": lambda d: {},
    "k5/adamw": lambda d: dict(optim=_adamw()),
    "k5/clip": lambda d: dict(clip=_clip(d)),
    "k5/lamb": lambda d: dict(optim=optim.LAMB(2e-3)),
    "k5/adamw+ema": lambda d: dict(optim=_adamw(), ema=_ema(d)),
    "k5/default+ema": lambda d: dict(ema=_ema(d)),
    "k5/default,adam-apart": lambda d: dict(fuse_adam=False),
    "k5/adamw,adam-apart": lambda d: dict(optim=_adamw(), fuse_adam=False),
    "k5/fp8-cut": lambda d: dict(cut_codec=Fp8Cut()),
}
# the stages on their own: the standalone K2 stages (gradient block, then step()) and the K5 hub path on one GPU
K2_STAGES = {
    "k2/stages,default": lambda d: {},
    "k2/stages,sgd+clip": lambda d: dict(optim=_sgd(), clip=_clip(d)),
}
K5_STAGES = {
    "k5/hub,default": lambda d: {},
    "k5/hub,adamw": lambda d: dict(optim=_adamw()),
}


class K2Stages:
    """ClientStage.backward + step() and ServerStage.compute + step(): each stage steps from its gradient block."""

    def __init__(self, dev, **kw):
        from splitcnn.data import init_models
        from splitcnn.engine import ClientStage, ServerStage
        a, b = init_models(seed=3)
        self.client = ClientStage(a, device=dev, **kw)
        self.server = ServerStage(b, device=dev, optim=self.client.optim, schedule=self.client.schedule,
                                  clip=self.client.clip)

    def step(self, x, y):
        act = self.client.forward(x)
        cut_grad, loss_i = self.server.compute(act, y, 1.0 / x.shape[0])
        self.server.log_loss(loss_i)
        self.server.step()
        self.client.backward(cut_grad)
        self.client.step()


class K5Hub:
    """The hub's calls on one GPU: accumulate x 2 + finish_step(2) on the server, backward_grads + step_from_grads
    on the client."""

    def __init__(self, dev, **kw):
        from splitcnn.wide import WideClientStage, WideServerStage, init_wide_models
        a, b = init_wide_models(seed=0)
        self.client = WideClientStage(a, dev, **kw)
        self.server = WideServerStage(b, dev, optim=self.client.optim, schedule=self.client.schedule,
                                      clip=self.client.clip)
        self.dcut = None

    def step(self, x, y):
        B, h = x.shape[0], x.shape[0] // 2
        cut = self.client.forward(x)
        if self.dcut is None:
            self.dcut = torch.empty_like(cut)
        for k, (lo, hi) in enumerate(((0, h), (h, B))):
            self.server.accumulate(cut[lo:hi], y[lo:hi], 1.0 / B, lo, k, 2, dcut=self.dcut[lo:hi])
        self.server.finish_step(2)
        self.client.backward_grads(self.dcut)
        self.client.step_from_grads()


def configurations(dev, graph=False):
    """(name, runner with .step(x, y) / .client / .server, batch) of every configuration, built one at a time."""
    for name, kw in K2_TRAINERS.items():
        yield name, k2_trainer(dev, graph=graph, **kw(dev)), k2_batch(dev)
    for name, kw in K2_STAGES.items():
        yield name, K2Stages(dev, **kw(dev)), k2_batch(dev)
    for name, kw in K5_TRAINERS.items():
        yield name, k5_trainer(dev, graph=graph, **kw(dev)), k5_batch(dev)
    for name, kw in K5_STAGES.items():
        yield name, K5Hub(dev, **kw(dev)), k5_batch(dev)


def record_all(dev):
    """{name: the records of the second eager step}."""
    out = {}
    for name, runner, (x, y) in configurations(dev):
        runner.step(x, y)
        with recording([]) as rec:
            runner.step(x, y)
        torch.cuda.synchronize()
        out[name] = rec
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=GOLDEN)
    ap.add_argument("--commit", default=None, help="the commit this tree is (default: git rev-parse HEAD)")
    args = ap.parse_args()
    commit = args.commit or subprocess.run(["git", "rev-parse", "HEAD"], cwd=ROOT, capture_output=True,
                                           text=True).stdout.strip() or "unknown"
    steps = record_all(torch.device("cuda:0"))
    doc = {"recorded_on_commit": commit, "build_id": _lib.build_id(), "batch": {"k2": K2_B, "k5": K5_B},
           "format": "[entry, arg, ...]: by-value arguments as numbers, pointers and host arrays \"p\", None null",
           "steps": steps}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("{\n")
        for k in ("recorded_on_commit", "build_id", "batch", "format"):
            f.write(f" {json.dumps(k)}: {json.dumps(doc[k])},\n")
        f.write(' "steps": {\n')
        for i, (name, rec) in enumerate(steps.items()):
            rows = ",\n".join("   " + json.dumps(r) for r in rec)
            f.write(f"  {json.dumps(name)}: [\n{rows}\n  ]{',' if i + 1 < len(steps) else ''}\n")
        f.write(" }\n}\n")
    print(f"{args.out}: {len(steps)} configurations, {sum(len(r) for r in steps.values())} launches, commit {commit[:12]}")


if __name__ == "__main__":
    main()
