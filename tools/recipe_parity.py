#!/usr/bin/env python
"""Digests of what six seeded training steps leave behind, for every configuration of
tools/record_step_launches.py: run it on two trees and diff the output.

    python tools/recipe_parity.py > digests.txt

The trainers run with graph=True (the step captured once, then replayed); the stage-level configurations (the
standalone K2 stages, the K5 hub path) have no graph and run eagerly. Per configuration one line per parameter
block, per tensor of optimizer_state() (the stages' own state tensors where there is no trainer), the flushed loss
history and grad_norms() / trust_ratios() where the recipe defines them: `name what sha256[:16]`. The kernels are
atomic-free and reduce in fixed order, so equal code gives equal digests run to run. Public API only.
"""
import hashlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

from record_step_launches import configurations  # noqa: E402

STEPS = 6


def digest(a) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:16]


def _t(t):
    return t.detach().cpu().numpy()


def state_of(runner):
    """{what: numpy array} after the steps."""
    c, s = runner.client, runner.server
    out = {"client.params": _t(c.params), "server.params": _t(s.params)}
    if hasattr(runner, "optimizer_state"):
        out.update({f"optim.{k}": _t(v) for k, v in runner.optimizer_state().items()})
    else:
        for n, st in (("client", c), ("server", s)):
            for a in ("buf", "m", "v", "step_ctr"):
                if getattr(st, a, None) is not None:
                    out[f"optim.{n}.{a}"] = _t(getattr(st, a))
    torch.cuda.synchronize()
    out["loss"] = np.asarray(s.loss_log.flush(), dtype=np.float64)
    if c.clip is not None:
        norms = (runner.grad_norms() if hasattr(runner, "grad_norms")
                 else {n: tuple(st.clip_out.tolist()) for n, st in (("client", c), ("server", s))})
        out["grad_norms"] = np.asarray([norms[k] for k in sorted(norms)], dtype=np.float64)
    if c.trust_out is not None:
        if hasattr(runner, "trust_ratios"):
            out["trust_ratios"] = np.asarray([row for st in runner.trust_ratios().values() for row in st.values()],
                                             dtype=np.float64)
        else:
            out["trust_ratios"] = np.concatenate([_t(c.trust_out), _t(s.trust_out)]).astype(np.float64)
    return out


def main():
    dev = torch.device("cuda:0")
    for name, runner, (x, y) in configurations(dev, graph=True):
        gen = torch.Generator().manual_seed(1234)
        for _ in range(STEPS):
            perm = torch.randperm(x.shape[0], generator=gen).to(dev)
            runner.step(x[perm].contiguous(), y[perm].contiguous())
        for what, a in state_of(runner).items():
            print(f"{name:40s} {what:28s} {digest(a)}", flush=True)


if __name__ == "__main__":
    main()
