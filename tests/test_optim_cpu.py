"""CPU-side checks of splitcnn.optim: the configs validate like torch's optimizers, LRSchedule records torch
schedulers element for element, the new C-ABI entry points validate their arguments without a launch, the
multi-GPU classes refuse a configured stage, and a configured stage constructs without touching a kernel."""
import ctypes
import math
import types

import numpy as np
import pytest
import torch

from splitcnn import optim


@pytest.mark.parametrize("kwargs", [dict(lr=-0.1), dict(lr=0.1, momentum=-0.5), dict(lr=0.1, weight_decay=-1e-4),
                                    dict(lr=0.1, nesterov=True), dict(lr=0.1, momentum=0.9, dampening=0.5, nesterov=True)])
def test_sgd_config_raises_like_torch(kwargs):
    p = [torch.nn.Parameter(torch.zeros(1))]
    with pytest.raises(ValueError) as want:
        torch.optim.SGD(p, **kwargs)
    with pytest.raises(ValueError) as got:
        optim.SGD(**kwargs)
    assert str(got.value) == str(want.value)


@pytest.mark.parametrize("kwargs", [dict(lr=-1e-3), dict(eps=-1e-8), dict(betas=(1.0, 0.999)), dict(betas=(0.9, -0.1)),
                                    dict(weight_decay=-0.01)])
def test_adam_config_raises_like_torch(kwargs):
    p = [torch.nn.Parameter(torch.zeros(1))]
    with pytest.raises(ValueError) as want:
        torch.optim.AdamW(p, **kwargs)
    with pytest.raises(ValueError) as got:
        optim.Adam(**kwargs)
    assert str(got.value) == str(want.value)


def test_configs_accept_what_torch_accepts():
    c = optim.SGD(0.05, momentum=0.9, nesterov=True, weight_decay=5e-4)
    assert c.kernel_args() == {"momentum": 0.9, "dampening": 0.0, "weight_decay": 5e-4, "nesterov": True}
    a = optim.Adam(2e-3, (0.8, 0.99), 1e-6, weight_decay=0.01, decoupled=False)
    assert a.kernel_args() == {"beta1": 0.8, "beta2": 0.99, "eps": 1e-6, "weight_decay": 0.01, "decoupled": False}
    assert optim.Adam().decoupled and optim.Adam().lr == 1e-3


def _torch_values(make, base_lr, steps):
    opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=base_lr)
    sched = make(opt)
    out = []
    for _ in range(steps):
        out.append(sched.get_last_lr()[0])
        opt.step()
        sched.step()
    return np.asarray(out, dtype=np.float32)


SCHEDULERS = {
    "StepLR": lambda o: torch.optim.lr_scheduler.StepLR(o, step_size=3, gamma=0.5),
    "CosineAnnealingLR": lambda o: torch.optim.lr_scheduler.CosineAnnealingLR(o, T_max=10, eta_min=1e-4),
    "warmup LambdaLR": lambda o: torch.optim.lr_scheduler.LambdaLR(o, lambda k: min(1.0, (k + 1) / 4)),
}


@pytest.mark.parametrize("name", sorted(SCHEDULERS))
def test_from_torch_equals_the_scheduler(name):
    sched = optim.LRSchedule.from_torch(SCHEDULERS[name], 0.1, 12, device="cpu")
    want = _torch_values(SCHEDULERS[name], 0.1, 12)
    assert len(sched) == 12 and sched.table.dtype == torch.float32 and sched.table.device.type == "cpu"
    assert np.array_equal(sched.table.numpy(), want)
    assert np.array_equal(sched.values, want)
    assert len(set(want.tolist())) > 1   # the schedule moves


def test_from_torch_records_a_fixed_length_scheduler_to_its_end():
    """OneCycleLR raises when stepped past total_steps: all of its values are recorded, no step beyond."""
    make = lambda o: torch.optim.lr_scheduler.OneCycleLR(o, max_lr=0.1, total_steps=10)  # noqa: E731
    s = optim.LRSchedule.from_torch(make, 0.1, 10, device="cpu")
    opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=0.1)
    sched, want = make(opt), []
    for k in range(10):
        want.append(sched.get_last_lr()[0])
        if k < 9:
            opt.step()
            sched.step()
    assert np.array_equal(s.values, np.asarray(want, dtype=np.float32)) and s.values.max() == np.float32(0.1)


def test_convenience_schedules():
    s = optim.LRSchedule.step_decay(0.1, step_size=2, gamma=0.1, steps=6, device="cpu")
    assert np.array_equal(s.values, np.asarray([0.1, 0.1, 0.1 * 0.1, 0.1 * 0.1, 0.1 * 0.1 * 0.1, 0.1 * 0.1 * 0.1],
                                               dtype=np.float32))
    w = optim.LRSchedule.warmup_cosine(0.2, warmup=4, total=20, min_lr=0.02, device="cpu")
    v = w.values.astype(np.float64)
    assert len(w) == 20
    assert np.allclose(v[:4], 0.2 * np.arange(1, 5) / 4, rtol=1e-6)          # linear warm-up to the base rate
    assert np.all(np.diff(v[4:]) < 0) and math.isclose(v[4], 0.2, rel_tol=1e-6)   # then a falling cosine
    assert math.isclose(v[-1], 0.02, rel_tol=1e-6)                           # ending at min_lr
    assert math.isclose(v[4 + 15 // 2 + 1], 0.5 * (0.2 + 0.02), rel_tol=0.1)  # half-way near the midpoint
    with pytest.raises(ValueError):
        optim.LRSchedule.warmup_cosine(0.1, warmup=5, total=5, device="cpu")


def test_schedule_clamps_and_set_lr():
    s = optim.LRSchedule.from_values([0.1, 0.05, 0.025], device="cpu")
    assert [s.lr_at(k) for k in (-1, 0, 1, 2, 3, 1000)] == [np.float32(x) for x in (0.1, 0.1, 0.05, 0.025, 0.025, 0.025)]
    with pytest.raises(ValueError, match="constant"):
        s.set_lr(0.01)
    c = optim.LRSchedule.constant(0.01, device="cpu")
    ptr = c.table.data_ptr()
    c.set_lr(0.002)
    assert c.table.data_ptr() == ptr and c.table.tolist() == [np.float32(0.002)] and c.lr_at(7) == np.float32(0.002)
    for bad in ([], [0.1, float("nan")], [-0.1]):
        with pytest.raises(ValueError):
            optim.LRSchedule.from_values(bad, device="cpu")


def _arr(ctype, *vals):
    return ctypes.cast((ctype * 4)(*vals), ctypes.c_void_p)


def test_new_entry_points_validate_without_gpu():
    """1 = hipErrorInvalidValue on null pointers, lr_len < 1 and nseg > 4; 0 on n == 0; never a launch (the
    non-null arguments here are dummy addresses no kernel gets to read)."""
    from splitcnn import _lib
    lib = _lib.load()
    D = 4096   # a dummy non-null "device pointer"
    P, I = ctypes.c_void_p, ctypes.c_int
    # single-segment forms
    assert lib.slk_sgdm_from_slabs(None, None, None, None, 1, 8, None, 1, None, 0.9, 0.0, 0.0, 0, None) == 1
    assert lib.slk_sgdm_from_slabs(D, None, D, D, 1, 8, D, 0, D, 0.9, 0.0, 0.0, 0, None) == 1       # lr_len 0
    assert lib.slk_sgdm_from_slabs(D, None, None, D, 1, 8, D, 1, D, 0.9, 0.0, 0.0, 0, None) == 1    # momentum, no buf
    assert lib.slk_sgdm_from_slabs(D, None, D, D, 1, 8, D, 1, None, 0.9, 0.0, 0.0, 0, None) == 1    # no step counter
    assert lib.slk_sgdm_from_slabs(D, None, D, D, 1, 0, D, 1, D, 0.9, 0.0, 0.0, 0, None) == 0       # n == 0
    assert lib.slk_adamw_from_slabs(None, None, None, None, None, 1, 8, None, 1, None, 0.9, 0.999, 1e-8, 0.0, 1, None) == 1
    assert lib.slk_adamw_from_slabs(D, None, D, D, D, 1, 8, D, 0, D, 0.9, 0.999, 1e-8, 0.0, 1, None) == 1   # lr_len 0
    assert lib.slk_adamw_from_slabs(D, None, D, D, D, 1, 8, None, 1, D, 0.9, 0.999, 1e-8, 0.0, 1, None) == 1  # no table
    assert lib.slk_adamw_from_slabs(D, None, D, D, D, 1, 0, D, 1, D, 0.9, 0.999, 1e-8, 0.0, 1, None) == 0   # n == 0
    # multi forms: host arrays of 4 entries
    ptrs, nul, ones, zeros = _arr(P, D, D, D, D), _arr(P, None, None, None, None), _arr(I, 1, 1, 1, 1), _arr(I, 0, 0, 0, 0)
    sgdm = lib.slk_sgdm_multi_from_slabs
    tail = (0.9, 0.0, 0.0, 0, None, 0, 0.0, None, 0, None, None)
    assert sgdm(ptrs, None, ptrs, ptrs, ones, ones, 5, D, 1, D, *tail) == 1        # nseg > 4
    assert sgdm(ptrs, None, ptrs, ptrs, ones, ones, 2, D, 0, D, *tail) == 1        # lr_len 0
    assert sgdm(ptrs, None, ptrs, ptrs, ones, ones, 2, None, 1, D, *tail) == 1     # no table
    assert sgdm(nul, None, ptrs, ptrs, ones, ones, 2, D, 1, D, *tail) == 1         # null params
    assert sgdm(ptrs, None, nul, ptrs, ones, ones, 2, D, 1, D, *tail) == 1         # momentum, null bufs
    assert sgdm(ptrs, None, ptrs, ptrs, ones, zeros, 2, D, 1, D, *tail) == 0       # every n == 0, no loss: no launch
    adamw = lib.slk_adamw_multi_from_slabs
    hyper = (0.9, 0.999, 1e-8, 0.01, 1, None)
    assert adamw(ptrs, None, ptrs, ptrs, ptrs, ones, ones, 5, D, 1, D, *hyper) == 1
    assert adamw(ptrs, None, ptrs, ptrs, ptrs, ones, ones, 2, D, 0, D, *hyper) == 1
    assert adamw(ptrs, None, nul, ptrs, ptrs, ones, ones, 2, D, 1, D, *hyper) == 1
    assert adamw(ptrs, None, ptrs, ptrs, ptrs, ones, ones, 2, D, 1, None, *hyper) == 1
    assert adamw(ptrs, None, ptrs, ptrs, ptrs, ones, zeros, 2, D, 1, D, *hyper) == 0
    assert lib.slk_abi_version() == 1


def test_configured_stage_constructs_on_cpu_without_a_kernel():
    from splitcnn import ops
    from splitcnn.engine import ClientStage, ServerStage
    cfg = optim.SGD(0.05, momentum=0.9, nesterov=True, weight_decay=5e-4)
    sched = optim.LRSchedule.from_values([0.05, 0.01], device="cpu")
    c = ClientStage(device="cpu", optim=cfg, schedule=sched)
    s = ServerStage(device="cpu", optim=cfg)
    assert c.optim is cfg and c.schedule is sched and c.lr == 0.05
    assert c.buf.shape == (ops.CLIENT_NPARAM,) and s.buf.shape == (ops.SERVER_NPARAM,)
    assert not c.buf.any() and not s.buf.any()
    assert c.step_ctr.dtype == torch.int32 and int(c.step_ctr) == 0 and c.auto_tick
    assert s.schedule.values.tolist() == [np.float32(0.05)]       # a constant table from the config's lr
    # a schedule alone implies the stage's plain SGD at its lr; nothing at all keeps today's path
    only = ServerStage(device="cpu", lr=0.02, schedule=optim.LRSchedule.constant(0.02, device="cpu"))
    assert only.optim.momentum == 0.0 and only.optim.lr == 0.02
    plain = ClientStage(device="cpu")
    assert plain.optim is None and plain.schedule is None and plain.buf is None and plain.step_ctr is None
    with pytest.raises(TypeError):
        ClientStage(device="cpu", optim=optim.Adam())
    with pytest.raises(RuntimeError, match="no CPU fallback"):    # the step itself needs the device
        c.step()


def test_dist_classes_refuse_a_configured_stage():
    from splitcnn import dist
    from splitcnn.engine import ClientStage, ServerStage
    cfg = optim.SGD(0.01, momentum=0.9)
    plain_c, plain_s = ClientStage(device="cpu"), ServerStage(device="cpu")
    conf_c = ClientStage(device="cpu", optim=cfg)
    sched_s = ServerStage(device="cpu", schedule=optim.LRSchedule.constant(0.01, device="cpu"))
    wide = types.SimpleNamespace(optim=optim.Adam(weight_decay=0.01), schedule=None)   # a K5 stage needs the GPU
    cases = [lambda: dist.Replicated(conf_c, plain_s), lambda: dist.Replicated(plain_c, sched_s),
             lambda: dist.FedAvg(conf_c, plain_s), lambda: dist.Hub(conf_c, 0, 2), lambda: dist.Hub(sched_s, 1, 2),
             lambda: dist.Pipeline(conf_c, "client", 1), lambda: dist.UShaped(sched_s, "server", 0),
             lambda: dist.WideHub(wide, 0, 2)]
    for make in cases:
        with pytest.raises(ValueError, match="only the default optimizer"):
            make()
