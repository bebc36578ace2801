"""The momentum / weight-decay / device-learning-rate kernels (slk_sgdm_*, slk_adamw_*) against torch's own
optimizers in float64, and bit for bit against the entry points they extend.

The float64 reference is torch.optim.SGD / AdamW / Adam on CPU, restarted every step from the device's f32
state and fed the gradient the kernel itself wrote, so only the update formula is under test. The C ABI takes
its hyper-parameters as `float` and the rate from an f32 table, so the reference gets exactly those f32
values (float(np.float32(0.9)), ...): the kernels are compared with torch at the numbers they were given.
Bound per element (the project's Adam-formula bound, tests/test_wide_gpu.py):
    |got - want| <= 1e-6 * max|want - before| + 2 * eps_f32 * |want|."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N = 5000
EPS32 = np.finfo(np.float32).eps


def f32(x):
    return float(np.float32(x))


def _np(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _t64(a):
    """A float64 CPU tensor with its own memory (the torch optimizer steps in place)."""
    return torch.from_numpy(np.array(a, dtype=np.float64, copy=True))


def within(got, want, before):
    tol = 1e-6 * np.abs(want - before).max() + 2 * EPS32 * np.abs(want)
    return bool((np.abs(got - want) <= tol).all())


_SLABS = {}


def slabs_for(nslab, gpu, n=N):
    """One slab set per (slab count, width), shared by every test and never written."""
    key = (nslab, n)
    if key not in _SLABS:
        g = torch.Generator(device=gpu).manual_seed(1000 + nslab)
        _SLABS[key] = torch.randn(nslab, n, device=gpu, generator=g) * 1e-2
    return _SLABS[key]


def _state(gpu, seed, n=N):
    g = torch.Generator(device=gpu).manual_seed(seed)
    return torch.randn(n, device=gpu, generator=g) * 0.1, torch.randn(n, device=gpu, generator=g)


SGD_CONFIGS = {
    "momentum": dict(momentum=0.9),
    "nesterov": dict(momentum=0.9, nesterov=True),
    "dampening": dict(momentum=0.9, dampening=0.5),
    "weight_decay": dict(weight_decay=5e-4),
    "all": dict(momentum=0.9, nesterov=True, weight_decay=5e-4),
}


@pytest.mark.parametrize("nslab", [1, 16, 17, 64, 65])
@pytest.mark.parametrize("name", sorted(SGD_CONFIGS))
def test_sgdm_matches_torch_sgd_float64(gpu, nslab, name):
    """Three steps on a table [0.1, 0.05]: step 0 initialises the buffer (over garbage), step 1 runs the
    recurrence, step 2 reads past the table's end (the last rate holds)."""
    from splitcnn import ops
    cfg = SGD_CONFIGS[name]
    slabs = slabs_for(nslab, gpu)
    table = torch.tensor([0.1, 0.05], device=gpu)
    rates = [f32(0.1), f32(0.05), f32(0.05)]
    p, buf = _state(gpu, 7)          # buf starts as garbage: the first step must overwrite it
    grad = torch.empty_like(p)
    step = torch.zeros(1, dtype=torch.int32, device=gpu)
    want_grad = ops.reduce_slabs(slabs)
    tcfg = dict(momentum=f32(cfg.get("momentum", 0.0)), dampening=f32(cfg.get("dampening", 0.0)),
                nesterov=cfg.get("nesterov", False), weight_decay=f32(cfg.get("weight_decay", 0.0)))
    for k in range(3):
        p0, buf0 = _np(p), _np(buf)
        ops.sgdm_from_slabs(p, grad, buf, slabs, table, step, **cfg)
        ops.tick(step)
        assert torch.equal(grad, want_grad), "grad is the fixed-order slab sum, before weight decay"
        ref = torch.nn.Parameter(_t64(p0))
        opt = torch.optim.SGD([ref], lr=rates[k], **tcfg)
        if k > 0 and tcfg["momentum"] != 0:
            opt.state[ref]["momentum_buffer"] = _t64(buf0)
        ref.grad = _t64(_np(grad))
        opt.step()
        want_p = ref.detach().numpy()
        assert within(_np(p), want_p, p0), (name, nslab, k, np.abs(_np(p) - want_p).max())
        if tcfg["momentum"] != 0:
            want_buf = opt.state[ref]["momentum_buffer"].numpy()
            assert within(_np(buf), want_buf, buf0), (name, nslab, k, np.abs(_np(buf) - want_buf).max())
        else:
            assert np.array_equal(_np(buf), buf0)   # no momentum: the buffer is not touched
    assert int(step.item()) == 3


@pytest.mark.parametrize("nslab", [1, 16, 17, 64, 65])
def test_sgdm_plain_is_bitwise_sgd_from_slabs(gpu, nslab):
    from splitcnn import ops
    slabs = slabs_for(nslab, gpu)
    p, _ = _state(gpu, 3)
    pa, pb = p.clone(), p.clone()
    ga, gb = torch.empty_like(p), torch.empty_like(p)
    ops.sgd_from_slabs(pa, ga, slabs, 0.01)
    step = torch.full((1,), 5, dtype=torch.int32, device=gpu)
    ops.sgdm_from_slabs(pb, gb, None, slabs, torch.tensor([0.01], device=gpu), step)
    assert torch.equal(pa, pb) and torch.equal(ga, gb)
    assert not torch.equal(pa, p)


def test_sgdm_multi_bit_identical_to_separate_launches(gpu):
    """slk_sgdm_multi_from_slabs (every optimizer step + the loss log of a split step in one launch) ==
    slk_sgdm_from_slabs per segment + slk_loss_log, bit for bit; the loss ring counter ticks once. The
    segments are the K2 step's: client (128 slabs), conv2 (256), fc (64). Two steps: the second runs the
    momentum recurrence."""
    from splitcnn import ops
    g = torch.Generator(device=gpu).manual_seed(5)
    shapes = [(128, 320), (256, 18496), (64, 92170)]
    slabs = [torch.randn(s, device=gpu, generator=g) for s in shapes]
    params = [torch.randn(s[1], device=gpu, generator=g) for s in shapes]
    loss_i = torch.rand(4093, device=gpu, generator=g)
    cfg = dict(momentum=0.9, nesterov=True, weight_decay=5e-4)
    table = torch.tensor([0.05, 0.02], device=gpu)
    out = []
    for multi in (False, True):
        p = [t.clone() for t in params]
        gr = [torch.empty_like(t) for t in params]
        buf = [torch.full_like(t, 3.0) for t in params]
        ring = torch.zeros(8, device=gpu)
        ctr = torch.full((1,), 3, dtype=torch.int32, device=gpu)
        step = torch.zeros(1, dtype=torch.int32, device=gpu)
        for _ in range(2):
            if multi:
                ops.sgdm_multi_from_slabs(list(zip(p, gr, buf, slabs)), table, step,
                                          loss=(loss_i, 1.0 / 4093, ring, ctr), **cfg)
            else:
                for seg in zip(p, gr, buf, slabs):
                    ops.sgdm_from_slabs(*seg, table, step, **cfg)
                ops.loss_log(loss_i, 1.0 / 4093, ring, ctr)
            ops.tick(step)
        torch.cuda.synchronize()
        out.append((p + gr + buf + [ring], int(ctr.item()), int(step.item())))
    for a, b in zip(out[0][0], out[1][0]):
        assert torch.equal(a, b)
    assert out[0][1:] == out[1][1:] == (5, 2)
    assert not torch.equal(out[1][0][0], params[0])


# ------------------------------------------------------------------------------------------------ Adam
B1, B2, EPS, LR, WD = f32(0.9), f32(0.999), f32(1e-8), f32(1e-3), f32(0.01)


def _adam_slk(p, grad, m, v, slabs, lr, step):
    from splitcnn import _lib, ops
    _lib.call("slk_adam_from_slabs", p.data_ptr(), grad.data_ptr(), m.data_ptr(), v.data_ptr(), slabs.data_ptr(),
              slabs.shape[0], slabs.shape[1], lr, 0.9, 0.999, 1e-8, step.data_ptr(), ops._stream(p))


@pytest.mark.parametrize("nslab", [16, 17, 33, 64, 65])
@pytest.mark.parametrize("decoupled", [True, False])
def test_adamw_matches_torch_float64(gpu, nslab, decoupled):
    """Two steps (the second reads m, v and the counter the first wrote) against torch.optim.AdamW
    (decoupled) and torch.optim.Adam(weight_decay=...) in float64, for p, m and v."""
    from splitcnn import ops
    slabs = slabs_for(nslab, gpu)
    table = torch.tensor([1e-3, 5e-4], device=gpu)
    rates = [f32(1e-3), f32(5e-4)]
    p, _ = _state(gpu, 11)
    m, v, grad = torch.zeros_like(p), torch.zeros_like(p), torch.empty_like(p)
    step = torch.zeros(1, dtype=torch.int32, device=gpu)
    want_grad = ops.reduce_slabs(slabs)
    Opt = torch.optim.AdamW if decoupled else torch.optim.Adam
    for k in range(2):
        p0, m0, v0 = _np(p), _np(m), _np(v)
        ops.adamw_from_slabs(p, grad, m, v, slabs, table, step, 0.9, 0.999, 1e-8, weight_decay=0.01,
                             decoupled=decoupled)
        ops.tick(step)
        assert torch.equal(grad, want_grad)
        ref = torch.nn.Parameter(_t64(p0))
        opt = Opt([ref], lr=rates[k], betas=(B1, B2), eps=EPS, weight_decay=WD)
        opt.state[ref] = {"step": torch.tensor(float(k)), "exp_avg": _t64(m0), "exp_avg_sq": _t64(v0)}
        ref.grad = _t64(_np(grad))
        opt.step()
        st = opt.state[ref]
        assert int(st["step"]) == k + 1
        for what, got, want, before in (("p", p, ref.detach().numpy(), p0), ("m", m, st["exp_avg"].numpy(), m0),
                                        ("v", v, st["exp_avg_sq"].numpy(), v0)):
            assert within(_np(got), want, before), (what, nslab, k, np.abs(_np(got) - want).max())


@pytest.mark.parametrize("nslab", [16, 17, 33, 64, 65])
def test_adamw_without_decay_is_bitwise_adam_and_matches_float64(gpu, nslab):
    """weight_decay 0 and a one-entry table: bitwise slk_adam_from_slabs over two steps — which therefore
    stands under the float64 check as well, mid-slab reduction (17-64 slabs) included."""
    from splitcnn import ops
    slabs = slabs_for(nslab, gpu)
    p, _ = _state(gpu, 13)
    a = [p.clone(), torch.empty_like(p), torch.zeros_like(p), torch.zeros_like(p)]
    b = [t.clone() for t in a]
    sa, sb = (torch.zeros(1, dtype=torch.int32, device=gpu) for _ in range(2))
    table = torch.tensor([1e-3], device=gpu)
    for k in range(2):
        p0, m0, v0 = _np(a[0]), _np(a[2]), _np(a[3])
        _adam_slk(*a, slabs, 1e-3, sa)
        ops.tick(sa)
        ops.adamw_from_slabs(*b, slabs, table, sb, 0.9, 0.999, 1e-8, weight_decay=0.0)
        ops.tick(sb)
        for x, y in zip(a, b):
            assert torch.equal(x, y)
        ref = torch.nn.Parameter(_t64(p0))
        opt = torch.optim.Adam([ref], lr=LR, betas=(B1, B2), eps=EPS)
        opt.state[ref] = {"step": torch.tensor(float(k)), "exp_avg": _t64(m0), "exp_avg_sq": _t64(v0)}
        ref.grad = _t64(_np(a[1]))
        opt.step()
        st = opt.state[ref]
        for what, got, want, before in (("p", a[0], ref.detach().numpy(), p0), ("m", a[2], st["exp_avg"].numpy(), m0),
                                        ("v", a[3], st["exp_avg_sq"].numpy(), v0)):
            assert within(_np(got), want, before), (what, nslab, k, np.abs(_np(got) - want).max())
    assert not torch.equal(a[0], p)


def test_adamw_multi_bit_identical_to_separate_launches(gpu):
    from splitcnn import ops
    sets = [slabs_for(ns, gpu) for ns in (16, 33, 65)]
    out = []
    for multi in (False, True):
        segs = []
        for i, sl in enumerate(sets):
            p, _ = _state(gpu, 20 + i)
            segs.append((p, torch.empty_like(p), torch.zeros_like(p), torch.zeros_like(p), sl))
        step = torch.zeros(1, dtype=torch.int32, device=gpu)
        table = torch.tensor([1e-3, 5e-4], device=gpu)
        for _ in range(2):
            if multi:
                ops.adamw_multi_from_slabs(segs, table, step, 0.9, 0.999, 1e-8, weight_decay=0.01)
            else:
                for seg in segs:
                    ops.adamw_from_slabs(*seg, table, step, 0.9, 0.999, 1e-8, weight_decay=0.01)
            ops.tick(step)
        torch.cuda.synchronize()
        out.append([t for seg in segs for t in seg[:4]])
    for x, y in zip(*out):
        assert torch.equal(x, y)
