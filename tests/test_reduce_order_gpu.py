"""The fixed-order reductions of csrc/slk_optim.hip and csrc/slk_wide_head.hip pinned, bit for bit, to the summation
order include/slk.h documents (every multi-GPU bit-identity claim rests on it), plus plain SGD, the loss reductions
and the out-of-range fallback of slk_mnist_batch.

Slab reductions: n = 1300 columns (a partial last block of the 1024-, 256- and 64-column forms), values
randn * 10**U(-3, 3), slab counts 1, 7, 8, 9, 16 (ascending), 17, 33, 64 (4 strided partials), 65, 200 (16 strided
partials). tests/test_head_ref64_cpu.py shows that the float32 emulations of the three forms, the "prior added last"
wording and the rounded float64 sum all differ from each other in 39-90 % of the columns at these counts, so any
other order fails here. Every output has 64 floats of NaN sentinel behind it.

slk_sgd: torch.optim.SGD's `p.add_(g, alpha=-lr)` is a FUSED multiply-add on the CPU (ATen's vectorised add kernel
calls fmadd) and so is the kernel's `p - lr * g` (one v_fma_f32): the pinned value is the float32 expression with ONE
rounding, fl(p - lr g). Operands are chosen so that float64 holds p - lr g exactly (lr = 3 * 2^-8, |g| in [0.25, 4),
|p| in [2^-6, 2^-4): bits 2^-4 .. 2^-33), which makes the reference the correctly rounded value; the two-rounding
expression fl(p - fl(lr g)) differs from it in about a quarter of the elements and is asserted NOT to match.
"""
import ctypes

import numpy as np
import pytest
import torch

import head_ref64 as R

pytestmark = pytest.mark.gpu

NAN = float("nan")
N = 1300
SLAB_COUNTS = [1, 7, 8, 9, 16, 17, 33, 64, 65, 200]
PAD = 64


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _padded(values, dev):
    """A device buffer holding `values` followed by PAD NaNs; returns (buffer, view of the values)."""
    v = torch.as_tensor(values, dtype=torch.float32).reshape(-1)
    buf = torch.full((v.numel() + PAD,), NAN, dtype=torch.float32, device=dev)
    buf[:v.numel()] = v.to(dev)
    return buf, buf[:v.numel()]


def _nan_out(n, dev):
    return torch.full((n + PAD,), NAN, dtype=torch.float32, device=dev)


def _same_bits(got, want, what):
    got = got.detach().cpu().numpy().view(np.int32)
    want = np.asarray(want, dtype=np.float32).view(np.int32)
    bad = got != want
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} columns differ from the documented order"


def _ints(dev, *vals):
    return torch.tensor(vals, dtype=torch.int32, device=dev)


# ----------------------------------------------------------------------------- slab reductions
@pytest.mark.parametrize("nslab", SLAB_COUNTS)
def test_reduce_slabs_order(gpu, nslab):
    """slk_reduce_slabs, accumulate 0 and 1: the ascending form adds the prior LAST (prior + g), the 4- and 16-partial
    forms START their chain of partials at the prior (((prior + p0) + p1) + ...)."""
    from splitcnn import _lib
    s = R.reduce_case(nslab, N, 1000 + nslab)
    sd = torch.from_numpy(s).to(gpu)
    out = _nan_out(N, gpu)
    _lib.call("slk_reduce_slabs", sd.data_ptr(), nslab, N, out.data_ptr(), 0, _stream())
    torch.cuda.synchronize()
    R.assert_sentinel(out, N, "reduce out")
    _same_bits(out[:N], R.reduce_emulated(s), f"slk_reduce_slabs nslab={nslab}")
    prior = R.reduce_case(1, N, 2000 + nslab)[0]
    buf, acc = _padded(prior, gpu)
    _lib.call("slk_reduce_slabs", sd.data_ptr(), nslab, N, acc.data_ptr(), 1, _stream())
    torch.cuda.synchronize()
    R.assert_sentinel(buf, N, "reduce accumulate out")
    _same_bits(acc, R.reduce_emulated(s, prior), f"slk_reduce_slabs accumulate nslab={nslab}")
    if R.reduce_form(nslab) > 1:
        other = R.reduce_partials_prior_last(s, R.reduce_form(nslab), prior)
        assert R.differ_share(acc.cpu().numpy(), other) >= 0.25, "the prior is not where include/slk.h says"


@pytest.mark.parametrize("nslab", SLAB_COUNTS)
def test_optimizers_from_slabs_grad_order(gpu, nslab):
    """The `grad` output of slk_sgd_from_slabs, slk_sgdm_from_slabs, slk_adam_from_slabs and slk_adamw_from_slabs ==
    the emulation of the form for this slab count, bit for bit."""
    from splitcnn import _lib
    s = R.reduce_case(nslab, N, 3000 + nslab)
    want = R.reduce_emulated(s)
    sd = torch.from_numpy(s).to(gpu)
    step = _ints(gpu, 0)
    table = torch.tensor([0.01], dtype=torch.float32, device=gpu)
    st = _stream()

    def state():
        return [_padded(np.full(N, v, dtype=np.float32), gpu) for v in (0.5, 0.0, 0.0)]

    runs = {}
    (pb, p), _, _ = state()
    g = _nan_out(N, gpu)
    _lib.call("slk_sgd_from_slabs", p.data_ptr(), g.data_ptr(), sd.data_ptr(), nslab, N, 0.01, st)
    runs["slk_sgd_from_slabs"] = (g, pb)
    (pb, p), _, _ = state()
    g = _nan_out(N, gpu)
    _lib.call("slk_sgdm_from_slabs", p.data_ptr(), g.data_ptr(), None, sd.data_ptr(), nslab, N, table.data_ptr(), 1,
              step.data_ptr(), 0.0, 0.0, 0.0, 0, st)
    runs["slk_sgdm_from_slabs"] = (g, pb)
    (pb, p), (mb, m), (vb, v) = state()
    g = _nan_out(N, gpu)
    _lib.call("slk_adam_from_slabs", p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), sd.data_ptr(), nslab, N, 1e-3,
              0.9, 0.999, 1e-8, step.data_ptr(), st)
    runs["slk_adam_from_slabs"] = (g, pb, mb, vb)
    (pb, p), (mb, m), (vb, v) = state()
    g = _nan_out(N, gpu)
    _lib.call("slk_adamw_from_slabs", p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), sd.data_ptr(), nslab, N,
              table.data_ptr(), 1, step.data_ptr(), 0.9, 0.999, 1e-8, 0.0, 1, st)
    runs["slk_adamw_from_slabs"] = (g, pb, mb, vb)
    torch.cuda.synchronize()
    for name, bufs in runs.items():
        for b in bufs:
            R.assert_sentinel(b, N, name)
            assert torch.isfinite(b[:N]).all(), name
        _same_bits(bufs[0][:N], want, f"{name} nslab={nslab}")
        assert (bufs[1][:N] != 0.5).float().mean() > 0.9, f"{name}: the parameters were not updated"


def _host(ctype, vals):
    return ctypes.cast((ctype * 4)(*vals), ctypes.c_void_p)


def test_multi_launches_grad_order(gpu):
    """One slk_sgd_multi_from_slabs launch and one slk_adam_multi_from_slabs launch, each over three segments of
    different forms (9, 33 and 200 slabs): every segment's grad == its emulation bit for bit."""
    from splitcnn import _lib
    P = ctypes.c_void_p
    counts = [9, 33, 200]
    slabs = [R.reduce_case(k, N, 4000 + k) for k in counts]
    sd = [torch.from_numpy(s).to(gpu) for s in slabs]
    step = _ints(gpu, 0)
    for which in ("sgd", "adam"):
        ps = [_padded(np.full(N, 0.5, dtype=np.float32), gpu) for _ in counts]
        ms = [_padded(np.zeros(N, dtype=np.float32), gpu) for _ in counts]
        vs = [_padded(np.zeros(N, dtype=np.float32), gpu) for _ in counts]
        gs = [_nan_out(N, gpu) for _ in counts]
        ptr = lambda ts: _host(P, [t.data_ptr() for t in ts])  # noqa: E731
        args = [ptr([p for _, p in ps]), ptr(gs)]
        if which == "adam":
            args += [ptr([m for _, m in ms]), ptr([v for _, v in vs])]
        args += [ptr(sd), _host(ctypes.c_int, counts), _host(ctypes.c_int, [N] * 3), 3]
        if which == "sgd":
            _lib.call("slk_sgd_multi_from_slabs", *args, 0.01, None, 0, 0.0, None, 0, None, _stream())
        else:
            _lib.call("slk_adam_multi_from_slabs", *args, 1e-3, 0.9, 0.999, 1e-8, step.data_ptr(), _stream())
        torch.cuda.synchronize()
        for k, s, g, (pb, p) in zip(counts, slabs, gs, ps):
            R.assert_sentinel(g, N, f"{which} multi grad")
            R.assert_sentinel(pb, N, f"{which} multi param")
            _same_bits(g[:N], R.reduce_emulated(s), f"slk_{which}_multi_from_slabs segment nslab={k}")
            assert (p != 0.5).float().mean() > 0.9


# ----------------------------------------------------------------------------- plain SGD
@pytest.mark.parametrize("n", [1, 255, 257, 2048 * 256 + 77])
def test_sgd_is_the_fused_float32_expression(gpu, n):
    """slk_sgd: p <- fl(p - lr g), one rounding (see the module docstring); n above 2048 * 256 reaches the grid-stride
    loop (the grid is capped at 2048 blocks of 256)."""
    from splitcnn import _lib
    rng = np.random.default_rng(n)
    lr = np.float32(3 * 2.0 ** -8)
    p = (rng.uniform(2.0 ** -6, 2.0 ** -4, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32)
    g = (rng.uniform(0.25, 4.0, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32)
    exact = p.astype(np.float64) - np.float64(lr) * g.astype(np.float64)      # 30 bits at most: exact in float64
    want = exact.astype(np.float32)
    two = (p - (lr * g).astype(np.float32)).astype(np.float32)
    pb, pd = _padded(p, gpu)
    gd = torch.from_numpy(g).to(gpu)
    _lib.call("slk_sgd", pd.data_ptr(), gd.data_ptr(), n, float(lr), _stream())
    torch.cuda.synchronize()
    R.assert_sentinel(pb, n, "slk_sgd param")
    _same_bits(pd, want, f"slk_sgd n={n}")
    assert torch.equal(gd.cpu(), torch.from_numpy(g))
    if n > 1:
        assert R.differ_share(want, two) >= 0.2 and R.differ_share(pd.cpu().numpy(), two) >= 0.2


# ----------------------------------------------------------------------------- loss reductions
@pytest.mark.parametrize("n", [1, 63, 64, 255, 256, 257, 1000, 4099])
def test_loss_sum_and_log_exact(gpu, n):
    """Values = multiples of 2^-10 whose partial sums stay below 2^24 units (head_ref64.exact_values): any order is
    exact, so out == float64's sum times the power-of-two scale, bit for bit, from slk_loss_sum and slk_loss_log."""
    from splitcnn import _lib
    v = R.exact_values(n, 5000 + n)
    want = np.float32(v.sum() * 0.25)
    assert float(want) == v.sum() * 0.25
    vb, vd = _padded(v, gpu)
    out = _nan_out(1, gpu)
    _lib.call("slk_loss_sum", vd.data_ptr(), n, 0.25, out.data_ptr(), _stream())
    ring = _nan_out(2, gpu)
    ctr = _ints(gpu, 1, -1)
    _lib.call("slk_loss_log", vd.data_ptr(), n, 0.25, ring.data_ptr(), 2, ctr.data_ptr(), _stream())
    torch.cuda.synchronize()
    R.assert_sentinel(out, 1, "loss_sum out")
    R.assert_sentinel(ring, 2, "loss ring")
    _same_bits(out[:1], [want], f"slk_loss_sum n={n}")
    _same_bits(ring[1:2], [want], f"slk_loss_log n={n}")
    assert torch.isnan(ring[0]) and ctr.tolist() == [2, -1]


@pytest.mark.parametrize("via", ["slk_loss_log", "slk_sgd_multi_from_slabs"])
def test_loss_ring_wraps(gpu, via):
    """Capacity 3, counter starting at 2, three logs: they land in slots 2, 0, 1, the counter ends at 5 and a fourth
    slot behind the ring keeps its sentinel — through slk_loss_log and through slk_sgd_multi_from_slabs' loss block
    (with one reduce-only segment riding along)."""
    from splitcnn import _lib
    P = ctypes.c_void_p
    ring = torch.full((4,), NAN, dtype=torch.float32, device=gpu)
    ctr = _ints(gpu, 2, -1)
    vals = [R.exact_values(300, 6000 + i) for i in range(3)]
    s = R.reduce_case(9, N, 77)
    sd = torch.from_numpy(s).to(gpu)
    for v in vals:
        vd = torch.from_numpy(v).float().to(gpu)
        if via == "slk_loss_log":
            _lib.call("slk_loss_log", vd.data_ptr(), 300, 0.5, ring.data_ptr(), 3, ctr.data_ptr(), _stream())
        else:
            g = _nan_out(N, gpu)
            _lib.call("slk_sgd_multi_from_slabs", _host(P, [None]), _host(P, [g.data_ptr()]), _host(P, [sd.data_ptr()]),
                      _host(ctypes.c_int, [9]), _host(ctypes.c_int, [N]), 1, 0.0, vd.data_ptr(), 300, 0.5,
                      ring.data_ptr(), 3, ctr.data_ptr(), _stream())
            torch.cuda.synchronize()
            R.assert_sentinel(g, N, "reduce-only segment")
            _same_bits(g[:N], R.reduce_emulated(s), "reduce-only segment of the multi launch")
    torch.cuda.synchronize()
    want = [np.float32(v.sum() * 0.5) for v in vals]
    _same_bits(ring[:3], [want[1], want[2], want[0]], via)
    assert torch.isnan(ring[3]) and ctr.tolist() == [5, -1]


# ----------------------------------------------------------------------------- MNIST gather fallback
def test_mnist_batch_out_of_range_reads_image_zero(gpu):
    """Indices -1 and n_images set the flag and return image 0's pixels and label bit for bit; repeated indices are
    allowed; rows of valid indices equal the float32 ToTensor + Normalize expression."""
    from splitcnn import _lib
    rng = np.random.default_rng(3)
    n_images, mean, std = 37, 0.1307, 0.3081
    img = rng.integers(0, 256, (n_images, 784), dtype=np.uint8)
    lbl = rng.integers(0, 10, n_images, dtype=np.uint8)
    lbl[0] = 7
    idx = np.array([5, -1, 36, n_images, 5, 0, 36], dtype=np.int64)
    B = len(idx)
    di, dl, dx = (torch.from_numpy(a).to(gpu) for a in (img, lbl, idx))
    for flagged in (True, False):
        ids = dx if flagged else torch.from_numpy(np.array([5, 0, 36, 0, 5, 0, 36], dtype=np.int64)).to(gpu)
        x = torch.full((B + 1, 784), NAN, dtype=torch.float32, device=gpu)
        y = torch.full((B + 1,), -1, dtype=torch.int64, device=gpu)
        err = _ints(gpu, 0, -1)
        _lib.call("slk_mnist_batch", di.data_ptr(), dl.data_ptr(), n_images, ids.data_ptr(), B, mean, std, x.data_ptr(),
                  y.data_ptr(), err.data_ptr(), _stream())
        torch.cuda.synchronize()
        R.assert_sentinel(x, B * 784, "mnist x")
        R.assert_sentinel(y, B, "mnist y")
        assert err.tolist() == [1 if flagged else 0, -1]
        src = np.array([5, 0, 36, 0, 5, 0, 36])
        t = torch.from_numpy(img[src]).to(torch.float32).div(255).sub(np.float32(mean)).div(np.float32(std))
        assert torch.equal(x[:B].cpu().view(torch.int32), t.view(torch.int32))
        assert y[:B].tolist() == [int(v) for v in lbl[src]]
