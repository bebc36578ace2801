"""The DP-SGD kernels alone (csrc/slk_dpsgd.hip; include/slk.h, "DP-SGD on the K5 client") against float64 numpy.
Batch sizes: a workgroup owns one sample and a launch the whole batch, so 1, 2 (one more than a workgroup), 3, and 9, which
carries every special row. Every output is a NaN-filled slice of a larger NaN buffer whose tail must stay NaN.
Real step: a reference-side float32 emulation (every dW element one float32 chain over the pixels in steps of 32, float32
squares and sums) gives the yardstick |emulation - float64| / float64; the kernel may use 4 x that plus 2^-20, because its
lanes add up to 170 nonnegative float32 terms in another order than the emulation: a walk of sqrt(170) ~ 13 x 2^-24.
slk_dp_noise: from the documented errors (logf, sqrtf, cospif 1 ulp each; u1, u2, -2 log, 2 u2 exact) the radius carries
2^-23 / 2 from the logarithm and 2^-23 of its own, the cosine 2^-23, the product and the multiplication by std half an
ulp each: 3.5 x 2^-23 of |std z|; std's own roundings are reproduced in float32 on the reference side."""
import numpy as np
import pytest
import torch

from oracle import wide_step as W

pytestmark = pytest.mark.gpu
NOISE_RTOL = 3.5 * 2.0 ** -23
KINDS = ("random", "blocked", "first", "last", "conv1", "conv2", "conv3")
SHAPES = dict(x=(3, 32, 32), da1m=(64, 32, 32), a1=(64, 32, 32), dp2=(128, 16, 16), p2=(128, 16, 16), dcut=(256, 8, 8))
ORDER = ("x", "da1m", "a1", "dp2", "code2", "p2", "dcut", "code3")


def guarded(shape, gpu):
    n = int(np.prod(shape))
    buf = torch.full((n + 64,), float("nan"), device=gpu)
    return buf[n:], buf[:n].view(shape)


def sqnorm(args, gpu):
    from splitcnn import ops
    tail, work = guarded((args[0].shape[0], 6), gpu)
    ops.wide_grad_sqnorm(*args, work=work)
    assert torch.isnan(tail).all()
    return work


def coef(work, unit, C, gpu):
    from splitcnn import ops
    tail, stats = guarded((work.shape[0], 2), gpu)
    ops.dp_coef(work, unit, torch.full((1,), C, device=gpu), stats)
    assert torch.isnan(tail).all()
    return stats


def exact_rows(B, seed=0):
    """Logical NCHW operands of B samples (kind b % 7): small dyadic values, sparse enough that every accumulator
    (|operand| <= 2, K <= 1024: below 2^12 in steps of 1/4) and every sum of squares is exact in float32."""
    rng = np.random.default_rng(seed)
    rows = {k: [] for k in ORDER}
    for b in range(B):
        kind = KINDS[b % len(KINDS)]
        point = kind in ("first", "last")
        r = {k: np.where(rng.random(s) < ((0.5 if point else 0.05) if k in ("x", "a1", "p2") else 0.04),
                         rng.choice([0.5, -0.5, 1.0, -1.0, 2.0, -2.0], s), 0.0) for k, s in SHAPES.items()}
        r["code2"], r["code3"] = rng.integers(0, 5, SHAPES["dp2"]), rng.integers(0, 5, SHAPES["dcut"])
        if kind == "blocked":
            r["code2"][:], r["code3"][:], r["da1m"] = 4, 4, 0 * r["da1m"]
        for layer, g, c in (("conv1", "da1m", None), ("conv2", "dp2", "code2"), ("conv3", "dcut", "code3")):
            if point:   # one gradient element: pixel (0, 0) of channel 0, or the last pixel of the last channel
                i = 0 if kind == "first" else -1
                r[g] = 0 * r[g]
                r[g][i, i, i] = 2.0
                if c:
                    r[c][i, i, i] = 0 if kind == "first" else 3
            if kind in ("conv1", "conv2", "conv3") and kind != layer:
                r[g] = 0 * r[g]
        for k in ORDER:
            rows[k].append(r[k])
    return {k: np.stack(v) for k, v in rows.items()}


def layer_operands(r, b):
    """(input, unpooled dY) of conv1, conv2, conv3 for sample b, float64."""
    s = slice(b, b + 1)
    return ((W.bf16(r["x"][s]).astype(np.float64), r["da1m"][s]), (r["a1"][s], W.unpool(r["dp2"][s], r["code2"][s])),
            (r["p2"][s], W.unpool(r["dcut"][s], r["code3"][s])))


def ref_sumsq(r, b):
    return np.array([sum((g ** 2).sum() for g in W.conv3x3p1_wgrad(inp, dy)) for inp, dy in layer_operands(r, b)])


def device_args(r, gpu):
    from splitcnn.wide import nchw_to_c8
    t = {k: torch.from_numpy(np.ascontiguousarray(r[k], dtype=np.float32)) for k in ORDER}
    return [t["x"].to(gpu)] + [nchw_to_c8(t[k]).to(torch.uint8 if "code" in k else torch.bfloat16).to(gpu)
                               for k in ORDER[1:]]


def layer_sums(work):
    w = work.double().cpu().numpy()
    return np.stack([w[:, 0], w[:, 1], w[:, 2:].sum(axis=1)], axis=1)


@pytest.mark.parametrize("B", (1, 2, 3, 9))
def test_exact_class_bit_for_bit(gpu, B):
    r = exact_rows(B)
    want = np.stack([ref_sumsq(r, b) for b in range(B)])
    assert (want < 2 ** 20).all() and (want * 16 == np.round(want * 16)).all()   # exact in float32 in any order
    work = sqnorm(device_args(r, gpu), gpu)
    assert np.array_equal(layer_sums(work), want)
    if B == 9:   # blocked: norm 0, coef 1; the point rows reach every layer; each layer alone
        assert (want[1] == 0).all() and (want[2:4] > 0).all() and (np.argwhere(want[4:7] > 0) == [[0, 0], [1, 1], [2, 2]]).all()
        assert coef(work, 1.0, 1.0, gpu)[1].tolist() == [0.0, 1.0]


def test_nan_in_one_row_stays_there(gpu):
    args = device_args(exact_rows(3, seed=1), gpu)
    clean = sqnorm(args, gpu)
    args[6][1, 3, 2, 1, 5], args[7][1, 3, 2, 1, 5] = float("nan"), 0    # a routed element of row 1's dcut
    work = sqnorm(args, gpu)
    stats, cstats = coef(work, 3.0, 1.0, gpu), coef(clean, 3.0, 1.0, gpu)
    for got, ref in ((work, clean), (stats, cstats)):
        assert torch.equal(got[[0, 2]].view(torch.int32), ref[[0, 2]].view(torch.int32))
    assert torch.isnan(work[1, 2:]).any() and torch.isnan(stats[1, 0]) and stats[1, 1] == 1.0


def test_real_step_against_float64_and_the_wgrad_entries(gpu):
    """The seeded model's backward at B = 3 on the stage's own bf16 tensors; then every sample's norm from
    slk_wide_conv{1,2,3}_wgrad at B = 1 on that sample, slabs reduced in float64, under the same allowance."""
    from splitcnn.wide import SyntheticCIFAR, WideTrainer, _k, c8_to_nchw, client_backward_slab_shapes, init_wide_models
    tr = WideTrainer(*init_wide_models(seed=0), device=gpu, graph=False)
    x, y = (t.to(gpu) for t in SyntheticCIFAR(42).batch(3))
    c = tr.client
    dcut = tr.server.step_request(c.forward(x), y)[0].clone()
    c.backward_slabs(dcut)
    args = [x, c._da1m, c._a1, c._dp2, c._code2, c._p2, dcut, c._code3]
    got = layer_sums(sqnorm(args, gpu)).sum(axis=1)
    r = {k: (t if k == "x" else c8_to_nchw(t)).double().cpu().numpy() for k, t in zip(ORDER, args)}
    slabs = [guarded(s, gpu)[1] for s in client_backward_slab_shapes(1)]
    st = torch.cuda.current_stream(gpu).cuda_stream
    for b in range(3):
        want, emul = ref_sumsq(r, b).sum(), np.float32(0)
        for inp, dy in layer_operands(r, b):
            H = inp.shape[2]
            cols = np.vstack([W._cols(W._pad1(inp), H, H)[0].reshape(-1, H * H), np.ones((1, H * H))])   # + bias column
            dyf, acc = dy[0].reshape(dy.shape[1], -1), np.float32(0)
            for k in range(0, H * H, 32):
                acc = acc + (dyf[:, k:k + 32] @ cols[:, k:k + 32].T).astype(np.float32)
            emul += np.sum(acc * acc, dtype=np.float32)
        yard = abs(float(emul) - want) / want
        allow = 4 * yard + 2.0 ** -20
        p = [t[b:b + 1].contiguous().data_ptr() for t in args]
        _k("wide_conv3_wgrad", p[6], p[7], p[5], slabs[2].data_ptr(), 1, st)
        _k("wide_conv2_wgrad", p[3], p[4], p[2], slabs[1].data_ptr(), 1, st)
        _k("wide_conv1_wgrad", p[0], p[1], slabs[0].data_ptr(), 1, st)
        entries = sum((s.double().sum(axis=0) ** 2).sum().item() for s in slabs)
        print(f"sample {b}: sumsq {got[b]:.9g} float64 {want:.9g} wgrad entries {entries:.9g} yardstick {yard:.3g} "
              f"used {abs(got[b] - want) / want / allow:.3g} and {abs(got[b] - entries) / entries / allow:.3g}")
        assert want > 0 and yard <= 1e-4 and abs(got[b] - want) <= allow * want and abs(got[b] - entries) <= allow * entries


def test_dp_coef_against_the_formula(gpu):
    f = np.float32
    C, unit = f(1.5), f(3.0)
    edge = (C / unit) ** 2
    work = np.zeros((10, 6), dtype=f)
    work[:, 3] = [0.0, np.inf, np.nan, 1e-20, 1e30, np.nextafter(edge, f(0)), 0, np.nextafter(edge, f(9)),
                  edge * f(1 - 1e-5), edge * f(1 + 1e-5)]
    work[6] = edge / 6                                         # six equal partials: the float64 sum
    got = coef(torch.from_numpy(work).to(gpu), float(unit), float(C), gpu).cpu().numpy()
    with np.errstate(invalid="ignore"):
        norm = unit * np.sqrt(work.astype(np.float64).sum(axis=1).astype(f))
        q = C / (norm + f(1e-6))
        want = np.where(q < 1, q, f(1))
    assert np.array_equal(got[:, 0], norm, equal_nan=True) and np.array_equal(got[:, 1], want)
    assert want[0] == 1 and want[1] == 0 and want[2] == 1 and (want[5:] < 1).any() and (want[5:] == 1).any()


def test_dp_noise_against_the_host_twin(gpu):
    from splitcnn import ops
    from splitcnn.privacy import DPSGD
    f = np.float32
    n, i0, gs = 4099, 370816 - 4099, 0.25
    dp = DPSGD(2.0, 1.5, seed=3, device=gpu)
    ctr = torch.full((1,), 7, dtype=torch.int32, device=gpu)
    tail, out = guarded((n,), gpu)
    ops.dp_noise(out, i0, dp.sigma_value, dp.norm_value, gs, dp.seed, ctr)
    want = float(f(f(1.5) * f(2.0)) * f(gs)) * dp.noise_draws(i0 + np.arange(n), 7)
    assert (np.abs(out.double().cpu().numpy() - want) <= NOISE_RTOL * np.abs(want)).all() and torch.isnan(tail).all()
    tail, part = guarded((100,), gpu)
    ops.dp_noise(part, i0 + 1000, dp.sigma_value, dp.norm_value, gs, dp.seed, ctr)   # a slice with its own i0
    assert torch.equal(part.view(torch.int32), out[1000:1100].view(torch.int32)) and torch.isnan(tail).all()
    ops.dp_noise(part[:0], i0, dp.sigma_value, dp.norm_value, gs, dp.seed, ctr)      # n == 0: nothing is launched
    assert torch.equal(part.view(torch.int32), out[1000:1100].view(torch.int32))
    ops.dp_noise(part, i0, torch.zeros(1, device=gpu), dp.norm_value, gs, dp.seed, ctr)
    assert (part == 0).all()


def test_refusals_and_empty_batches(gpu):
    from splitcnn import _lib
    args = device_args(exact_rows(1), gpu)
    tail, work = guarded((1, 6), gpu)
    p = [t.data_ptr() for t in args] + [work.data_ptr()]
    one, w = torch.ones(1, device=gpu).data_ptr(), work.data_ptr()
    ctr = torch.zeros(1, dtype=torch.int32, device=gpu).data_ptr()
    for name, a in (("slk_wide_grad_sqnorm", (*p, 7, -1, None)), ("slk_wide_grad_sqnorm", (*p[:8], None, 7, 1, None)),
                    ("slk_wide_grad_sqnorm", (*p[:6], p[6] + 2, *p[7:], 7, 1, None)),
                    ("slk_dp_coef", (w, -1, 1.0, one, w, None)), ("slk_dp_coef", (w, 1, 1.0, one, w + 4, None)),
                    ("slk_dp_coef", (w, 1, 1.0, None, w, None)), ("slk_dp_noise", (w, -1, 0, one, one, 1.0, 0, ctr, None)),
                    ("slk_dp_noise", (w, 6, 0, None, one, 1.0, 0, ctr, None)),
                    ("slk_dp_noise", (w + 2, 6, 0, one, one, 1.0, 0, ctr, None))):
        with pytest.raises(_lib.SLKError, match="invalid argument"):
            _lib.call(name, *a)
    _lib.call("slk_wide_grad_sqnorm", *p, 7, 0, None)          # B == 0 / n == 0: nothing is launched
    _lib.call("slk_dp_coef", w, 0, 1.0, one, w, None)
    assert _lib.query("slk_wide_grad_sqnorm_work", 5) == 30 and torch.isnan(work).all() and torch.isnan(tail).all()
