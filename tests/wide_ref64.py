"""Test infrastructure: a float64 reference of the K5 conv stack (oracle/wide_step.py's conv3x3p1 / _dgrad / _wgrad /
relu_pool_code / unpool / bf16, restated in torch so it runs on the GPU), the K5 counterpart of tests/ref64.py.
Everything is float64 unfold / fold + matmul (no MIOpen, no reduced precision), chunked over the batch so that conv2
at B = 261 (the largest case of tests/test_wide_conv_gpu.py) fits in memory and finishes in seconds.
tests/test_wide_ref64_cpu.py pins every function to oracle/wide_step.py, which tests/test_wide_oracle.py pins to
torch autograd.

Also here: the seeded operand generators of the per-kernel tests and the precondition checks of their exact regime.

Exact regime. The kernels multiply bf16 operands exactly and accumulate in f32. If every operand is a small integer
and the sum of the absolute values of the products of every output stays below 2^24, every partial sum in ANY
summation order is an integer below 2^24, so the f32 accumulation is exact and the kernel's output must equal the
float64 reference's (rounded to bf16 where the kernel stores bf16) bit for bit: no tolerance, no excused element, no
waived tie. `assert_exact_operands` and `assert_abs_bound` assert those two preconditions on the reference side.
  wide variant   activations [0, 15] (signed where the sign matters), weights [-7, 7], biases [-31, 31], pooled
                 gradients [-15, 15]: outputs reach thousands, so the bf16 store rounds and meets exact halfway values;
  narrow variant activations nonzero with probability 0.15 in {1, 2, 3}, weights nonzero with probability 0.3 in
                 {-1, +1}, biases [-2, 2]: pre-pool values are small integers, so exact ties between window candidates
                 and maxima of exactly 0 occur by the thousand;
  wgrad variant  every operand magnitude <= 3, so that the batch sum stays below 2^24 (B = 515: 515 x 1024 x 9 = 4.7 M).
Real-valued regime: the distributions of tests/test_wide_gpu.py::test_pooled_gradient_routing_random_codes.

Operands are drawn on the CPU from a seeded generator (bit-identical everywhere, so what the CPU test establishes
about the generators holds for what the GPU tests feed the kernels) and moved to `device`.
"""
import numpy as np
import torch
import torch.nn.functional as F

CODE_NONE = 4
# layer -> (CI, CO, HW of the conv's input = of its pre-pool output)
LAYERS = {1: (3, 64, 32), 2: (64, 128, 32), 3: (128, 256, 16)}
W_SCALE = {1: 0.2, 2: 0.05, 3: 0.03}
CHUNK = 32


# ----------------------------------------------------------------------------- the reference
def bf16(x):
    """Round to the nearest bf16, ties to even (a bf16 tensor)."""
    return x.to(torch.float32).to(torch.bfloat16)


def bf16_f64(x):
    """bf16(x) as float64 values."""
    return bf16(x).double()


def conv_fwd(x, W, b=None, chunk=CHUNK):
    """conv2d(x, W, b, stride 1, padding 1) in float64: x [B,Ci,H,W], W [Co,Ci,3,3] -> [B,Co,H,W]."""
    B, Ci, H, Wd = x.shape
    Co = W.shape[0]
    Wm = W.double().reshape(Co, Ci * 9)
    out = torch.empty(B, Co, H, Wd, dtype=torch.float64, device=x.device)
    for s in range(0, B, chunk):
        cols = F.unfold(x[s:s + chunk].double(), 3, padding=1)          # b, Ci*9, H*W
        out[s:s + chunk] = torch.matmul(Wm, cols).reshape(-1, Co, H, Wd)
    if b is not None:
        out += b.double()[None, :, None, None]
    return out


def conv_dgrad(dy, W, chunk=CHUNK):
    """dx = full correlation of dy with W cropped to the input size: dy [B,Co,H,W] -> [B,Ci,H,W] float64."""
    B, Co, H, Wd = dy.shape
    Ci = W.shape[1]
    Wt = W.double().reshape(Co, Ci * 9).t().contiguous()
    out = torch.empty(B, Ci, H, Wd, dtype=torch.float64, device=dy.device)
    for s in range(0, B, chunk):
        cols = torch.matmul(Wt, dy[s:s + chunk].double().reshape(-1, Co, H * Wd))   # b, Ci*9, H*W
        out[s:s + chunk] = F.fold(cols, (H, Wd), 3, padding=1)
    return out


def conv_wgrad(x, dy, chunk=CHUNK):
    """dW [Co,Ci,3,3] = sum dy[b,o,h,w] * xpad[b,c,h+ky,w+kx] and db [Co] = sum dy, float64."""
    B, Ci, H, Wd = x.shape
    Co = dy.shape[1]
    dW = torch.zeros(Co, Ci * 9, dtype=torch.float64, device=x.device)
    for s in range(0, B, chunk):
        cols = F.unfold(x[s:s + chunk].double(), 3, padding=1)          # b, Ci*9, H*W
        d = dy[s:s + chunk].double().reshape(-1, Co, H * Wd)
        dW += torch.matmul(d, cols.transpose(1, 2)).sum(0)
    return dW.reshape(Co, Ci, 3, 3), dy.double().sum(dim=(0, 2, 3))


def windows(c):
    """[B,C,H,W] -> the 2x2 windows [B,C,H/2,W/2,4], row-major inside the window."""
    B, C, H, Wd = c.shape
    return c.reshape(B, C, H // 2, 2, Wd // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(B, C, H // 2, Wd // 2, 4)


def relu_pool_code(c):
    """maxpool2(relu(c)) and its routing code: strict > scan (the first maximum wins); code 4 and pooled value +0
    where the maximum is <= 0. Returns (pooled float64 [B,C,H/2,W/2], code int64)."""
    win = windows(c)
    win = torch.where(win > 0, win, torch.zeros_like(win))
    best = win[..., 0].clone()
    idx = torch.zeros(best.shape, dtype=torch.long, device=c.device)
    for q in range(1, 4):
        better = win[..., q] > best
        best = torch.where(better, win[..., q], best)
        idx = torch.where(better, torch.full_like(idx, q), idx)
    pos = best > 0
    return torch.where(pos, best, torch.zeros_like(best)), torch.where(pos, idx, torch.full_like(idx, CODE_NONE))


def pooled_at(c, code):
    """relu(c) at window position `code` (0 where code == 4): the pooled value a given routing selects."""
    win = windows(c).clamp_min(0.0)
    v = win.gather(-1, code.long().clamp_max(3)[..., None])[..., 0]
    return torch.where(code.long() < 4, v, torch.zeros_like(v))


def unpool(pooled, code):
    """max-pool backward: pooled [B,C,h,w] at window position code (0..3), nothing where code == 4: [B,C,2h,2w]."""
    B, C, h, w = pooled.shape
    code = code.long()
    d = torch.zeros(B, C, h, w, 4, dtype=pooled.dtype, device=pooled.device)
    for q in range(4):
        d[..., q] = torch.where(code == q, pooled, torch.zeros_like(pooled))
    return d.reshape(B, C, h, w, 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(B, C, 2 * h, 2 * w)


def pos_zero(x):
    """-0 -> +0. A float64 GEMM may return either zero; the kernels' sums start at +0 and +0 + (-0) = +0, so a zero
    result is +0 there. Bit comparisons use this form of the reference."""
    return x + 0.0


# ----------------------------------------------------------------------------- preconditions of the exact regime
def assert_exact_operands(*tensors):
    """Every operand equals its own bf16 rounding (and is finite)."""
    for t in tensors:
        t = t.double()
        assert torch.isfinite(t).all()
        assert torch.equal(bf16_f64(t), t), "an operand of an exact test is not representable in bf16"


def assert_abs_bound(abs_sum):
    """abs_sum = the same contraction on absolute values (with |bias|): below 2^24 for every output, so every
    partial sum of the kernel's f32 accumulation is an exact integer."""
    m = float(abs_sum.max())
    assert m < 2.0 ** 24, f"absolute-value sum {m} reaches 2^24: the f32 accumulation is not exact"


def halfway_share(v):
    """Share of the f32 values v that are an exact halfway case of bf16 rounding (low 16 bits 0x8000)."""
    bits = v.to(torch.float32).contiguous().view(torch.int32)
    return float(((bits & 0xFFFF) == 0x8000).double().mean())


# ----------------------------------------------------------------------------- generators
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _ints(g, shape, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=g).double()


def _narrow_act(g, shape):
    nz = torch.rand(shape, generator=g) < 0.15
    return torch.where(nz, _ints(g, shape, 1, 3), torch.zeros(shape, dtype=torch.float64))


def _narrow_w(g, shape):
    nz = torch.rand(shape, generator=g) < 0.3
    sign = _ints(g, shape, 0, 1) * 2 - 1
    return torch.where(nz, sign, torch.zeros(shape, dtype=torch.float64))


def codes(g, shape):
    return torch.randint(0, 5, shape, generator=g)


def fwd_case(layer, B, regime, seed, device="cpu"):
    """Operands of conv<layer>'s forward: (inp [B,CI,HW,HW], W [CO,CI,3,3], b [CO]) float64. regime: "wide" / "narrow"
    (exact) or "real". conv1's input x is signed; the other layers' inputs are activations (>= 0). In the real
    regime inp is already bf16-representable for layers 2 and 3 (a stored activation) and a raw f32 x for layer 1;
    W and b are raw f32 values (the kernels round W, and x, to bf16 themselves; the bias stays f32)."""
    CI, CO, HW = LAYERS[layer]
    g = _gen(seed)
    ishape, wshape = (B, CI, HW, HW), (CO, CI, 3, 3)
    if regime == "wide":
        inp = _ints(g, ishape, -15, 15) if layer == 1 else _ints(g, ishape, 0, 15)
        W, b = _ints(g, wshape, -7, 7), _ints(g, (CO,), -31, 31)
    elif regime == "narrow":
        inp = _narrow_act(g, ishape)
        if layer == 1:
            inp = inp * (_ints(g, ishape, 0, 1) * 2 - 1)
        W, b = _narrow_w(g, wshape), _ints(g, (CO,), -2, 2)
    else:
        assert regime == "real"
        inp = torch.randn(ishape, generator=g)
        inp = inp.double() if layer == 1 else bf16_f64(inp.abs())
        W = (torch.randn(wshape, generator=g) * W_SCALE[layer]).double()
        b = (torch.randn(CO, generator=g) * 0.1).double()
    return tuple(t.to(device) for t in (inp, W, b))


def dgrad_case(layer, B, regime, seed, device="cpu"):
    """Operands of conv<layer>'s input gradient (layer 3: dcut -> dp2; layer 2: dp2 -> da1m): (dpooled [B,CO,HW/2,HW/2]
    float64, code int64, W [CO,CI,3,3] float64, relu [B,CI,HW,HW] bool or None). regime "wide" (exact) or "real".
    relu (layer 2 only) holds random bits, independent of any a1; samples 0 and 1 (where B allows) are all ones and
    all zeros."""
    CI, CO, HW = LAYERS[layer]
    g = _gen(seed)
    pshape = (B, CO, HW // 2, HW // 2)
    if regime == "wide":
        dp, W = _ints(g, pshape, -15, 15), _ints(g, (CO, CI, 3, 3), -7, 7)
    else:
        assert regime == "real"
        dp = bf16_f64(torch.randn(pshape, generator=g) * 1e-2)
        W = (torch.randn((CO, CI, 3, 3), generator=g) * W_SCALE[layer]).double()
    code = codes(g, pshape)
    relu = None
    if layer == 2:
        relu = torch.rand((B, CI, HW, HW), generator=g) < 0.5
        relu[0] = True
        if B > 1:
            relu[1] = False
    return tuple(t.to(device) if t is not None else None for t in (dp, code, W, relu))


def wgrad_case(layer, B, regime, seed, device="cpu"):
    """Operands of conv<layer>'s weight gradient. Layers 2, 3: (inp [B,CI,HW,HW], dpooled [B,CO,HW/2,HW/2], code);
    layer 1: (x [B,3,32,32], da1m [B,64,32,32], None). regime "exact" (every magnitude <= 3) or "real"."""
    CI, CO, HW = LAYERS[layer]
    g = _gen(seed)
    ishape = (B, CI, HW, HW)
    dshape = (B, CO, HW, HW) if layer == 1 else (B, CO, HW // 2, HW // 2)
    if regime == "exact":
        inp = _ints(g, ishape, -3, 3) if layer == 1 else _ints(g, ishape, 0, 3)
        d = _ints(g, dshape, -3, 3)
    else:
        assert regime == "real"
        inp = torch.randn(ishape, generator=g)
        inp = inp.double() if layer == 1 else bf16_f64(inp.abs())
        d = bf16_f64(torch.randn(dshape, generator=g) * 1e-2)
    code = None if layer == 1 else codes(g, dshape)
    return tuple(t.to(device) if t is not None else None for t in (inp, d, code))


# ----------------------------------------------------------------------------- the project's bf16 bars (numpy)
def bf16_close(got, want, frac=1e-3, acc_floor=4e-6):
    """One bf16 ulp where the rounding flipped, on top of the f32 accumulation noise floor
    (acc_floor x the tensor's max: f32 sums of O(1) terms carry absolute, not relative, error)."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (got.shape, want.shape)
    bad = got != want
    if not bad.any():
        return
    d = np.abs(got - want)[bad]
    lim = 2.0 ** -7 * np.abs(want)[bad] + acc_floor * np.abs(want).max() + 1e-30
    assert (d <= lim * 1.0001).all(), f"max rel diff {np.max(d / np.maximum(np.abs(want[bad]), 1e-30)):.3g}"
    assert bad.mean() <= frac, f"{bad.mean():.2e} of elements differ by one bf16 ulp"


def codes_close(c_pre, code_got, code_want, rtol=1e-5):
    """Routing differences must be numerical ties of the f32/f64 pre-pool values c_pre."""
    diff = code_got != code_want
    if not diff.any():
        return
    B, C, H, Wd = c_pre.shape
    win = c_pre.reshape(B, C, H // 2, 2, Wd // 2, 2).transpose(0, 1, 2, 4, 3, 5).reshape(B, C, H // 2, Wd // 2, 4)
    win = np.maximum(win, 0.0)[diff]
    scale = max(np.abs(c_pre).max(), 1e-30)

    def val(code):
        return np.where(code < 4, np.take_along_axis(win, np.minimum(code, 3)[:, None], axis=1)[:, 0], 0.0)
    va, vb = val(code_got[diff]), val(code_want[diff])
    assert (np.abs(va - vb) <= rtol * scale).all(), f"{diff.sum()} non-tie routing differences"
    assert diff.mean() < 1e-3


def grad_close(got, want, rtol=1e-5):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    err = np.abs(got - want).max() / max(np.abs(want).max(), 1e-30)
    assert err <= rtol, err
