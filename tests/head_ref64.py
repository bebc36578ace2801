"""Float64 references, float32 reduction emulations and seeded operand generators for the kernels AROUND the
convolutions: the K2 client (csrc/slk_client.hip), the K2 fc head and its weight gradient (csrc/slk_server.hip), the
K5 server head (csrc/slk_wide_head.hip), the cross-entropy copies, the fixed-order slab reductions and the loss
reductions (csrc/slk_optim.hip). Test infrastructure only (tests/test_head_ref64_cpu.py pins it on the CPU;
tests/test_client_fc_exact_gpu.py, test_xent_edges_gpu.py, test_reduce_order_gpu.py and test_wide_head_exact_gpu.py
use it on the GPU).

Exact regime: integer-valued operands sized so that every partial sum of absolute values stays below 2^24. An f32
accumulation is then exact in ANY order, so a kernel's output must equal the float64 result bit for bit; each generator
states its bound.

The conv / fc references are plain torch float64 expressions (shifted sums and matmuls), device-agnostic; the
cross-entropy and the reduction emulations are numpy. A reference takes a `mutate` name where a test needs a subtly
wrong version of it (the mutation tests assert that the GPU result differs from the mutated reference).
"""
from __future__ import annotations

import math

import numpy as np
import torch

from oracle import wide_step as WO

F64 = torch.float64
NCLS = 10
LN10 = math.log(10.0)


def pos_zero(t):
    """-0.0 -> +0.0 (a kernel's `s > 0 ? s : 0` and zero-initialised accumulators give +0)."""
    return t + 0.0


def f32_bits(t):
    return t.contiguous().view(torch.int32)


def assert_bits_f32(got, want64, what):
    """got (f32) == want64 (float64, exactly representable) bit for bit: NaN (unwritten) or -0.0 fail."""
    want = pos_zero(want64).to(torch.float32)
    assert torch.equal(want.double(), pos_zero(want64)), f"{what}: the reference is not exact in f32"
    bad = f32_bits(got) != f32_bits(want)
    n = int(bad.sum())
    if n:
        i = tuple(bad.nonzero()[0].tolist())
        raise AssertionError(f"{what}: {n} of {bad.numel()} values differ from float64; first at {i}: got "
                             f"{got[i].item()!r}, want {want[i].item()!r}")


def assert_sentinel(buf, used, what):
    """buf is a flat over-allocated output: everything past `used` elements still holds its fill pattern
    (NaN for floats, all-ones bytes for integers)."""
    tail = buf.reshape(-1)[used:]
    assert tail.numel() > 0, f"{what}: no sentinel allocated"
    if tail.dtype.is_floating_point:
        ok = torch.isnan(tail.float()).all()
    else:
        ok = (tail == -1).all() if tail.dtype != torch.uint8 else (tail == 0xFF).all()
    assert bool(ok), f"{what}: a write landed past the last row"


# ============================================================================ K2 client: conv1 + ReLU, its wgrad
def _shifts(x):
    """x [B,1,28,28] -> the 9 tap operands [9][B,26,26], tap k = (ky, kx) row-major: x[b, y + ky, x + kx]."""
    return [x[:, 0, k // 3:k // 3 + 26, k % 3:k % 3 + 26] for k in range(9)]


def conv1_pre(x, W1, b1):
    """conv2d(x, W1, b1), stride 1, no padding, float64: [B,32,26,26]."""
    x, W1, b1 = x.to(F64), W1.to(F64).reshape(32, 9), b1.to(F64)
    out = b1[None, :, None, None].expand(x.shape[0], 32, 26, 26).clone()
    for k, xs in enumerate(_shifts(x)):
        out += W1[None, :, k, None, None] * xs[:, None]
    return out


def conv1_relu(x, W1, b1):
    """act = relu(conv1(x)): exactly +0.0 wherever the pre-activation is <= 0."""
    pre = conv1_pre(x, W1, b1)
    return torch.where(pre > 0, pre, torch.zeros_like(pre))


def conv1_abs_bound(x, W1, b1):
    """sum_k |x_k W_k| + |b| per output (the exact regime needs it < 2^24; the real regime's error bound scales by it)."""
    return conv1_pre(x.abs(), W1.abs(), b1.abs())


def conv1_cut_bound_f32(x, W1, b1):
    """include/slk.h's act_amax: max_c fma(sum_k |W1[c][k]| (taps in order, f32), max|x[b]|, max(b1[c], 0)) in f32.
    Computed in float64 from f32 operands; the callers use integer operands, where every step is exact."""
    xm = x.to(torch.float32).abs().reshape(x.shape[0], -1).max(dim=1).values.double()
    ws = torch.zeros(32, dtype=torch.float32, device=x.device)
    for k in range(9):
        ws = ws + W1.to(torch.float32).reshape(32, 9)[:, k].abs()
    v = ws.double()[None, :] * xm[:, None] + b1.to(F64).clamp_min(0.0)[None, :]
    return v.to(torch.float32).max(dim=1).values


def conv1_ranges(B):
    """Sample ranges of slk_conv1_wgrad: G = min(B, 128) ranges, range grp = [grp * B // G, (grp + 1) * B // G)."""
    G = min(B, 128)
    return [(g * B // G, (g + 1) * B // G) for g in range(G)]


def conv1_wgrad_per_sample(x, act, g, mutate=None):
    """Per-sample client gradient [B, 320] = [dW1 c*9+tap (288) | db1 (32)]: the cut gradient g masked by act > 0
    (relu backward: 0 at act == 0), then dW1[c][k] = sum_pix gm[c][pix] x[pix + tap k], db1[c] = sum_pix gm[c][pix].
    mutate: 'ge' (mask act >= 0), 'drop_last_pair' (the last two pixels of every plane ignored), 'shift_tap' (tap 4
    reads tap 5's pixels)."""
    x, act, g = x.to(F64), act.to(F64), g.to(F64)
    keep = act >= 0 if mutate == "ge" else act > 0
    gm = torch.where(keep, g, torch.zeros_like(g))
    if mutate == "drop_last_pair":
        gm = gm.clone()
        gm[:, :, 25, 24:] = 0.0
    sh = _shifts(x)
    if mutate == "shift_tap":
        sh[4] = sh[5]
    dW = torch.stack([(gm * xs[:, None]).sum(dim=(2, 3)) for xs in sh], dim=2)      # [B,32,9]
    return torch.cat([dW.reshape(x.shape[0], 288), gm.sum(dim=(2, 3))], dim=1)


def conv1_wgrad_slabs(x, act, g, mutate=None):
    """[G, 320]: slab grp = the float64 sum of the per-sample gradients of its own sample range.
    mutate 'drop_last_sample': every range of more than one sample loses its last sample."""
    per = conv1_wgrad_per_sample(x, act, g, mutate)
    rows = []
    for lo, hi in conv1_ranges(x.shape[0]):
        if mutate == "drop_last_sample" and hi - lo > 1:
            hi -= 1
        rows.append(per[lo:hi].sum(dim=0))
    return torch.stack(rows)


def _ints(gen, lo, hi, shape):
    return torch.randint(lo, hi + 1, shape, generator=gen).to(F64)


def conv1_int_case(B, seed, device="cpu"):
    """Integer x in [-4, 4], W1 in [-3, 3], b1 in [-3, 3]: |pre-activation| <= 9 * 12 + 3 = 111 < 2^24, and exact-zero
    pre-activations occur (a few per cent: the `>` / `>=` boundary)."""
    gen = torch.Generator().manual_seed(seed)
    x = _ints(gen, -4, 4, (B, 1, 28, 28))
    W1 = _ints(gen, -3, 3, (32, 1, 3, 3))
    b1 = _ints(gen, -3, 3, (32,))
    return x.to(device), W1.to(device), b1.to(device)


def conv1_real_case(B, seed, device="cpu"):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn((B, 1, 28, 28), generator=gen).float().double()
    W1 = (torch.randn((32, 1, 3, 3), generator=gen) * 0.3).float().double()
    b1 = (torch.randn((32,), generator=gen) * 0.1).float().double()
    return x.to(device), W1.to(device), b1.to(device)


def cut_grad_int(B, seed, device="cpu"):
    """Integer cut gradient in [-4, 4]: with |x| <= 4 a slab entry is at most 16 * 676 pixels * 3 samples per range
    (B <= 300 -> ranges of at most 3) = 32,448 < 2^24."""
    gen = torch.Generator().manual_seed(seed)
    return _ints(gen, -4, 4, (B, 32, 26, 26)).to(device)


# ============================================================================ K2 fc head
P_SAMPLE = 9216


def fc_fwd(pooled, W3, b3):
    return pooled.to(F64) @ W3.to(F64).T + b3.to(F64)


def fc_dgrad(dlogits, W3):
    return dlogits.to(F64) @ W3.to(F64)


def fc_wgrad_per(B):
    """Samples per slice of slk_fc_wgrad: ceil(B / min(64, ceil(B / 64)))."""
    ns = max(1, min(64, -(-B // 64)))
    return -(-B // ns)


def fc_wgrad_nslab(B):
    return -(-B // fc_wgrad_per(B))


def fc_wgrad_slabs(dlogits, pooled, mutate=None):
    """[nslab, 92170] = [dW3 (10 x 9216) | db3 (10)] per slice of fc_wgrad_per(B) samples, float64.
    mutate: 'transpose_class' (the class index of dW3 rotated by one), 'drop_last_sample' (slices of more than one sample lose
    their last one)."""
    dl, p = dlogits.to(F64), pooled.to(F64)
    B, per = dl.shape[0], fc_wgrad_per(dl.shape[0])
    rows = []
    for lo in range(0, B, per):
        hi = min(B, lo + per)
        if mutate == "drop_last_sample" and hi - lo > 1:
            hi -= 1
        dW = dl[lo:hi].T @ p[lo:hi]
        if mutate == "transpose_class":
            dW = dW.roll(1, dims=0)
        rows.append(torch.cat([dW.reshape(-1), dl[lo:hi].sum(dim=0)]))
    return torch.stack(rows)


def fc_int_case(B, seed, device="cpu"):
    """Integer pooled in [0, 3], W3 in [-2, 2], b3 in [-3, 3]: |logit| <= 9216 * 6 + 3 < 2^24."""
    gen = torch.Generator().manual_seed(seed)
    pooled = _ints(gen, 0, 3, (B, P_SAMPLE))
    W3 = _ints(gen, -2, 2, (NCLS, P_SAMPLE))
    b3 = _ints(gen, -3, 3, (NCLS,))
    return pooled.to(device), W3.to(device), b3.to(device)


def dlogits_int(B, seed, device="cpu"):
    """Integer dlogits in [-3, 3]: |dpooled| <= 10 * 3 * 2 = 60; a weight-gradient slab entry <= 3 * 3 * 64 samples
    = 576 (K2, pooled <= 3) or 3 * 6 * 64 = 1,152 (K5, dropped cut <= 6): all < 2^24."""
    gen = torch.Generator().manual_seed(seed)
    return _ints(gen, -3, 3, (B, NCLS)).to(device)


def onehot_features(B):
    """The feature k_s of sample s in the one-hot construction: features 0 and 9215, the first and last feature of
    waves 0, 1, 3, 7 (wave w owns 1152 w ..), and the first and last feature of 64-feature chunks inside a wave."""
    ks = [0, 9215]
    for w in (0, 1, 3, 7):
        ks += [1152 * w, 1152 * w + 1151]
    for c in (0, 1, 17, 18, 19, 71, 143):
        ks += [64 * c, 64 * c + 63]
    ks += [15, 16, 3, 4, 4607, 4608]
    ks = list(dict.fromkeys(ks))
    ks += [k for k in range(100, P_SAMPLE, 263) if k not in ks]       # distinct fillers, every wave
    assert B <= len(ks)
    return ks[:B]


def onehot_rows(B, F, ks, device="cpu"):
    p = torch.zeros((B, F), dtype=F64, device=device)
    p[torch.arange(B), torch.tensor(ks)] = 1.0
    return p


# ============================================================================ cross-entropy
def xent64(z, y, grad_scale=1.0):
    """numpy float64, max-subtracted: (loss_i [B], dlogits [B,10], softmax p [B,10]). -inf logits are allowed off the
    label."""
    z = np.asarray(z, dtype=np.float64)
    y = np.asarray(y, dtype=np.int64)
    B = z.shape[0]
    m = z.max(axis=1, keepdims=True)
    with np.errstate(divide="ignore"):
        lse = m + np.log(np.exp(z - m).sum(axis=1, keepdims=True))
        logp = z - lse
    p = np.exp(logp)
    onehot = np.zeros_like(z)
    onehot[np.arange(B), y] = 1.0
    return -logp[np.arange(B), y], (p - onehot) * grad_scale, p


def xent32_naive(z, y):
    """float32, WITHOUT the max-subtraction: what a wrong kernel copy would compute."""
    z = np.asarray(z, dtype=np.float32)
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        lse = np.log(np.exp(z).sum(axis=1, dtype=np.float32))
        return (lse - z[np.arange(z.shape[0]), y]).astype(np.float32)


def _finite_absmax(z):
    a = np.abs(np.asarray(z, dtype=np.float64))
    return np.where(np.isfinite(a), a, 0.0).max(axis=1)


def loss_bound(z, loss64):
    """|loss - loss64| <= 2^-23 (max|z| + ln 10) + (2e-6 |loss64| + 1e-6): the two f32 roundings of m + log(se) and
    lse - z_y (each at most 2^-24 of a value below max|z| + ln 10), plus the project's loss bar."""
    return 2.0 ** -23 * (_finite_absmax(z) + LN10) + 2e-6 * np.abs(loss64) + 1e-6


def grad_bound(z, p64, grad_scale=1.0):
    """|dlogits - d64| <= grad_scale (p64 2^-22 (max|z| + ln 10) + 2e-7): the exponent's argument z - lse carries the
    roundings of loss_bound (a relative error of the exponential), plus the project's gradient bar."""
    return grad_scale * (p64 * 2.0 ** -22 * (_finite_absmax(z) + LN10)[:, None] + 2e-7)


def gradsum_bound(z, grad_scale=1.0):
    """|sum_j dlogits_j| <= grad_scale (2^-22 (max|z| + ln 10) + 10 * 2^-23).
    The second term is ten f32 roundings of values below 1. The first is grad_bound's relative term summed over the
    row (sum_j p64_j = 1): every p_j = exp(z_j - lse) of a row shares the rounding of lse = fl(m + log se), an absolute
    error up to 2^-24 (max|z| + ln 10) of the exponent, so the whole row is scaled by exp(that error) and its sum
    misses 1 by as much. (At max|z| = 1e4, lse's ulp is 2^-10: the row sums to 1 +- 4.9e-4, not 1 +- 1e-6.)"""
    return grad_scale * (2.0 ** -22 * (_finite_absmax(z) + LN10) + 10 * 2.0 ** -23)


def xent_rows(finite_only=True):
    """The crafted logit rows as (name, z [10]); every row is paired with labels at its maximum, its minimum and in
    between by xent_cases. `naive_breaks` names the rows on which xent32_naive is non-finite or wrong."""
    dn = np.arange(NCLS, dtype=np.float64)
    small = np.array([0.3, -1.2, 0.7, 0.1, -0.4, 1.1, -0.9, 0.5, 0.0, -0.2])
    one30, one200 = small.copy(), small.copy()
    one30[6] += 30.0
    one200[2] += 200.0
    big = np.full(NCLS, -1e30)
    big[3] = 1e30
    rows = [("zeros", np.zeros(NCLS)), ("equal_1e4", np.full(NCLS, 1e4)), ("down_from_100", 100.0 - dn),
            ("down_from_-100", -100.0 - dn), ("one_30_above", one30), ("one_200_above", one200),
            ("1e4_unit_gaps", 1e4 - dn[::-1]), ("-1e4_unit_gaps", -1e4 - dn), ("pm_1e30", big)]
    if not finite_only:
        a = small.copy()
        a[[1, 4, 8]] = -np.inf
        b = 100.0 - dn
        b[[0, 9]] = -np.inf
        rows += [("neg_inf_some", a), ("neg_inf_ends", b)]
    return rows


NAIVE_BREAKS = ("equal_1e4", "down_from_100", "down_from_-100", "one_200_above", "1e4_unit_gaps", "-1e4_unit_gaps",
                "pm_1e30")


def xent_cases(finite_only=True):
    """(names, z [n,10] float32-exact float64, y [n]): each row with the label at its (first) maximum, at its (last)
    finite minimum and at a class in between (the median finite class)."""
    names, zs, ys = [], [], []
    for name, z in xent_rows(finite_only):
        z = z.astype(np.float32).astype(np.float64)
        fin = np.where(np.isfinite(z))[0]
        order = fin[np.argsort(z[fin], kind="stable")]
        for tag, y in (("max", int(np.argmax(z))), ("min", int(order[0])), ("mid", int(order[len(order) // 2]))):
            names.append(f"{name}/{tag}")
            zs.append(z)
            ys.append(y)
    return names, np.stack(zs), np.asarray(ys, dtype=np.int64)


def xent_batch(B, shift, finite_only=True):
    """B samples cycling through xent_cases from case `shift` (different shifts put different cases into the first and
    last slot of a 16-sample workgroup and into the ragged last one)."""
    names, z, y = xent_cases(finite_only)
    idx = (np.arange(B) + shift) % len(names)
    return [names[i] for i in idx], z[idx], y[idx]


# ============================================================================ slab reductions, float32 emulation
def reduce_ascending(slabs, prior=None):
    """nslab <= 16: g = ((0 + s0) + s1) + ...; out = prior + g."""
    s = np.asarray(slabs, dtype=np.float32)
    g = np.zeros(s.shape[1], dtype=np.float32)
    for k in range(s.shape[0]):
        g = g + s[k]
    return g if prior is None else np.asarray(prior, dtype=np.float32) + g


def reduce_partials(slabs, nparts, prior=None):
    """nparts strided partials: part w = ((0 + s_w) + s_{w+nparts}) + ...; out = (((prior or 0) + part 0) + part 1)
    + ... — the prior is the START of the chain, not added to the finished sum."""
    s = np.asarray(slabs, dtype=np.float32)
    parts = []
    for w in range(nparts):
        g = np.zeros(s.shape[1], dtype=np.float32)
        for k in range(w, s.shape[0], nparts):
            g = g + s[k]
        parts.append(g)
    t = np.zeros(s.shape[1], dtype=np.float32) if prior is None else np.asarray(prior, dtype=np.float32).copy()
    for g in parts:
        t = t + g
    return t


def reduce_partials_prior_last(slabs, nparts, prior):
    """include/slk.h's earlier wording, out = prior + (sum of the partials): NOT what the kernels do."""
    return np.asarray(prior, dtype=np.float32) + reduce_partials(slabs, nparts)


def reduce_form(nslab):
    return 1 if nslab <= 16 else (4 if nslab <= 64 else 16)


def reduce_emulated(slabs, prior=None):
    """The documented form for this slab count (include/slk.h, slk_reduce_slabs)."""
    f = reduce_form(np.asarray(slabs).shape[0])
    return reduce_ascending(slabs, prior) if f == 1 else reduce_partials(slabs, f, prior)


def reduce_case(nslab, n, seed):
    """randn * 10**U(-3, 3): magnitudes spread over six decades, so every summation order rounds differently."""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((nslab, n)) * 10.0 ** rng.uniform(-3, 3, (nslab, n))).astype(np.float32)


def differ_share(a, b):
    return float((np.asarray(a, dtype=np.float32).view(np.int32) != np.asarray(b, dtype=np.float32).view(np.int32)).mean())


def exact_values(n, seed):
    """Multiples of 2^-10 in [0, 8) whose every partial sum, in units of 2^-10, stays below 2^24 (so any summation
    order is exact in f32): n <= 2048 values below 8 sum to less than 2048 * 2^13 = 2^24; above that the values are
    drawn below 2 (n <= 8192 of them sum to less than 2^24)."""
    assert n <= 8192
    rng = np.random.default_rng(seed)
    top = 8 * 1024 if n <= 2048 else 2 * 1024
    return rng.integers(0, top, n).astype(np.float64) / 1024.0


# ============================================================================ K5 server head
CUT_F = WO.CUT_F


def c8_of_flat(flat):
    """[B, 16384] in torch flatten order (c*64 + pix) -> the C8 order [B, 16384]: index (plane*64 + pix)*8 + k holds
    feature (plane*8 + k)*64 + pix."""
    B = flat.shape[0]
    return flat.reshape(B, 32, 8, 64).permute(0, 1, 3, 2).reshape(B, CUT_F).contiguous()


def flat_of_c8(c8):
    B = c8.shape[0]
    return c8.reshape(B, 32, 64, 8).permute(0, 1, 3, 2).reshape(B, CUT_F).contiguous()


def keep_mask(seed, step, B, p, b0=0):
    """oracle.wide_step.dropout_keep as a numpy bool [B, 16384] (torch flatten order)."""
    return WO.dropout_keep(seed, step, B, p=p, b0=b0)


def keep_bytes(keep):
    """The `work` bytes of slk_wide_head: [B, 2048] uint8, byte (plane*64 + pix), bit k = keep of feature
    (plane*8 + k)*64 + pix."""
    B = keep.shape[0]
    k = keep.reshape(B, 32, 8, 64).transpose(0, 1, 3, 2).reshape(B, 2048, 8).astype(np.uint8)
    return (k << np.arange(8, dtype=np.uint8)[None, None, :]).sum(axis=2).astype(np.uint8)


def head_fwd(cut, Wf, bf, keep, keep_scale):
    """logits = (cut * keep * keep_scale) @ Wf^T + bf, float64. cut [B,16384] (flatten order), keep bool tensor."""
    d = cut.to(F64) * keep.to(F64) * keep_scale
    return d @ Wf.to(F64).T + bf.to(F64)


def head_bwd(cut, Wf, dlogits, keep, keep_scale, mutate=None):
    """(dcut [B,16384] float64 before the bf16 store, slabs [ceil(B/64), 163850] = [dWf | dbf] per 64-sample group).
    mutate: 'drop_last_sample' (groups of more than one sample lose their last), 'scale_once' (keep_scale applied to
    the forward's dropped cut only, not to the cut gradient)."""
    cut, Wf, dl, k = cut.to(F64), Wf.to(F64), dlogits.to(F64), keep.to(F64)
    d = cut * k * keep_scale
    dcut = (dl @ Wf) * k * (1.0 if mutate == "scale_once" else keep_scale)
    rows = []
    B = cut.shape[0]
    for lo in range(0, B, 64):
        hi = min(B, lo + 64)
        if mutate == "drop_last_sample" and hi - lo > 1:
            hi -= 1
        rows.append(torch.cat([(dl[lo:hi].T @ d[lo:hi]).reshape(-1), dl[lo:hi].sum(dim=0)]))
    return dcut, torch.stack(rows)


def head_int_case(B, seed, device="cpu"):
    """Integer cut in [0, 3] (exact in bf16), Wf in [-2, 2], bf in [-3, 3]; with keep_scale 2 a dropped value is at
    most 6, so |logit| <= 16384 * 2 * 6 + 3 < 2^24."""
    gen = torch.Generator().manual_seed(seed)
    cut = _ints(gen, 0, 3, (B, CUT_F))
    Wf = _ints(gen, -2, 2, (NCLS, CUT_F))
    bf = _ints(gen, -3, 3, (NCLS,))
    return cut.to(device), Wf.to(device), bf.to(device)
