"""slk_dcor_grad (privacy.DcorLoss, WideTrainer(leak_loss=...)) against the rule of include/slk.h, "Distance correlation
gradient", in float64 numpy under the same tau, rounded to bf16 last.

The allowance is not a constant. Per case a reference-side emulation of what the kernels round (float32 Gram distances,
float64 centring, u rounded to bf16, row sums of the rounded values, float64 product, bf16 output) is compared with the
float64 reference; the case's yardstick is the emulation's largest per-row relative L2 error, and every row of the
kernel's output may use 4 x that, relative to the reference row's norm (the margin is for float32 accumulation in
another order). Asserted on the reference side: no pair sits within a factor 4 of the resolution threshold, and the
yardstick stays at or below 1e-2. dcut is random bf16 at the scale of the reference term (so neither part hides the
other) in one pass and zero in the other.

Two of the cases are degenerate: with two distinct points (n = 2, and "duplicates" at n = 3) b is proportional to a,
dCor^2 is identically 1 and the exact gradient is 0, so the reference term is the rounding noise of a weight that
cancels and there is no row norm to be relative to. They are recognised on the reference side (1 - dCor^2 < 1e-12) and
assert what still can go wrong there instead: with a unit-scale random dcut the output is dcut bit for bit, and with a
zero dcut every row stays under the term that weights of (tau_x + tau_z) a_ij / b_ij would give — the float32
distances carry up to tau / 2 relative error each and the weights are of order a / b, while a wrong pair or a lost
centring term leaves weights of order a / b itself, a thousand times that. Yardsticks and used shares
are recorded in profiles/nopeek_check.txt."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NS = (2, 3, 127, 128, 129, 300)
DIMS = ((64, 64), (64, 192), (3072, 16384))     # one K step; ragged against a 128- or 256-wide feature tile; K5
KINDS = ("relu", "linear", "duplicates")
ALPHA = 0.5


POOL = []    # the module's device memory pool, kept until the process ends


@pytest.fixture(scope="module", autouse=True)
def private_device_memory():
    """Every device allocation of this module comes from a memory pool of its own that is never released: the module
    fills workspaces and outputs with NaN on purpose, and neither torch's shared cache nor the runtime's own (which hands
    a freed block back uncleared) may pass those blocks to a later test's torch.empty. The shared cache is left as it
    was found."""
    POOL.append(torch.cuda.MemPool())
    with torch.cuda.use_mem_pool(POOL[0]):
        yield
        from splitcnn import privacy
        privacy._DCOR_GRAD_WORKSPACES.clear()
        privacy._DCOR_WORKSPACES.clear()


def bf16(v):
    return torch.from_numpy(np.ascontiguousarray(v)).to(torch.bfloat16)


def bf16_round(v):
    return bf16(v).double().numpy()


@functools.lru_cache(maxsize=None)
def base(dx, dz):
    g = np.random.default_rng(2000 + dx + dz)
    return (g.standard_normal((max(NS), dx), dtype=np.float32), g.standard_normal((max(NS), dz), dtype=np.float32),
            g.integers(0, dx, (2, dz)), g.uniform(0.5, 1.5, (2, dz)).astype(np.float32),
            g.standard_normal((max(NS), dz), dtype=np.float32))


def inputs(kind, n, dx, dz):
    """x float32 [n, dx], z bf16 [n, dz] and unit-scale gradient noise [n, dz] (torch / numpy, CPU) of a value class."""
    xb, zb, idx, coef, noise = base(dx, dz)
    x, z = xb[:n].copy(), zb[:n].copy()
    if kind == "linear":        # a fixed sparse random linear map of x, rounded to bf16: dCor close to 1
        z = x[:, idx[0]] * coef[0] + x[:, idx[1]] * coef[1]
    elif kind == "relu":        # about half zeros
        z = np.maximum(z, 0)
    elif kind == "duplicates":  # rows 0 and n - 1 equal in both operands
        x[n - 1], z[n - 1] = x[0], z[0]
    return torch.from_numpy(x), bf16(z), noise[:n]


def distances(x, z, tau_x, tau_z, dtype):
    """a, b (float64 values of distances computed in `dtype`) and d2 / (s_i + s_j) of every pair of distinct rows."""
    out, ratios = [], []
    for v, tau in ((x, tau_x), (z, tau_z)):
        v = v.astype(dtype)
        s = (v * v).sum(1)
        sm = s[:, None] + s[None, :]
        d2 = sm - 2 * (v @ v.T)
        ratios.append(((d2 / np.where(sm > 0, sm, 1))[~np.eye(len(v), dtype=bool)], tau))
        d = np.sqrt(np.where(d2 <= dtype(tau) * sm, 0, d2))
        np.fill_diagonal(d, 0)
        out.append(d.astype(np.float64))
    return out[0], out[1], ratios


def term(a, b, z, alpha, squared, round_u):
    """alpha * d dCor^2 / d z (dCor for squared=False) in float64 from the distances, with dCor^2 and the factor f."""
    n = float(len(a))

    def centred(d):
        r = d.sum(1)
        return d - r[:, None] / n - r[None, :] / n + r.sum() / n ** 2
    ab, bb = centred(a), centred(b)
    c, vx, vz = (ab * b).sum() / n ** 2, (ab * a).sum() / n ** 2, (bb * b).sum() / n ** 2
    if vx * vz <= 0 or c <= 0:      # where the closed form clamps there is no term
        return np.zeros_like(z), None, 0.0
    u = np.where(b > 0, (ab - c / vz * bb) / np.where(b > 0, b, 1), 0)
    if round_u:
        u = bf16_round(u)
    f = alpha * 2 / (n ** 2 * np.sqrt(vx * vz))
    if not squared:
        f /= 2 * np.sqrt(c / np.sqrt(vx * vz))
    return f * (u.sum(1)[:, None] * z - u @ z), c / np.sqrt(vx * vz), f


@functools.lru_cache(maxsize=None)
def expected(kind, n, dx, dz, squared, tau_x, tau_z):
    """Per dcut pass (random, zero): dcut (bf16 torch), the float64 reference rounded to bf16, its row norms and the
    yardstick — or, for the zero pass of a degenerate case, None and the rows' noise floors."""
    x, z, noise = inputs(kind, n, dx, dz)
    x, z = x.numpy(), z.double().numpy()
    a, b, ratios = distances(x, z, tau_x, tau_z, np.float64)
    for r, tau in ratios:
        assert not ((r >= tau / 4) & (r <= 4 * tau)).any(), "a pair sits at the resolution threshold: change the input"
    ref, r2, f = term(a, b, z, ALPHA, squared, False)
    a32, b32, _ = distances(x, z, tau_x, tau_z, np.float32)
    emu = term(a32, b32, z, ALPHA, squared, True)[0]
    assert (r2 is None) == (n == 2 and kind == "duplicates")        # two equal rows: every distance is 0
    degenerate = r2 is not None and 1 - r2 < 1e-12
    assert degenerate == (r2 is not None and (n == 2 or (n == 3 and kind == "duplicates")))
    out = []
    scale = 1.0 if degenerate or r2 is None else np.sqrt((ref ** 2).mean())
    for dcut in (bf16(noise * scale), bf16(np.zeros_like(noise))):
        d = dcut.double().numpy()
        want, have = bf16_round(d + ref), bf16_round(d + emu)
        norm = np.sqrt((want ** 2).sum(1))
        if degenerate and not d.any():
            out.append((dcut, want, (tau_x + tau_z) * f * a.sum(1), None))
            continue
        yard = (np.sqrt(((have - want) ** 2).sum(1)) / np.where(norm > 0, norm, 1)).max()
        assert yard <= 1e-2, f"the yardstick {yard} exceeds 1e-2: change the input"
        out.append((dcut, want, norm, yard))
    return out


def workspace_nan(device, n):
    from splitcnn import privacy
    privacy._DCOR_GRAD_WORKSPACES[(device, n)].view(torch.float32).fill_(float("nan"))


def run(loss, x, z, dcut, inplace=False):
    """add_grad with the cached workspace and `out` pre-filled with NaN and a sentinel row behind row n - 1."""
    n = x.shape[0]
    stats = torch.full((8,), -7.0, device="cuda")
    buf = torch.full((n + 1,) + tuple(z.shape[1:]), float("nan"), dtype=torch.bfloat16, device="cuda")
    loss.add_grad(x, z, dcut, out=buf[:n], stats=stats[:4])          # makes the workspace of this n exist
    workspace_nan(x.device, n)
    buf.fill_(float("nan"))
    if inplace:
        buf[:n] = dcut
    got = loss.add_grad(x, z, buf[:n] if inplace else dcut, out=None if inplace else buf[:n], stats=stats[:4])
    assert got.data_ptr() == buf.data_ptr() and buf[n].isnan().all() and (stats[4:] == -7.0).all()
    return got, stats[:4]


@pytest.mark.parametrize("squared", (True, False))
@pytest.mark.parametrize("dx,dz", DIMS)
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("kind", KINDS)
def test_against_float64(kind, n, dx, dz, squared):
    from splitcnn import privacy
    x, z, _ = inputs(kind, n, dx, dz)
    x, z = x.cuda(), z.cuda()
    loss = privacy.DcorLoss(ALPHA, squared=squared)
    passes = expected(kind, n, dx, dz, squared, privacy.dcor_tau("x"), privacy.dcor_tau("z"))
    for name, (dcut, want, norm, yard) in zip(("random", "zero"), passes):
        got, stats = run(loss, x, z, dcut.cuda())
        got = got.double().cpu().numpy()
        assert np.isfinite(got).all()
        if yard is None:    # a degenerate case's zero pass: `norm` holds the rows' noise floors (see the docstring)
            rows = np.sqrt((got ** 2).sum(1))
            print(f"nopeek_check {kind} n={n} dx={dx} dz={dz} squared={squared} dcut={name} degenerate: "
                  f"used={(rows / norm).max():.3g} of the noise floor")
            assert (rows <= norm).all()
            continue
        if yard == 0:       # nothing for the term to change (a degenerate case's random pass, a clamped form)
            assert np.array_equal(got, want)
            continue
        err = np.sqrt(((got - want) ** 2).sum(1)) / norm
        print(f"nopeek_check {kind} n={n} dx={dx} dz={dz} squared={squared} dcut={name} yardstick={yard:.3e} "
              f"worst row={err.max():.3e} used={err.max() / (4 * yard):.3f}")
        assert (err <= 4 * yard).all(), (err.max(), yard)
    assert torch.equal(stats.view(torch.int32), privacy.distance_correlation(x, z).values.view(torch.int32))


def bits(t):
    return t.contiguous().view(torch.int16)


@pytest.mark.parametrize("n,dx,dz", ((129, 64, 192), (300, 64, 64)))
def test_exact_cases(n, dx, dz):
    from splitcnn import privacy
    x, z, noise = inputs("relu", n, dx, dz)
    x, z, dcut = x.cuda(), z.cuda(), bf16(noise).cuda()
    dcut[0, 0], dcut[1, 1] = -0.0, float("inf")           # bits an addition of 0 would not keep
    loss = privacy.DcorLoss(3.0)
    first, stats = run(loss, x, z, dcut)
    assert not torch.equal(bits(first), bits(dcut))
    again, _ = run(loss, x, z, dcut)                        # the same bits every run; in place equals out of place
    inplace, _ = run(loss, x, z, dcut, inplace=True)
    assert torch.equal(bits(again), bits(first)) and torch.equal(bits(inplace), bits(first))
    zero, _ = run(privacy.DcorLoss(0.0), x, z, dcut)        # alpha = 0
    assert torch.equal(bits(zero), bits(dcut))
    same = z[:1].expand_as(z).contiguous()                  # identical cut rows: Vz = 0, the closed form clamps
    flat, stats = run(loss, x, same, dcut)
    assert torch.equal(bits(flat), bits(dcut)) and stats[0].item() == 0 and stats[3].item() == 0
    xn = x.clone()
    xn[n // 2, dx // 3] = float("nan")
    bad, stats = run(loss, xn, z, dcut)
    assert bad.isnan().all() and stats.isnan().all()
    one, stats = run(loss, x[:1], z[:1], dcut[:1])          # n = 1 copies
    assert torch.equal(bits(one), bits(dcut[:1])) and (stats == 0).all()


def test_graph_replay_follows_alpha_and_inputs():
    from splitcnn import privacy
    n, dx, dz = 129, 64, 192
    x0, z0, noise = inputs("relu", n, dx, dz)
    x1, z1, _ = inputs("linear", n, dx, dz)
    x, z, dcut = x0.cuda(), z0.cuda(), bf16(noise).cuda()
    out, stats = torch.zeros_like(dcut), torch.zeros(4, device="cuda")
    loss = privacy.DcorLoss(1.5)
    loss.add_grad(x, z, dcut, out=out, stats=stats)           # the workspace exists before the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss.add_grad(x, z, dcut, out=out, stats=stats)
    loss.set_alpha(3.0)
    for xi, zi in ((x1, z1), (x0, z0)):
        x.copy_(xi)
        z.copy_(zi)
        graph.replay()
        replayed, rstats = out.clone(), stats.clone()
        estats = torch.zeros(4, device="cuda")
        eager = privacy.DcorLoss(3.0).add_grad(x, z, dcut, out=torch.zeros_like(dcut), stats=estats)
        assert torch.equal(bits(replayed), bits(eager)) and torch.equal(rstats.view(torch.int32), estats.view(torch.int32))
        assert not torch.equal(bits(replayed), bits(dcut))


def test_refusals():
    from splitcnn import privacy
    for alpha in (-1.0, float("nan"), float("inf"), "1", True):
        with pytest.raises(ValueError, match="alpha"):
            privacy.DcorLoss(alpha)
    loss = privacy.DcorLoss(1.0)
    with pytest.raises(ValueError, match="alpha"):
        loss.set_alpha(-2.0)
    with pytest.raises(TypeError, match="DcorLoss"):
        privacy.check_dcor_loss(1.0)
    x, z = torch.zeros(4, 64, device="cuda"), torch.zeros(4, 128, dtype=torch.bfloat16, device="cuda")
    for args, err in (((x.double(), z, z), TypeError), ((x, z.float(), z), TypeError), ((x, z, z.float()), TypeError),
                      ((x[:, :32].contiguous(), z, z), ValueError), ((x, z[:, :96].contiguous(), z[:, :96].contiguous()), ValueError),
                      ((x[:3], z, z), ValueError), ((x, z, z[:3]), ValueError),
                      ((x.view(-1)[1:129].view(2, 64), z[:2], z[:2]), ValueError),
                      ((x, torch.zeros(4 * 128 + 8, dtype=torch.bfloat16, device="cuda")[1:-7].view(4, 128), z), ValueError)):
        with pytest.raises(err):
            loss.add_grad(*args)
    with pytest.raises(ValueError, match="stats"):
        loss.add_grad(x, z, z.clone(), stats=torch.zeros(3, device="cuda"))
    with pytest.raises(ValueError, match="out"):
        loss.add_grad(x, z, z.clone(), out=torch.zeros(4, 64, dtype=torch.bfloat16, device="cuda"))


def trainer(graph, **kw):
    from splitcnn.wide import WideTrainer, init_wide_models
    return WideTrainer(*init_wide_models(seed=0), device="cuda", graph=graph, **kw)


def batch():
    g = torch.Generator().manual_seed(5)
    return torch.randn(8, 3, 32, 32, generator=g).cuda(), torch.randint(0, 10, (8,), generator=g).cuda()


def same_params(p, q):
    return all(torch.equal(getattr(p, st).params, getattr(q, st).params) for st in ("client", "server"))


@pytest.mark.parametrize("graph", (False, True))
def test_trainer_alpha_zero_and_stats_leave_the_step_alone(graph):
    """alpha = 0 lands on leak_loss=None's bits after three steps; leak_stats() between two steps changes nothing and
    equals the distance correlation of (x, the raw cut the step saw)."""
    from splitcnn import privacy
    x, y = batch()
    plain, zero, read = trainer(graph), trainer(graph, leak_loss=privacy.DcorLoss(0.0)), trainer(graph, leak_loss=privacy.DcorLoss(0.0))
    raw = plain.client.forward(x, tag="eval").clone()        # the first step's raw cut: the same weights, no dropout
    for k in range(3):
        for tr in (plain, zero, read):
            tr.step(x, y)
        if k == 0:
            got = read.leak_stats()
            want = privacy.distance_correlation(x, raw)
            assert torch.equal(got.values.view(torch.int32), want.values.view(torch.int32)) and 0 < got.dcor <= 1
    torch.cuda.synchronize()
    assert same_params(plain, zero) and same_params(plain, read)
    with pytest.raises(RuntimeError, match="leak_loss"):
        plain.leak_stats()


@pytest.mark.parametrize("graph", (False, True))
def test_trainer_step_equals_the_public_pieces(graph):
    """One step with alpha > 0 and a clipping CutNoise against the same step composed by hand."""
    from splitcnn import privacy
    x, y = batch()
    noise = lambda: privacy.CutNoise("gaussian", scale=0.0, clip=1.0, seed=3)
    tr = trainer(graph, cut_noise=noise(), leak_loss=privacy.DcorLoss(50.0))
    tr.step(x, y)
    hand, nz, loss = trainer(False), noise(), privacy.DcorLoss(50.0)
    c, s = hand.client, hand.server
    raw = c.forward(x)
    stats = torch.zeros(8, 2, device="cuda")
    cut = nz.apply(raw, torch.empty_like(raw), step=c.step_ctr, stats=stats)
    dcut = s.step_request(cut, y)[0]
    nz.scale_rows(dcut, stats, dcut)
    before = dcut.clone()
    loss.add_grad(x, raw, dcut)
    assert not torch.equal(bits(before), bits(dcut))          # the term is not lost in bf16 at this alpha
    c.backward_step(dcut)
    torch.cuda.synchronize()
    assert same_params(tr, hand)
    assert (stats[:, 1] < 1).any()                            # the clip did clip
