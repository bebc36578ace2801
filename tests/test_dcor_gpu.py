"""slk_dcor (privacy.distance_correlation) against a float64 numpy reference of the rule in include/slk.h.

The tolerance is not a constant: per case it is 16 x the error of a plain float32 emulation of the same formula
(float32 square norms and Gram blocks by numpy, the same resolution rule, float64 finishing, float32 outputs like the
kernel's) against the float64 reference on the same inputs. The yardstick of a case is the emulation's largest relative
error among its nonzero outputs, and every output is allowed 16 x that, relative to its own reference value: one
output's error alone is a single draw of float32 output rounding, anywhere between 0 and half an ulp, while the
largest of three or four is a stable measure of what float32 loses here. An output whose reference is 0 must be 0.
Every input keeps the allowance at or below 1e-4 on dcor, and no pair of rows sits within a factor 4 of the resolution
threshold, so the rule never decides a case (both asserted below, on the reference side). Yardsticks and measured
errors are recorded in profiles/dcor_check.txt."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NS = (2, 3, 127, 128, 129, 300)           # one tile, its edge, ragged tiles, three tiles with a ragged last one
DIMS = ((64, 64), (3072, 16384))          # one K step; the K5 operands
KINDS = ("independent", "linear", "relu", "identical", "duplicates", "nan")


@pytest.fixture(scope="module", autouse=True)
def private_device_memory():
    """Every device allocation of this module comes from a memory pool of its own, released at the end: the module
    fills workspaces with NaN on purpose, and torch's shared cache would hand those blocks to a later test's
    torch.empty."""
    pool = torch.cuda.MemPool()
    with torch.cuda.use_mem_pool(pool):
        yield
        from splitcnn import privacy
        privacy._DCOR_WORKSPACES.clear()
    del pool
    torch.cuda.empty_cache()


def statistic(x, z, tau_x, tau_z, dtype):
    """(dcor, dcov2, dvar_x, dvar_z) with distances in `dtype` and float64 sums; also
    d2 / (s_i + s_j) of every pair of distinct rows, for the resolution-margin assert."""
    dist, ratios = [], []
    for v, tau in ((x, tau_x), (z, tau_z)):
        v = v.astype(dtype)
        s = (v * v).sum(1)
        sm = s[:, None] + s[None, :]
        d2 = sm - 2 * (v @ v.T)
        r = (d2 / np.where(sm > 0, sm, 1))[~np.eye(len(v), dtype=bool)]
        ratios.append((r, tau))
        d = np.sqrt(np.where(d2 <= dtype(tau) * sm, 0, d2))
        np.fill_diagonal(d, 0)
        dist.append(d.astype(np.float64))
    a, b = dist
    n = float(len(a))

    def dcov2(p, q):
        return (p * q).sum() / n ** 2 - 2 * (p.sum(1) * q.sum(1)).sum() / n ** 3 + p.sum() * q.sum() / n ** 4
    cov, vx, vz = dcov2(a, b), dcov2(a, a), dcov2(b, b)
    cor = 0.0 if vx * vz <= 0 else np.sqrt(max(cov, 0) / np.sqrt(vx * vz))
    return np.array([cor, cov, vx, vz]), ratios


@functools.lru_cache(maxsize=None)
def base(dx, dz):
    g = np.random.default_rng(1000 + dx)
    return (g.standard_normal((max(NS), dx), dtype=np.float32), g.standard_normal((max(NS), dz), dtype=np.float32),
            g.integers(0, dx, (2, dz)), g.uniform(0.5, 1.5, (2, dz)).astype(np.float32))


def bf16(v):
    return torch.from_numpy(np.ascontiguousarray(v)).to(torch.bfloat16)


def inputs(kind, n, dx, dz):
    """x float32 [n, dx] and z bf16 [n, dz] (torch, CPU) of one value class."""
    xb, zb, idx, coef = base(dx, dz)
    x, z = xb[:n].copy(), zb[:n].copy()
    if kind == "linear":        # a fixed sparse random linear map of x, rounded to bf16: dCor close to 1
        z = x[:, idx[0]] * coef[0] + x[:, idx[1]] * coef[1]
    elif kind == "relu":        # about half zeros
        z = np.maximum(z, 0)
    elif kind == "identical":
        z[:] = z[0]
    elif kind == "duplicates":  # rows 0 and n - 1 equal in both operands (exact zero distances among distinct rows)
        x[n - 1], z[n - 1] = x[0], z[0]
    elif kind == "nan":
        x[n // 2, dx // 3] = np.nan
    return torch.from_numpy(x), bf16(z)


@functools.lru_cache(maxsize=None)
def expected(kind, n, dx, dz, tau_x, tau_z):
    """The float64 reference and the allowance on each output, from the reference side only."""
    x, z = inputs(kind, n, dx, dz)
    x, z = x.numpy(), z.float().numpy()
    ref, ratios = statistic(x, z, tau_x, tau_z, np.float64)
    for r, tau in ratios:
        assert not ((r >= tau / 4) & (r <= 4 * tau)).any(), "a pair sits at the resolution threshold: change the input"
    emu, _ = statistic(x, z, tau_x, tau_z, np.float32)
    rel = np.abs(emu.astype(np.float32).astype(np.float64) - ref)[ref != 0] / np.abs(ref[ref != 0])
    allow = 16 * rel.max(initial=0.0) * np.abs(ref)
    assert allow[0] <= 1e-4, "the allowance on dcor exceeds 1e-4: change the input"
    return ref, allow


def run(x, z, out=None):
    """distance_correlation with the cached workspace pre-filled with NaN and a sentinel behind the outputs."""
    from splitcnn import privacy
    n = x.shape[0]
    buf = torch.full((8,), -7.0, device="cuda") if out is None else out
    privacy.distance_correlation(x, z, out=buf[:4])          # makes the workspace of this n exist
    privacy._DCOR_WORKSPACES[(x.device, n)].view(torch.float32).fill_(float("nan"))
    buf[:4] = -7.0
    res = privacy.distance_correlation(x, z, out=buf[:4])
    assert res.values.data_ptr() == buf.data_ptr() and (buf[4:] == -7.0).all()
    return res


@pytest.mark.parametrize("dx,dz", DIMS)
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("kind", KINDS)
def test_against_float64(kind, n, dx, dz):
    from splitcnn import privacy
    x, z = inputs(kind, n, dx, dz)
    res = run(x.cuda(), z.cuda())
    got = res.values.double().cpu().numpy()
    assert np.array_equal([res.dcor, res.dcov2, res.dvar_x, res.dvar_z], got, equal_nan=True)
    if kind == "nan":
        assert np.isnan(got).all()
        return
    ref, allow = expected(kind, n, dx, dz, privacy.dcor_tau("x"), privacy.dcor_tau("z"))
    err = np.abs(got - ref)
    print(f"dcor_check {kind} n={n} dx={dx} dz={dz} ref={ref.tolist()} allow={allow.tolist()} err={err.tolist()}")
    if kind == "identical":
        assert got[0] == 0 and got[3] == 0 and got[1] == 0
    assert (err <= allow).all(), (err, allow)
    again = run(x.cuda(), z.cuda()).values
    assert torch.equal(again.view(torch.int32).cpu(), res.values.view(torch.int32).cpu())   # the same bits every run


def test_graph_replay_follows_changed_inputs():
    """The launch captured once, replayed over inputs changed in place: every replay equals the eager result."""
    from splitcnn import privacy
    n, dx, dz = 129, 64, 64
    xs = [inputs(k, n, dx, dz) for k in ("independent", "linear", "relu")]
    x, z = xs[0][0].cuda(), xs[0][1].cuda()
    out = torch.zeros(4, device="cuda")
    privacy.distance_correlation(x, z, out=out)               # workspace exists before the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        privacy.distance_correlation(x, z, out=out)
    for xi, zi in xs[1:] + xs[:1]:
        x.copy_(xi)
        z.copy_(zi)
        graph.replay()
        replayed = out.clone()
        eager = privacy.distance_correlation(x, z).values
        assert torch.equal(replayed.view(torch.int32), eager.view(torch.int32))


def test_trainer_cut_leakage_reads_only():
    """WideTrainer.cut_leakage at B = 8: the statistic of (x, the evaluation cut) bit for bit, and the step after
    it lands where a trainer that never called it lands."""
    from splitcnn import privacy
    from splitcnn.wide import WideTrainer, init_wide_models
    g = torch.Generator().manual_seed(5)
    x = torch.randn(8, 3, 32, 32, generator=g).cuda()
    y = torch.randint(0, 10, (8,), generator=g).cuda()
    trainers = [WideTrainer(*init_wide_models(seed=0), device="cuda", graph=False) for _ in range(2)]
    for k, tr in enumerate(trainers):
        tr.step(x, y)
        if k == 0:
            res = tr.cut_leakage(x)
            direct = privacy.distance_correlation(x, tr.eval_cut)
            assert torch.equal(res.values.view(torch.int32), direct.values.view(torch.int32))
            assert 0 < res.dcor <= 1 and res.dvar_x > 0 and res.dvar_z > 0
        tr.step(x, y)
    torch.cuda.synchronize()
    for st in ("client", "server"):
        assert torch.equal(getattr(trainers[0], st).params, getattr(trainers[1], st).params)
