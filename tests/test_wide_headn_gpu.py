"""The n-class K5 head (csrc/slk_wide_headn.hip) against tests/headn_ref.py: exactly on dyadic operands, within the
float64 bounds on the seeded model, the n-class evaluation kernels against numpy, and WideTrainer at 100 classes.
Sample tiles are 128 (logits) and 16 (dcut) samples, a K share of the weight gradient 256: B = 129 and 257 are the
smallest batches that put a second tile and a second share into every kernel."""
import numpy as np
import pytest
import torch

import headn_ref as R
from oracle import wide_step as W

pytestmark = pytest.mark.gpu
KS, THRESH = float(np.float32(4.0 / 3.0)), 1 << 30
BF = torch.bfloat16


def _guarded(shape, dtype=torch.float32):
    """A NaN-filled (0xFF for bf16 words) output with one guard row behind it: (whole, view)."""
    t = torch.full((shape[0] + 1,) + tuple(shape[1:]), float("nan"), dtype=dtype, device="cuda")
    return t, t[:shape[0]]


def _case(nc, B, seed=0, single=None):
    g = np.random.default_rng(seed)
    cut = g.integers(-8, 9, (B, R.CUT_F)) / 8.0
    wf = g.integers(-8, 9, (nc, R.CUT_F)) / 64.0
    if single is not None:   # one nonzero of the last sample
        cut[-1] = 0.0
        cut[-1, single] = 0.625
    return cut, wf, g.integers(-8, 9, nc) / 4.0, g.integers(-8, 9, (B, nc)) / 64.0


def _run(nc, B, cut, wf, bf, dl, thresh, ks, b0=0, step=0, seed=5):
    from splitcnn import ops
    dev = "cuda"
    cut_d = torch.from_numpy(R.c8(cut)).to(dev, BF)
    wq = ops.wide_fcn_shadow(torch.from_numpy(wf).float().reshape(-1).to(dev), nc)
    stp = torch.tensor([step], dtype=torch.int32, device=dev)
    work = torch.empty(ops.wide_headn_work(B), device=dev)
    lg_all, lg = _guarded((B, nc))
    ops.wide_headn_fwd(cut_d, wq, torch.from_numpy(bf).float().to(dev), nc, None, stp, seed, thresh, ks, 0.0, lg, work, b0=b0)
    dc_all, dc = _guarded((B, R.CUT_F), BF)
    sl_all, sl = _guarded((ops.wide_headn_nslab(B), nc * R.CUT_F + nc))
    ops.wide_headn_bwd(cut_d, wq, torch.from_numpy(dl).float().to(dev), nc, stp, seed, thresh, ks, dc, sl, work, b0=b0)
    torch.cuda.synchronize()
    for whole in (lg_all, dc_all, sl_all):
        assert torch.isnan(whole[-1].float()).all(), "guard row written"
    return wq, lg.cpu().numpy(), R.flat(dc.float().cpu().numpy().astype(np.float64)), sl, seed


def _check_exact(nc, B, thresh=THRESH, ks=KS, b0=0, step=0, single=None):
    from splitcnn import ops
    cut, wf, bf, dl = _case(nc, B, single=single)
    wq, lg, dc, sl, seed = _run(nc, B, cut, wf, bf, dl, thresh, ks, b0, step)
    keep = W.dropout_keep(seed, step, B, p=thresh / 2.0 ** 32, b0=b0).reshape(B, R.CUT_F) if thresh else np.ones_like(cut, bool)
    z, _, _ = R.logits(cut, wf, bf, keep, ks)
    assert np.array_equal(lg, z), "logits"
    dcut, slabs = R.backward(cut, wf, dl, keep, ks)
    assert np.array_equal(dc, dcut) and not np.signbit(dc[~keep]).any(), "dcut (dropped elements +0)"
    assert np.array_equal(sl.cpu().numpy(), slabs), "slabs"
    assert np.array_equal(ops.reduce_slabs(sl.contiguous()).cpu().numpy(), slabs.sum(axis=0, dtype=np.float32)), "slab sum"
    shadow = wq.float().cpu().numpy().reshape(2, -1)
    rows = shadow[0].reshape(128, R.CUT_F)
    assert np.array_equal(R.flat(rows[:nc]), wf) and not rows[nc:].any(), "class rows >= nc leave no trace"
    assert np.array_equal(shadow[1].reshape(R.CUT_F, 128).T, rows), "transposed shadow"


@pytest.mark.parametrize("B", [1, 17, 129, 257])
@pytest.mark.parametrize("nc", [2, 17, 100, 128])
def test_headn_exact_on_dyadic_operands(gpu, nc, B):
    _check_exact(nc, B)


@pytest.mark.parametrize("kw", [dict(thresh=0, ks=1.0), dict(b0=4093), dict(step=7), dict(single=0),
                                dict(single=R.CUT_F - 1)], ids=["no-dropout", "b0", "step", "first", "last"])
def test_headn_exact_cases(gpu, kw):
    _check_exact(100, 17, **kw)


def test_headn_seeded_model_within_float64_bounds(gpu, capsys):
    """The training form on the seeded model: logits against float64 on the same bf16 operands, loss_i and dlogits
    against the float64 cross-entropy of the kernel's own logits, then the same batch with two bad labels."""
    from splitcnn import ops
    from splitcnn.wide import KEEP_SCALE, KEEP_THRESHOLD, SyntheticCIFAR, WideClientStage, init_wide_models
    nc, B, gs = 100, 17, 1.0 / 17
    client, server = init_wide_models(0, num_classes=nc)
    x, _ = SyntheticCIFAR(3).batch(B)
    cut_d = WideClientStage(client, "cuda").forward(x.cuda()).reshape(B, R.CUT_F).clone()
    y = torch.arange(B, dtype=torch.int64) * 5 % nc
    wf, bf = server.fc.weight.detach().cuda(), server.fc.bias.detach().cuda()
    wq = ops.wide_fcn_shadow(wf.reshape(-1).contiguous(), nc)
    stp = torch.zeros(1, dtype=torch.int32, device="cuda")

    def fwd(labels):
        err = torch.zeros(1, dtype=torch.int32, device="cuda")
        lg, li, dl = (torch.full(s, float("nan"), device="cuda") for s in ((B, nc), (B,), (B, nc)))
        ops.wide_headn_fwd(cut_d, wq, bf, nc, labels.cuda(), stp, 0, KEEP_THRESHOLD, KEEP_SCALE, gs, lg, torch.empty(
            ops.wide_headn_work(B), device="cuda"), loss_i=li, dlogits=dl, err_flag=err)
        return int(err.item()), lg.cpu().numpy(), li.cpu().numpy(), dl.cpu().numpy()

    err, lg, li, dl = fwd(y)
    cut = R.flat(cut_d.float().cpu().numpy().astype(np.float64))
    keep = W.dropout_keep(0, 0, B, p=0.25).reshape(B, R.CUT_F)
    bf64 = bf.cpu().numpy().astype(np.float64)
    _, S, A = R.logits(cut, R.bf16(wf.cpu().numpy()), bf64, keep, KEEP_SCALE)
    loss, dl64, loss_b, dl_b = R.xent_bounds(lg, y.numpy(), gs)
    shares = [np.max(np.abs(a - r) / b) for a, r, b in ((lg, KEEP_SCALE * S + bf64, R.logits_bound(A, bf64, KEEP_SCALE)),
                                                       (li, loss, loss_b), (dl, dl64, dl_b))]
    with capsys.disabled():
        print(f"\nheadn float64 bounds used: logits {shares[0]:.3g}, loss {shares[1]:.3g}, dlogits {shares[2]:.3g}")
    assert err == 0 and max(shares) <= 1.0, shares
    yb = y.clone()
    yb[3], yb[5] = nc, -1   # a label outside [0, nc): the flag, that row's loss and dlogits NaN, every other row as before
    errb, lgb, lib, dlb = fwd(yb)
    bad = np.isin(np.arange(B), (3, 5))
    assert errb == 1 and np.array_equal(lgb, lg) and np.isnan(lib[bad]).all() and np.isnan(dlb[bad]).all()
    assert np.array_equal(lib[~bad], li[~bad]) and np.array_equal(dlb[~bad], dl[~bad])


def test_headn_one_class_through_the_c_entries(gpu):
    """The C entries also serve nc = 1 (the Python layer does not): logits = fl(ks S) + bf, loss 0, dlogits 0."""
    from splitcnn import _lib
    B, dev = 17, "cuda"
    cut, wf, bf, _ = _case(1, B)
    cut_d = torch.from_numpy(R.c8(cut)).to(dev, BF)
    wq = torch.empty(2 * 128 * R.CUT_F, dtype=BF, device=dev)
    wfd, bfd = torch.from_numpy(wf).float().reshape(-1).to(dev), torch.from_numpy(bf).float().to(dev)
    y, stp, err = (torch.zeros(n, dtype=t, device=dev) for n, t in ((B, torch.int64), (1, torch.int32), (1, torch.int32)))
    lg, li, dl = (torch.full(s, float("nan"), device=dev) for s in ((B, 1), (B,), (B, 1)))
    work = torch.empty(_lib.query("slk_wide_headn_work", B), device=dev)
    s = torch.cuda.current_stream().cuda_stream
    _lib.call("slk_wide_fcn_shadow", wfd.data_ptr(), 1, wq.data_ptr(), s)
    _lib.call("slk_wide_headn_fwd", cut_d.data_ptr(), wq.data_ptr(), bfd.data_ptr(), 1, y.data_ptr(), stp.data_ptr(), 5, THRESH,
              KS, 1.0, lg.data_ptr(), li.data_ptr(), dl.data_ptr(), work.data_ptr(), err.data_ptr(), 0, B, s)
    keep = W.dropout_keep(5, 0, B, p=0.25).reshape(B, R.CUT_F)
    assert np.array_equal(lg.cpu().numpy(), R.logits(cut, wf, bf, keep, KS)[0])
    assert int(err.item()) == 0 and not li.cpu().numpy().any() and not dl.cpu().numpy().any()


@pytest.mark.parametrize("nc", [2, 10, 100, 128])
def test_eval_n_against_numpy_and_the_ten_class_entries(gpu, nc):
    from splitcnn import ops
    g = torch.Generator().manual_seed(nc)
    acc = torch.zeros(4 + nc * nc, dtype=torch.int64, device="cuda")
    acc10 = torch.zeros(104, dtype=torch.int64, device="cuda")
    want = np.zeros((nc, nc), np.int64)
    n = correct = nbad = 0
    for B in (300, 37):   # two batches accumulated, the first past one 256-thread stride
        z = torch.randn(B, nc, generator=g)
        z[1, :] = z[1, 0]                      # an exact tie across the row: the first maximum wins
        z[2, nc - 1] = float("nan")            # a NaN logit counts as the maximum
        y = torch.randint(0, nc, (B,), generator=g)
        y[3], y[4] = nc, -1                    # bad labels
        err = torch.zeros(1, dtype=torch.int32, device="cuda")
        li, pred = ops.eval_logits_n(z.cuda(), y.cuda(), err_flag=err)
        ops.eval_accumulate_n(li, pred, y.cuda(), nc, acc)
        rp, rl, bad = R.eval_ref(z.numpy(), y.numpy())
        assert np.array_equal(pred.cpu().numpy(), rp) and int(err.item()) == 1
        got = li.cpu().numpy().astype(np.float64)
        ok = ~bad & ~np.isnan(rl)
        assert np.isnan(got[bad]).all() and np.allclose(got[ok], rl[ok], rtol=0, atol=(nc + 8) * R.U * (1 + np.abs(rl[ok]).max() + 8))
        assert np.array_equal(ops.eval_logits_n(z.cuda())[1].cpu().numpy(), rp), "predict only"
        np.add.at(want, (y.numpy()[~bad], rp[~bad]), 1)
        n, correct, nbad = n + B, correct + int((rp == y.numpy())[~bad].sum()), nbad + int(bad.sum())
        if nc == 10:   # bit for bit the 10-class entries
            l10, p10 = ops.eval_logits(z.cuda(), y.cuda())
            assert torch.equal(l10.view(torch.int32), li.view(torch.int32)) and torch.equal(p10, pred)
            ops.eval_accumulate(l10, p10, y.cuda(), acc10)
    a = acc.cpu().numpy()
    assert (a[0], a[1], a[2]) == (n, correct, nbad) and np.array_equal(a[4:].reshape(nc, nc), want)
    assert nc != 10 or torch.equal(acc, acc10)


def _batch(B, nc, seed):
    from splitcnn.wide import SyntheticCIFAR
    x, _ = SyntheticCIFAR(seed).batch(B)
    return x.cuda(), (torch.arange(B, dtype=torch.int64) * 13 % nc).cuda()


def test_trainer_100_classes_eager_graph_and_by_hand(gpu, tmp_path):
    from splitcnn import ops
    from splitcnn.cifar import Cifar100Bin, write_cifar100_bin
    from splitcnn.metrics import EvalMetrics
    from splitcnn.wide import KEEP_SCALE, KEEP_THRESHOLD, WideTrainer, init_wide_models
    nc, B = 100, 8
    runs = []
    for graph in (False, True):
        tr = WideTrainer(*init_wide_models(0, num_classes=nc), graph=graph)
        for s in range(2):
            tr.step(*_batch(B, nc, s))
        torch.cuda.synchronize()
        runs.append(tr)
    e, g = runs
    for a, b in ((e.client.params, g.client.params), (e.server.params, g.server.params), (e.server.m, g.server.m)):
        assert torch.equal(a, b), "eager and graphed steps differ"
    # the server half of step 2 composed by hand through ops, from the eager trainer's state before it
    ref = WideTrainer(*init_wide_models(0, num_classes=nc), graph=False)
    ref.step(*_batch(B, nc, 0))
    x, y = _batch(B, nc, 1)
    cut = ref.client.forward(x)
    s = ref.server
    wq = ops.wide_fcn_shadow(s.params[:s.nw], nc)
    lg, li, dl = (torch.empty(sh, device="cuda") for sh in ((B, nc), (B,), (B, nc)))
    err, work = torch.zeros(1, dtype=torch.int32, device="cuda"), torch.empty(ops.wide_headn_work(B), device="cuda")
    ops.wide_headn_fwd(cut, wq, s.params[s.nw:], nc, y, s.step_ctr, s.seed, KEEP_THRESHOLD, KEEP_SCALE, 1.0 / B, lg, work,
                       loss_i=li, dlogits=dl, err_flag=err)
    dcut, slabs = torch.empty_like(cut), torch.empty((ops.wide_headn_nslab(B), s.nparam), device="cuda")
    ops.wide_headn_bwd(cut, wq, dl, nc, s.step_ctr, s.seed, KEEP_THRESHOLD, KEEP_SCALE, dcut, slabs, work)
    grad = ops.reduce_slabs(slabs)
    ref.step(x, y)
    torch.cuda.synchronize()
    assert torch.equal(ref.server._logits, lg) and torch.equal(ref.server.grads, grad)
    assert torch.equal(ref.server._b("dcut", tuple(cut.shape), BF), dcut) and torch.equal(ref.server.params, e.server.params)
    # evaluate on a CIFAR-100 fixture
    rng = np.random.default_rng(0)
    fine = rng.integers(0, 100, 20)
    write_cifar100_bin(str(tmp_path / "test.bin"), rng.integers(0, 256, (20, 3, 32, 32), dtype=np.uint8), fine, fine // 5)
    ds = Cifar100Bin(str(tmp_path), train=False)
    assert ds.num_classes == 100 and np.array_equal(ds.labels, fine)
    assert np.array_equal(Cifar100Bin(str(tmp_path), train=False, labels="coarse").labels, fine // 5)
    xs = ((torch.from_numpy(ds.images).float() / 255 - 0.5) / 0.25).cuda()
    res = e.evaluate([(xs, torch.from_numpy(ds.labels).long().cuda())], metrics=EvalMetrics("cuda", num_classes=100))
    pred = e.predict(xs)
    assert res.n == 20 and res.bad_labels == 0 and res.confusion.shape == (100, 100)
    assert res.correct == int((pred.cpu().numpy() == fine).sum()) and np.isfinite(res.loss)


def test_refusals_and_the_ten_class_constructors(gpu):
    from splitcnn import dist, ops
    from splitcnn.loss import SoftCrossEntropy
    from splitcnn.wide import WideModelPartB, WideServerStage, WideTrainer, init_wide_models
    for bad in (1, 129, 0):
        with pytest.raises(ValueError, match="2..128"):
            WideModelPartB(num_classes=bad)
    with pytest.raises(ValueError, match="10 classes"):
        WideTrainer(*init_wide_models(0, num_classes=100), loss=SoftCrossEntropy(0.1))
    st = WideServerStage(WideModelPartB(100), "cuda")
    with pytest.raises(ValueError, match="10 classes"):
        st.forward_backward_records(None, "e4m3", None, 1.0, None, None)
    with pytest.raises(ValueError, match="10 classes"):
        st.accumulate_records(None, "e4m3", None, 1.0, 0, 0, 1, None, None)
    for cls, args in ((dist.WideHub, (st, 0, 2)), (dist.Hub, (st, 0, 2)), (dist.UShaped, (st, "server", 1)),
                      (dist.Pipeline, (st, "server", 1)), (dist.Replicated, (None, st)), (dist.FedAvg, (None, st))):
        with pytest.raises(ValueError, match="limited to 10 classes"):
            cls(*args)
    m = WideModelPartB(100).cuda()
    cut = torch.randn(3, 256, 8, 8, device="cuda").to(BF).requires_grad_(True)
    out = m(cut)
    assert out.shape == (3, 100)
    with pytest.raises(NotImplementedError, match="no module backward"):
        out.sum().backward()
    z, pr = torch.zeros(256, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda")
    for nc in (0, 129, -1):   # the C entries refuse a class count outside the kernels' range (on real buffers)
        assert ops._lib.load().slk_eval_logits_n(z.data_ptr(), nc, None, 1, None, pr.data_ptr(), None, None) == 1
    with pytest.raises(IndexError, match=r"\[0, 100\)"):
        st.err_flag.fill_(1)
        st.check_labels()
    # a 10-class trainer through the new constructors is today's, bit for bit
    a = WideTrainer(*init_wide_models(0), graph=False)
    b = WideTrainer(*init_wide_models(0, num_classes=10), graph=False)
    for tr in (a, b):
        tr.step(*_batch(8, 10, 0))
    torch.cuda.synchronize()
    assert torch.equal(a.server.params, b.server.params) and torch.equal(a.client.params, b.client.params)
    assert a.server.wf8.dtype == torch.float32 and a.server.PAIRS == ((0, 163850, 163840),)
