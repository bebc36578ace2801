"""GPU tests of the evaluation / prediction path (K2): the fc head's evaluation mode, slk_eval_logits,
the metric accumulator, the code-less conv2 forward, and SplitTrainer.eval_batch / evaluate / predict
against the golden fixtures, the float64 oracle and the training forward.

Tolerances: logits rel_err <= 1e-5 and loss relative <= 1e-5 against the fixtures / the oracle (the
forward's bar in test_gpu_parity.py); predictions must equal argmax of the reference logits for every
sample whose reference top-2 margin is >= 2e-5 * max|logit| (one 1e-5 per logit) — with these inputs
that is every sample, and the tests assert that none is excluded. Everything compared between two of
this library's own paths (evaluation vs training forward, graph vs eager, x3p vs x3i) is bitwise."""
import functools

import numpy as np
import pytest
import torch

from conftest import FIXTURES, load_fixture, rel_err

pytestmark = pytest.mark.gpu


def bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


# ------------------------------------------------------------------------------------ the head
@functools.lru_cache(maxsize=None)
def head_case(B):
    """Random non-negative pooled, fc weights and labels, and the training head's logits / loss_i (computed
    once per B and shared; nothing modifies them)."""
    from splitcnn import ops
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(1000 + B)
    pooled = torch.rand(B, 64, 12, 12, generator=g).mul_(torch.rand(B, 1, 1, 1, generator=g) * 2).to(dev)
    W3 = (torch.randn(10, 9216, generator=g) * 0.02).to(dev)
    b3 = (torch.randn(10, generator=g) * 0.1).to(dev)
    y = torch.randint(0, 10, (B,), generator=g).to(dev)
    logits, loss_i, _ = ops.fc_logits_xent(pooled, W3, b3, y, 1.0 / B)
    torch.cuda.synchronize()
    return pooled, W3, b3, y, logits, loss_i


@pytest.mark.parametrize("B", [1, 15, 16, 17, 33])   # one workgroup, the ragged last one, two workgroups of 16
def test_fc_eval_bitwise_vs_training_head(gpu, B):
    from splitcnn import ops
    pooled, W3, b3, y, logits_t, loss_t = head_case(B)
    logits, loss_i, pred = ops.fc_eval(pooled, W3, b3, y)
    assert same_bits(logits, logits_t)
    assert same_bits(loss_i, loss_t)
    assert pred.dtype == torch.int64
    want = np.argmax(logits_t.cpu().numpy(), axis=1)
    assert np.array_equal(pred.cpu().numpy(), want)
    # predict only: the loss buffer keeps its fill, the flag is not touched, pred is the same
    fill = torch.full((B,), -7.0, device=gpu)
    flag = torch.zeros(1, dtype=torch.int32, device=gpu)
    _, l2, p2 = ops.fc_eval(pooled, W3, b3, None, loss_i=fill, err_flag=flag)
    assert l2 is fill and bool((fill == -7.0).all()) and int(flag.item()) == 0
    assert torch.equal(p2, pred)
    # logits not stored: the same loss and prediction
    lg3, l3, p3 = ops.fc_eval(pooled, W3, b3, y, store_logits=False)
    assert lg3 is None and same_bits(l3, loss_t) and torch.equal(p3, pred)


# ------------------------------------------------------------------------------------ eval_logits
def test_eval_logits_crafted_rows(gpu):
    from splitcnn import ops
    inf, nan = float("inf"), float("nan")
    rows = np.zeros((12, 10), dtype=np.float32)
    rows[0] = [1, 5, 5, 0, -1, 2, 5, 0, 0, 0]            # exact three-way tie of the maximum -> 1
    rows[1] = [0, 0, 0, 0, 3, 0, 0, 0, 3, 0]             # two-way tie -> 4
    rows[2] = 2.0                                         # ten-way tie -> 0
    rows[3] = [9, 8, 7, 6, 5, 4, 3, nan, 2, 1]           # NaN at class 7 -> 7
    rows[4] = [0, 0, inf, 0, 0, 0, 0, nan, 0, 0]         # NaN beats +inf -> 7
    rows[5] = [0, nan, 0, 0, 0, 0, 0, nan, 0, 0]         # the first NaN -> 1
    rows[6] = [0, 0, 0, inf, 0, 0, 0, 0, 0, 0]           # +inf -> 3
    rows[7] = [0, 0, 0, inf, 0, 0, inf, 0, 0, 0]         # two +inf -> 3
    rows[8] = [-inf] * 4 + [0.5] + [-inf] * 5            # -inf everywhere else -> 4
    rows[9] = -inf                                        # all -inf: ten-way tie -> 0
    rows[10] = [-3, -2, -1, -1, -2, -3, -4, -5, -6, -1]  # negative maximum, tie -> 2
    rows[11] = [0, 0, 0, 0, 0, 0, 0, 0, 0, 1e-30]        # last class
    want = [1, 4, 0, 7, 7, 1, 3, 3, 4, 0, 2, 9]
    assert np.array_equal(np.argmax(rows, axis=1), want)   # the stated numpy semantics
    _, pred = ops.eval_logits(torch.from_numpy(rows).to(gpu))
    assert pred.cpu().tolist() == want


def test_eval_logits_bitwise_vs_fc_eval_and_bad_labels(gpu):
    from splitcnn import ops
    from splitcnn.metrics import EvalMetrics, evaluate_logits
    pooled, W3, b3, y, logits_t, loss_t = head_case(33)
    _, loss_h, pred_h = ops.fc_eval(pooled, W3, b3, y)
    loss_i, pred = ops.eval_logits(logits_t, y)
    assert same_bits(loss_i, loss_h) and same_bits(loss_i, loss_t) and torch.equal(pred, pred_h)
    # a label of 10 and a label of -1
    yb = y.clone()
    yb[3], yb[20] = 10, -1
    flag = torch.zeros(1, dtype=torch.int32, device=gpu)
    lb, pb = ops.eval_logits(logits_t, yb, err_flag=flag)
    _, lh, ph = ops.fc_eval(pooled, W3, b3, yb, err_flag=torch.zeros(1, dtype=torch.int32, device=gpu))
    assert int(flag.item()) == 1
    lbn = lb.cpu().numpy()
    assert np.isnan(lbn[[3, 20]]).all() and np.isnan(lh.cpu().numpy()[[3, 20]]).all()
    ok = np.ones(33, dtype=bool)
    ok[[3, 20]] = False
    assert np.array_equal(lbn[ok].view(np.int32), loss_t.cpu().numpy()[ok].view(np.int32))
    assert torch.equal(pb, pred_h) and torch.equal(ph, pred_h)
    m = EvalMetrics(gpu)
    p2, l2 = evaluate_logits(logits_t, yb, m)
    assert torch.equal(p2, pred_h)
    r = m.result()
    yn, pn = yb.cpu().numpy(), pred_h.cpu().numpy()
    conf = np.zeros((10, 10), dtype=np.int64)
    np.add.at(conf, (yn[ok], pn[ok]), 1)
    assert (r.n, r.bad_labels, r.correct) == (33, 2, int((yn[ok] == pn[ok]).sum()))
    assert np.array_equal(r.confusion, conf)
    want = float(lbn[ok].astype(np.float64).sum()) / 31
    assert abs(r.loss - want) <= 1e-10 * abs(want)
    with pytest.raises(IndexError, match="out of range"):
        r.check()


# ------------------------------------------------------------------------------------ the accumulator
def acc_case(B, seed):
    g = torch.Generator().manual_seed(seed)
    loss = torch.rand(B, generator=g) * 3
    pred = torch.randint(0, 10, (B,), generator=g)
    y = torch.where(torch.rand(B, generator=g) < 0.5, pred, torch.randint(0, 10, (B,), generator=g))
    return loss, pred, y


def acc_want(loss, pred, y):
    conf = np.zeros((10, 10), dtype=np.int64)
    np.add.at(conf, (y.numpy(), pred.numpy()), 1)
    return len(y), int((pred == y).sum()), conf, float(loss.numpy().astype(np.float64).sum())


@pytest.mark.parametrize("B", [1, 255, 256, 257, 1000])
def test_eval_accumulate(gpu, B):
    from splitcnn.metrics import EvalMetrics
    loss, pred, y = acc_case(B, 7 + B)
    n, correct, conf, lsum = acc_want(loss, pred, y)
    dl, dp, dy = loss.to(gpu), pred.to(gpu), y.to(gpu)
    m = EvalMetrics(gpu)
    m.update(dl, dp, dy)
    raw1 = m.acc.clone()
    r = m.result()
    assert (r.n, r.correct, r.bad_labels) == (n, correct, 0)
    assert np.array_equal(r.confusion, conf)
    # n * 2^-53 ~ 1e-13 for n <= 1000 bounds any float64 summation order; 1e-10 leaves two orders of margin
    assert abs(r.loss * n - lsum) <= 1e-10 * lsum
    assert abs(r.accuracy - correct / n) == 0
    # run to run: the same bits
    m2 = EvalMetrics(gpu)
    m2.update(dl, dp, dy)
    assert torch.equal(m2.acc, raw1)
    # three updates = one update over the concatenation
    parts = [acc_case(B, 100 * k + B) for k in range(3)]
    cat = [torch.cat([p[i] for p in parts]) for i in range(3)]
    n3, c3, conf3, l3 = acc_want(*cat)
    m.reset()
    assert int(m.acc.abs().sum().item()) == 0
    for p in parts:
        m.update(*(t.to(gpu) for t in p))
    r3 = m.result()
    one = EvalMetrics(gpu)
    one.update(*(t.to(gpu) for t in cat))
    r1 = one.result()
    for rr in (r3, r1):
        assert (rr.n, rr.correct, rr.bad_labels) == (n3, c3, 0)
        assert np.array_equal(rr.confusion, conf3)
        assert abs(rr.loss * n3 - l3) <= 1e-10 * l3


# ------------------------------------------------------------------------------------ code-less conv2
@pytest.mark.parametrize("B", [1, 5, 86, 173])   # 3 units on 3 workgroups, 15, 258 (two per workgroup), 519 (ragged)
def test_conv2_fwd_pool_x3p_bitwise_vs_x3i(gpu, B):
    from splitcnn import ops
    from splitcnn.data import SyntheticMNIST, init_models
    a, b = init_models(seed=B)
    a, b = a.to(gpu), b.to(gpu)
    x, _ = SyntheticMNIST(100 + B).batch(B)
    x = x.to(gpu)
    amax = torch.empty(B, device=gpu)
    a16 = torch.empty(ops.conv2_act16_bytes(B), dtype=torch.uint8, device=gpu)
    ops.conv1_fwd_x3(x, a.conv1.weight.detach(), a.conv1.bias.detach(), amax, a16)
    W2, b2 = b.conv2.weight.detach(), b.conv2.bias.detach()
    want, _ = ops.conv2_fwd_pool_x3i(a16, amax, W2, b2)
    nb = B * 9216
    buf = torch.empty(nb * 4 + nb, dtype=torch.uint8, device=gpu)   # pooled, then a code-sized guard
    pooled = buf[:nb * 4].view(torch.float32).view(B, 64, 12, 12)
    guard = buf[nb * 4:]
    for it in range(5):   # a stale-image race would show as rare wrong tiles
        pooled.fill_(float("nan"))
        guard.fill_(0xA5)
        ops.conv2_fwd_pool_x3p(a16, amax, W2, b2, pooled=pooled)
        assert same_bits(pooled, want), it
        assert bool((guard == 0xA5).all()), it


# ------------------------------------------------------------------------------------ trainer: fixtures
KEYS = {"W1": "conv1.weight", "b1": "conv1.bias", "W2": "conv2.weight", "b2": "conv2.bias", "W3": "fc1.weight",
        "b3": "fc1.bias"}


def trainer_from(fx, key, gpu, **kw):
    from splitcnn.engine import SplitTrainer
    from splitcnn.model_def import ModelPartA, ModelPartB
    a, b = ModelPartA(), ModelPartB()
    a.load_state_dict({KEYS[k]: torch.from_numpy(fx[key.format(k)]) for k in ("W1", "b1")})
    b.load_state_dict({KEYS[k]: torch.from_numpy(fx[key.format(k)]) for k in ("W2", "b2", "W3", "b3")})
    return SplitTrainer(a, b, device=gpu, **kw)


def check_fixture_step(tr, fx, s, gpu):
    from splitcnn.metrics import EvalMetrics
    x, y = torch.from_numpy(fx[f"x_{s}"]).to(gpu), torch.from_numpy(fx[f"y_{s}"]).to(gpu)
    m = EvalMetrics(gpu)
    pred, loss_i = tr.eval_batch(x, y, m)
    want = fx[f"logits_{s}"]
    e_logits = rel_err(tr.server.eval_logits.cpu().numpy(), want)
    loss, want_loss = float(loss_i.double().mean().item()), float(fx[f"loss_{s}"])
    print(f"step {s}: logits rel_err {e_logits:.3g}, loss rel {abs(loss - want_loss) / abs(want_loss):.3g}")
    assert e_logits <= 1e-5
    assert abs(loss - want_loss) <= 1e-5 * abs(want_loss)
    assert np.array_equal(pred.cpu().numpy(), np.argmax(want, axis=1))   # every sample (smallest margin 2e-3)
    r = m.result()
    assert r.n == len(want) and r.correct == int((np.argmax(want, axis=1) == fx[f"y_{s}"]).sum())
    assert abs(r.loss - want_loss) <= 1e-5 * abs(want_loss)


@pytest.mark.parametrize("name", FIXTURES)
def test_eval_batch_matches_reference_fixture(gpu, name):
    fx = load_fixture(name)
    tr = trainer_from(fx, "init_{}", gpu)
    check_fixture_step(tr, fx, 1, gpu)
    if int(fx["nsteps"]) >= 2:   # split_step_b4: step 2 from the reference's own post-step-1 weights ...
        tr = trainer_from(fx, "post_{}_1", gpu)
        check_fixture_step(tr, fx, 2, gpu)
        # ... and step 3 after this engine's own step 2 from them (the fixture keeps no post-step-2 weights)
        tr.step(torch.from_numpy(fx["x_2"]).to(gpu), torch.from_numpy(fx["y_2"]).to(gpu))
        check_fixture_step(tr, fx, 3, gpu)


# ------------------------------------------------------------------------------------ trainer: oracle
@functools.lru_cache(maxsize=None)
def oracle_case(B):
    """init_models(seed=B), SyntheticMNIST(100 + B).batch(B) and the float64 oracle forward (CPU, once per B)."""
    from oracle import split_step as O
    from splitcnn.data import SyntheticMNIST, init_models
    a, b = init_models(seed=B)
    x, y = SyntheticMNIST(100 + B).batch(B)
    p = {k: v.detach().double().numpy() for k, v in {**a.state_dict(), **b.state_dict()}.items()}
    act = O.client_forward(x.double().numpy(), p["conv1.weight"], p["conv1.bias"])
    pooled, _ = O.maxpool2(O.relu(O.conv3x3(act, p["conv2.weight"], p["conv2.bias"])))
    logits = pooled.reshape(B, -1) @ p["fc1.weight"].T + p["fc1.bias"]
    loss, loss_i, _ = O.cross_entropy(logits, y.numpy())
    return a.state_dict(), b.state_dict(), x, y, logits, float(loss)


@pytest.mark.parametrize("B", [33, 86, 173])
def test_evaluate_vs_oracle_graph_and_eager(gpu, B):
    from splitcnn.engine import SplitTrainer
    from splitcnn.model_def import ModelPartA, ModelPartB
    sd_a, sd_b, x, y, want, want_loss = oracle_case(B)
    top2 = np.sort(want, axis=1)[:, -2:]
    margin = top2[:, 1] - top2[:, 0]
    keep = margin >= 2e-5 * np.abs(want).max()
    print(f"B {B}: max|logit| {np.abs(want).max():.3g}, smallest top-2 margin {margin.min():.3g}")
    assert int((~keep).sum()) == 0   # with these inputs the oracle excludes no sample
    got = {}
    for graph in (True, False):
        a, b = ModelPartA(), ModelPartB()
        a.load_state_dict(sd_a)
        b.load_state_dict(sd_b)
        tr = SplitTrainer(a, b, device=gpu, graph=graph)
        r = tr.evaluate([(x.to(gpu), y.to(gpu))])
        logits = tr.server.eval_logits.clone()
        pred = tr.predict(x.to(gpu))
        e = rel_err(logits.cpu().numpy(), want)
        print(f"  graph={graph}: logits rel_err {e:.3g}, loss rel {abs(r.loss - want_loss) / want_loss:.3g}")
        assert e <= 1e-5
        assert abs(r.loss - want_loss) <= 1e-5 * want_loss
        assert np.array_equal(pred.cpu().numpy()[keep], np.argmax(want, axis=1)[keep])
        assert r.n == B and r.correct == int((np.argmax(want, axis=1) == y.numpy()).sum())
        assert len(tr._eval_graphs) == (1 if graph else 0) and len(tr._graphs) == 0
        got[graph] = (logits, pred, r)
    assert same_bits(got[True][0], got[False][0]) and torch.equal(got[True][1], got[False][1])
    assert got[True][2].loss == got[False][2].loss and np.array_equal(got[True][2].confusion, got[False][2].confusion)


# ------------------------------------------------------------------------------------ trainer: trained weights
@pytest.mark.parametrize("conv", ["x3", "f32"])
def test_eval_batch_bitwise_vs_training_forward(gpu, conv):
    from splitcnn.data import SyntheticMNIST, init_models
    from splitcnn.engine import SplitTrainer
    B = 64
    a, b = init_models(seed=3)
    tr = SplitTrainer(a, b, device=gpu, conv=conv)
    data = SyntheticMNIST(5)
    for _ in range(20):
        x, y = data.batch(B)
        tr.step(x.to(gpu), y.to(gpu))
    x, y = (t.to(gpu) for t in data.batch(B))
    pred, loss_i = tr.eval_batch(x, y)
    logits_e, loss_e, pred_e = tr.server.eval_logits.clone(), loss_i.clone(), pred.clone()
    # forward + backward with no optimizer step on the same batch
    c, s = tr.client, tr.server
    act = c.forward(x)
    _, loss_t, _, _ = s.forward_backward(act, y, 1.0 / B, act_amax=c._act_amax,
                                         act16=c._act16 if c.emit_act16 else None)
    logits_t = s._buf.get("logits", (B, 10), torch.float32, gpu)
    assert same_bits(logits_e, logits_t)
    assert same_bits(loss_e, loss_t)
    assert np.array_equal(pred_e.cpu().numpy(), np.argmax(logits_t.cpu().numpy(), axis=1))


# ------------------------------------------------------------------------------------ no side effects
def test_evaluate_leaves_training_state_alone(gpu):
    from splitcnn.data import SyntheticMNIST, init_models
    from splitcnn.engine import SplitTrainer
    B = 32
    data = SyntheticMNIST(9)
    b1, b2, b3 = (tuple(t.to(gpu) for t in data.batch(B)) for _ in range(3))

    def run(evaluate):
        a, b = init_models(seed=2)
        tr = SplitTrainer(a, b, device=gpu, graph=True)
        tr.step(*b1)
        if evaluate:
            state = [tr.client.params, tr.client.grads, tr.server.params, tr.server.grads, tr.loss_log.counter,
                     tr.server.err_flag]
            before = [t.clone() for t in state]
            gs, ng = tr.global_step, len(tr._graphs)
            r = tr.evaluate([b3, b3])
            assert r.n == 2 * B
            tr.predict(b3[0])
            for t, v in zip(state, before):
                assert same_bits(t, v)
            assert tr.global_step == gs and len(tr._graphs) == ng and len(tr._eval_graphs) == 1
        tr.step(*b2)
        torch.cuda.synchronize()
        return tr.client.params.clone(), tr.server.params.clone(), [v for _, v in tr.loss_log.flush()]

    c0, s0, l0 = run(False)
    c1, s1, l1 = run(True)
    assert same_bits(c0, c1) and same_bits(s0, s1)
    assert len(l0) == 2 and np.array_equal(np.float32(l0).view(np.int32), np.float32(l1).view(np.int32))


def test_stage_level_evaluation_between_forward_and_backward(gpu):
    """forward ... evaluate ... backward_step on the stages (a remote client's f32 cut): the training step's
    result does not change, and ServerStage.evaluate(act=...) gives the head's training logits."""
    from splitcnn.data import SyntheticMNIST, init_models
    from splitcnn.engine import ClientStage, ServerStage
    from splitcnn.metrics import EvalMetrics
    B = 17
    data = SyntheticMNIST(11)
    (x, y), (xe, ye) = (tuple(t.to(gpu) for t in data.batch(B)) for _ in range(2))

    def run(evaluate):
        a, b = init_models(seed=6)
        c, s = ClientStage(a, device=gpu), ServerStage(b, device=gpu)
        act = c.forward(x)
        if evaluate:
            m = EvalMetrics(gpu)
            acte, _, _ = c.forward_eval(xe)
            s.evaluate(acte, ye, metrics=m)
            assert m.result().n == B
        cut_grad, _ = s.step_request(act, y, step=0)
        if evaluate:   # the same cut through evaluate: the training forward's logits, bit for bit
            s2 = ServerStage(init_models(seed=6)[1], device=gpu)
            s2.evaluate(act, y)
            assert same_bits(s2.eval_logits, s._buf.get("logits", (B, 10), torch.float32, gpu))
        c.backward_step(cut_grad)
        return c.params.clone(), s.params.clone()

    c0, s0 = run(False)
    c1, s1 = run(True)
    assert same_bits(c0, c1) and same_bits(s0, s1)


# ------------------------------------------------------------------------------------ two batch sizes
def test_eval_logits_follow_the_replayed_batch_size(gpu):
    """A ragged loader (32, 32, 32, 4) leaves graphs for two batch sizes; a replay runs no Python, so
    server.eval_logits must still be the logits of the batch eval_batch was just given — bitwise eager's."""
    from splitcnn.data import SyntheticMNIST, init_models
    from splitcnn.engine import SplitTrainer
    data = SyntheticMNIST(21)
    b32a, b4, b32b = (tuple(t.to(gpu) for t in data.batch(B)) for B in (32, 4, 32))
    tg = SplitTrainer(*init_models(seed=8), device=gpu, graph=True)
    te = SplitTrainer(*init_models(seed=8), device=gpu, graph=False)
    tg.eval_batch(*b32a)          # captures B = 32
    tg.eval_batch(*b4)            # captures B = 4: the last capture
    assert len(tg._eval_graphs) == 2
    for xb, yb in (b32b, b4, b32a):   # replays only
        pg, lg = tg.eval_batch(xb, yb)
        pe, le = te.eval_batch(xb, yb)
        assert tuple(tg.server.eval_logits.shape) == (xb.shape[0], 10)
        assert same_bits(tg.server.eval_logits, te.server.eval_logits)
        assert same_bits(lg, le) and torch.equal(pg, pe)
    assert len(tg._eval_graphs) == 2


# ------------------------------------------------------------------------------------ loader
def test_evaluate_over_a_device_loader(gpu, tmp_path):
    from splitcnn import mnist
    from splitcnn.data import init_models
    from splitcnn.engine import SplitTrainer
    rng = np.random.default_rng(5)
    imgs = rng.integers(0, 256, size=(100, 28, 28), dtype=np.uint8)
    lbls = rng.integers(0, 10, size=(100,), dtype=np.uint8)
    mnist.write_idx(str(tmp_path / "t10k-images-idx3-ubyte"), imgs)
    mnist.write_idx(str(tmp_path / "t10k-labels-idx1-ubyte"), lbls)
    ds = mnist.MnistIDX(str(tmp_path), train=False)
    a, b = init_models(seed=1)
    tr = SplitTrainer(a, b, device=gpu)
    r32 = tr.evaluate(mnist.DeviceLoader(ds, 32, shuffle=False, device=gpu))     # 3 full batches + a ragged 4
    r100 = tr.evaluate(mnist.DeviceLoader(ds, 100, shuffle=False, device=gpu))
    assert r32.n == 100 and r100.n == 100
    assert r32.correct == r100.correct and np.array_equal(r32.confusion, r100.confusion)
    assert np.array_equal(r32.confusion.sum(axis=1), np.bincount(lbls, minlength=10))
    assert abs(r32.loss - r100.loss) <= 1e-10 * abs(r100.loss)
    r32.check()
