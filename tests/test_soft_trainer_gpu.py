"""loss=SoftCrossEntropy(...) in both trainers, mix=CutMix() into a trainer, the drop-in criterion, and the refusals.

  * loss=SoftCrossEntropy(0.0) on plain labels is the default trainer bit for bit over 3 steps (parameters, loss log,
    everything a step writes), graph and eager alike;
  * label_smoothing = 0.1 on mixed labels, one step:
      K2: ServerStage.grads and the logged loss against the float64 autograd reference (tests/dropin_ref64.py pooled
          by the kernel's routing code) driven with the float64 soft loss, at the bars of
          tests/test_dropin_autograd_gpu.py::test_canonical_step_three_paths_vs_float64 (rel_err <= 1e-4 per gradient
          tensor, 1e-5 relative for the loss);
      K5: the head's dlogits and loss_i against oracle.wide_step.server_step's float64 logits with the float64 soft
          loss, at the bars of tests/test_wide_gpu.py::test_wide_step_layer_by_layer_vs_oracle (dlogits atol 2e-7,
          loss_i rtol 2e-6 + 1e-6); the logged loss is the float32 fixed-order mean of those loss_i (1e-6 relative);
  * a default trainer fed a mixed batch raises IndexError from check_labels, a loss= trainer does not;
  * CifarLoader(augment, mix) into WideTrainer(loss=) over two epochs: finite, clean, reproducible bit for bit;
  * model_def.CrossEntropyLoss(label_smoothing=0.1) under autograd; dist refuses loss= stages."""
import numpy as np
import pytest
import torch

import dropin_ref64 as D
import ref64
import soft_ref64 as S
from conftest import rel_err
from oracle import wide_step as W

pytestmark = pytest.mark.gpu

BATCHES = [16, 33]


def k2(gpu, seed=3, **kw):
    from splitcnn.data import init_models
    from splitcnn.engine import SplitTrainer
    return SplitTrainer(*init_models(seed=seed), device=gpu, **kw)


def k5(gpu, seed=0, **kw):
    from splitcnn.wide import WideTrainer, init_wide_models
    return WideTrainer(*init_wide_models(seed=seed), device=gpu, **kw)


def k2_batches(gpu, B, n, seed=7):
    from splitcnn.data import SyntheticMNIST
    data = SyntheticMNIST(seed)
    return [tuple(t.to(gpu) for t in data.batch(B)) for _ in range(n)]


def k5_batches(gpu, B, n, seed=9):
    from splitcnn.wide import SyntheticCIFAR
    data = SyntheticCIFAR(seed)
    return [tuple(t.to(gpu) for t in data.batch(B)) for _ in range(n)]


def mixed(y, seed=1):
    """Mixed labels over the plain labels y: partner = the batch rolled by one, weights of every kind."""
    from splitcnn.loss import pack_mixed
    g = torch.Generator().manual_seed(seed)
    wb = torch.rand(y.shape[0], generator=g)
    wb[0], wb[-1] = 0.0, 1.0
    return pack_mixed(y, y.roll(1), wb.to(y.device))


def losses(tr):
    torch.cuda.synchronize()
    return [l for _, l in tr.loss_log.flush()]


def _np(t):
    return t.detach().float().cpu().numpy().astype(np.float64)


# ----------------------------------------------------------------------------- smoothing 0 == the default trainer
@pytest.mark.parametrize("which", ["k2", "k5"])
@pytest.mark.parametrize("B", BATCHES)
def test_soft_loss_zero_is_the_default_trainer_bitwise(gpu, which, B):
    from splitcnn.loss import SoftCrossEntropy
    make, batches = (k2, k2_batches(gpu, B, 3)) if which == "k2" else (k5, k5_batches(gpu, B, 3))
    runs = {}
    for name, kw in (("default/graph", dict(graph=True)), ("soft/graph", dict(graph=True, loss=SoftCrossEntropy(0.0))),
                     ("soft/eager", dict(graph=False, loss=SoftCrossEntropy(0.0)))):
        tr = make(gpu, **kw)
        assert (tr.server.loss is None) == name.startswith("default")
        for x, y in batches:
            tr.step(x, y)
        torch.cuda.synchronize()
        tr.server.check_labels()
        runs[name] = ([t.clone() for t in tr._state()], [t.clone() for t in tr._optim_state().values()], losses(tr))
    want = runs["default/graph"]
    assert len(want[2]) == 3 and all(np.isfinite(want[2]))
    for name, got in runs.items():
        assert all(torch.equal(a, b) for a, b in zip(got[0], want[0])), f"{name}: the state a step writes differs"
        assert all(torch.equal(a, b) for a, b in zip(got[1], want[1])), f"{name}: the optimizer state differs"
        assert got[2] == want[2], f"{name}: the loss log differs"


# ----------------------------------------------------------------------------- one step against float64
@pytest.mark.parametrize("B", BATCHES)
def test_k2_soft_step_meets_the_float64_autograd_reference(gpu, B):
    from splitcnn import ops
    from splitcnn.loss import SoftCrossEntropy
    eps = 0.1
    (x, y), = k2_batches(gpu, B, 1, seed=11 + B)
    ym = mixed(y)
    for graph in (False, True):
        tr = k2(gpu, graph=graph, loss=SoftCrossEntropy(eps))
        sd = {k: v.detach().clone() for m in (tr.client.model, tr.server.model) for k, v in m.state_dict().items()}
        # the kernels' routing code at these parameters, held to float64 (as tests/test_dropin_autograd_gpu.py's Data)
        act = ops.conv1_fwd(x, sd["conv1.weight"], sd["conv1.bias"])
        _, code = ops.conv2_fwd_pool(act, sd["conv2.weight"], sd["conv2.bias"], impl="x3", act_amax=ops.row_amax(act))
        ref64.assert_routing_ties(act, sd["conv2.weight"], sd["conv2.bias"], code)
        tr.step(x, ym)
        torch.cuda.synchronize()
        tr.server.check_labels()
        grads, (logged,) = tr.server.grads.clone(), losses(tr)

        A, Bm = D.load64(D.RefPartA(), {k: v for k, v in sd.items() if k.startswith("conv1")}), \
            D.load64(D.RefPartB(), {k: v for k, v in sd.items() if not k.startswith("conv1")})
        logits = Bm(A(x.double().cpu()), code.cpu())
        t = torch.from_numpy(S.targets64(ym.cpu().numpy(), eps))
        loss = -(t * torch.log_softmax(logits, dim=1)).sum(dim=1).mean()
        closed = S.soft_xent64(logits.detach().numpy(), ym.cpu().numpy(), eps)[0].mean()
        assert abs(loss.item() - closed) <= 1e-12
        loss.backward()
        err = abs(logged - loss.item()) / abs(loss.item())
        print(f"B={B} graph={graph}: logged loss relative {err:.3g}")
        assert err <= 1e-5
        want = {"conv2.weight": (0, 18432), "conv2.bias": (18432, 18496), "fc1.weight": (18496, 110656),
                "fc1.bias": (110656, 110666)}
        for name, (lo, hi) in want.items():
            e = rel_err(_np(grads[lo:hi]), dict(Bm.named_parameters())[name].grad.numpy().ravel())
            print(f"B={B} graph={graph}: grad {name} rel_err {e:.3g}")
            assert e <= 1e-4, (name, e)


@pytest.mark.parametrize("B", BATCHES)
def test_k5_soft_head_meets_the_float64_oracle(gpu, B):
    from splitcnn.loss import SoftCrossEntropy
    from splitcnn.wide import c8_to_nchw
    eps = 0.1
    (x, y), = k5_batches(gpu, B, 1, seed=20 + B)
    ym = mixed(y)
    tr = k5(gpu, graph=False, loss=SoftCrossEntropy(eps))
    c, s = tr.client, tr.server
    P0 = {k: _np(v) for m in (c.model, s.model) for k, v in m.state_dict().items()}
    cut = c.forward(x)
    dcut, loss_i = s.step_request(cut, ym)
    c.backward_step(dcut)
    torch.cuda.synchronize()
    s.check_labels()
    sv = W.server_step(P0, _np(c8_to_nchw(cut)), y.cpu().numpy(), W.dropout_keep(0, 0, B))
    loss64, d64, _, _ = S.soft_xent64(sv["logits"], ym.cpu().numpy(), eps, grad_scale=1.0 / B)
    np.testing.assert_allclose(_np(loss_i), loss64, rtol=2e-6, atol=1e-6)
    np.testing.assert_allclose(_np(s._dlogits), d64, rtol=0, atol=2e-7)
    (logged,) = losses(tr)
    assert abs(logged - _np(loss_i).mean()) <= 1e-6 * abs(_np(loss_i).mean())
    # ... and the hard-label oracle on the same logits is a different loss (the test can tell them apart)
    assert np.abs(_np(loss_i) - sv["loss_i"]).max() > 1e-2


def test_k2_every_head_path_runs_the_soft_entry(gpu):
    """The stage's three head paths — logits + cross-entropy in one launch (the default), the two-launch split, and
    the fused fc_xent — are the same kernels in other launch shapes: with loss= they stay bit-identical to each other
    (as they are without), and none of them is the hard-label head (which would flag the mixed batch)."""
    from splitcnn.loss import SoftCrossEntropy
    batches = k2_batches(gpu, 33, 2, seed=5)
    runs = {}
    for name, knobs in (("one launch", {}), ("two launches", {"fc_one_launch": False}), ("fused fc_xent", {"fc_split": False})):
        tr = k2(gpu, graph=False, loss=SoftCrossEntropy(0.1))
        for k, v in knobs.items():
            assert hasattr(tr.server, k)
            setattr(tr.server, k, v)
        for i, (x, y) in enumerate(batches):
            tr.step(x, mixed(y, seed=i))
        torch.cuda.synchronize()
        tr.server.check_labels()
        runs[name] = (tr.client.params.clone(), tr.server.params.clone(), tr.server.grads.clone(), losses(tr))
    want = runs["one launch"]
    for name, got in runs.items():
        assert all(torch.equal(a, b) for a, b in zip(got[:3], want[:3])) and got[3] == want[3], name


# ----------------------------------------------------------------------------- mixed labels need loss=
@pytest.mark.parametrize("which", ["k2", "k5"])
def test_mixed_batch_needs_a_soft_loss(gpu, which):
    from splitcnn.loss import SoftCrossEntropy
    make, ((x, y),) = (k2, k2_batches(gpu, 16, 1)) if which == "k2" else (k5, k5_batches(gpu, 16, 1))
    ym = mixed(y)
    assert int((ym >= 2 ** 32).sum()) >= 14
    tr = make(gpu, graph=False)
    tr.step(x, ym)
    with pytest.raises(IndexError, match=r"a label was out of range \[0, 10\).*malformed"):
        tr.server.check_labels()
    tr = make(gpu, graph=False, loss=SoftCrossEntropy(0.1))
    tr.step(x, ym)
    tr.server.check_labels()
    assert all(np.isfinite(losses(tr)))
    # a malformed target is flagged by the soft head as well
    bad = ym.clone()
    bad[3] = 10
    tr.step(x, bad)
    with pytest.raises(IndexError, match="malformed"):
        tr.server.check_labels()
    for T in (make,):
        with pytest.raises(TypeError, match="SoftCrossEntropy"):
            T(gpu, loss=0.1)


# ----------------------------------------------------------------------------- loader -> trainer
class _Set:
    def __init__(self, images, labels):
        self.images, self.labels = images, labels

    def __len__(self):
        return len(self.images)


def test_cifar_loader_with_cutmix_trains_the_wide_trainer_reproducibly(gpu):
    from splitcnn.cifar import Augment, CifarLoader
    from splitcnn.loss import CutMix, SoftCrossEntropy, unpack_mixed
    rng = np.random.default_rng(8)
    ds = _Set(rng.integers(0, 256, size=(100, 3, 32, 32), dtype=np.uint8), rng.integers(0, 10, size=100).astype(np.uint8))
    runs = []
    for _ in range(2):
        ld = CifarLoader(ds, batch_size=32, shuffle=True, seed=5, device=gpu, augment=Augment(), mix=CutMix())
        tr = k5(gpu, graph=True, loss=SoftCrossEntropy(0.1))
        seen = 0
        for _epoch in range(2):
            for x, y in ld:
                if not seen:
                    assert float(unpack_mixed(y)[2].max()) > 0, "the loader's labels are mixed"
                tr.step(x, y)
                seen += x.shape[0]
        torch.cuda.synchronize()
        tr.server.check_labels()
        assert seen == 200 and ld.epoch == 2 and int(ld.err.item()) == 0
        log = losses(tr)
        assert len(log) == 8 and all(np.isfinite(log))
        runs.append((tr.client.params.clone(), tr.server.params.clone(), log))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]) and runs[0][2] == runs[1][2]


# ----------------------------------------------------------------------------- the drop-in criterion
@pytest.mark.parametrize("B", [3, 17])
def test_dropin_criterion_with_label_smoothing(gpu, B):
    from splitcnn import library
    from splitcnn.model_def import CrossEntropyLoss
    eps = 0.1
    g = torch.Generator().manual_seed(B)
    z = (torch.randn(B, 10, generator=g) * 4).to(gpu)
    y = torch.randint(0, 10, (B,), generator=g).to(gpu)
    ym = mixed(y)

    def run(crit, labels):
        zz = z.clone().requires_grad_(True)
        loss = crit(zz, labels)
        (3.0 * loss).backward()
        return loss.detach().clone(), zz.grad.clone()

    crit = CrossEntropyLoss(label_smoothing=eps)
    loss, grad = run(crit, ym)
    z64, y64 = z.double().cpu().numpy(), ym.cpu().numpy()
    loss64, d64, p64, _ = S.soft_xent64(z64, y64, eps, grad_scale=1.0 / B)
    # the mean of B losses each inside its bound, summed in float32 (B more roundings of values below the sum)
    lim = S.soft_loss_bound(z64, y64, eps, loss64).mean() + B * 2.0 ** -24 * np.abs(loss64).sum() / B
    assert abs(loss.item() - loss64.mean()) <= lim
    lim_g = 3.0 * S.soft_grad_bound(z64, y64, eps, p64, grad_scale=1.0 / B) + 2.0 ** -23 * np.abs(3.0 * d64)
    assert (np.abs(_np(grad) - 3.0 * d64) <= lim_g).all()
    # eager Functions and the torch.library custom op: the same bits
    eager = library._EAGER
    try:
        library._EAGER = False
        loss_op, grad_op = run(crit, ym)
    finally:
        library._EAGER = eager
    assert torch.equal(loss_op, loss) and torch.equal(grad_op, grad)
    # plain labels through the soft form (label_smoothing = 0, mixed=True) and through today's form: the same bits
    hard = run(CrossEntropyLoss(), y)
    zz = z.clone().requires_grad_(True)
    today = library.CrossEntropyFn.apply(zz, y)
    (3.0 * today).backward()
    assert torch.equal(hard[0], today.detach()) and torch.equal(hard[1], zz.grad)
    soft0 = run(CrossEntropyLoss(mixed=True), y)
    assert torch.equal(soft0[0], hard[0]) and torch.equal(soft0[1], hard[1])
    # label_smoothing on class indices (wb = 0) is nn.CrossEntropyLoss(label_smoothing=eps)
    ls = run(crit, y)
    want = torch.nn.functional.cross_entropy(z.double().cpu(), y.cpu(), label_smoothing=eps)
    assert abs(ls[0].item() - want.item()) <= 1e-5 * abs(want.item())
    # a mixed label in the hard-label form is loud
    assert not torch.isfinite(run(CrossEntropyLoss(), ym)[0])
    with pytest.raises(ValueError):
        CrossEntropyLoss(label_smoothing=1.5)


# ----------------------------------------------------------------------------- dist refuses loss=
def test_dist_refuses_soft_loss_stages(gpu):
    from splitcnn import dist as sd
    from splitcnn.engine import ClientStage, ServerStage
    from splitcnn.loss import SoftCrossEntropy
    from splitcnn.wide import WideServerStage
    soft = SoftCrossEntropy(0.1)
    server, wide = ServerStage(device=gpu, loss=soft), WideServerStage(device=gpu, loss=soft)
    client = ClientStage(device=gpu)
    for make in (lambda: sd.Replicated(client, server), lambda: sd.Hub(server, 0, 1), lambda: sd.FedAvg(client, server),
                 lambda: sd.Pipeline(server, "server", 0), lambda: sd.WideHub(wide, 0, 1)):
        with pytest.raises(ValueError, match="soft-target loss.*without loss="):
            make()
    sd._default_optimizer_only("Hub", ServerStage(device=gpu))      # a default stage passes
