"""The K5 drop-in modules (WideModelPartA / WideModelPartB / WideFullModel, splitcnn/wide.py) under autograd use
beyond the reference's step: scaled losses, accumulation, retain_graph, a frozen head, a cut that does not
require grad, two training forwards before their backward passes (each backward must use its own forward's
dropout mask), eval mode, a float32 gradient into the bf16 cut, and the loud failures.

The canonical module step (the reference's step pattern on fresh modules) is pinned to the stages and to
oracle/wide_step.py by tests/test_wide_gpu.py, so the patterns here are held to it bit for bit: a power-of-two
loss scale is exact in bf16 and f32 alike, an accumulated .grad is the f32 (bf16 for the cut leaf) sum. The
dropout mask is the hash of (seed, forward count, sample, feature): "warm = n" below is a fresh module whose
counter was advanced by n throw-away training forwards.

B = 5, the batch tests/test_wide_gpu.py::test_wide_step_layer_by_layer_vs_oracle uses as ragged."""
import numpy as np
import pytest
import torch

from oracle import wide_step as W
from wide_ref64 import bf16_close, grad_close

pytestmark = pytest.mark.gpu

B = 5
_CACHE = {}


def batches(gpu):
    if "batches" not in _CACHE:
        from splitcnn.wide import SyntheticCIFAR
        gen = SyntheticCIFAR(42)
        _CACHE["batches"] = [tuple(t.to(gpu) for t in gen.batch(B)) for _ in range(2)]
    return _CACHE["batches"]


def fresh(gpu, warm=0):
    from splitcnn.model_def import CrossEntropyLoss
    from splitcnn.wide import init_wide_models
    client, server = (m.to(gpu) for m in init_wide_models(seed=0))
    for _ in range(warm):
        with torch.no_grad():
            server(torch.zeros(1, 256, 8, 8, dtype=torch.bfloat16, device=gpu))
    return client, server, CrossEntropyLoss()


def counter(server):
    return 0 if server._drop_step is None else int(server._drop_step.item())


def _leaf(act, grad=True):
    return act.clone().detach().requires_grad_(grad)


def _val(v):
    return None if v is None else v.detach().clone()


def _snap(mods, sfx="", **tensors):
    out = {k + sfx: _val(v) for k, v in tensors.items()}
    for m in mods:
        for n, p in m.named_parameters():
            out["grad_" + n + sfx] = _val(p.grad)
    return out


def assert_bitwise(got, want, what=""):
    assert got.keys() == want.keys(), (what, sorted(got), sorted(want))
    for k in want:
        if want[k] is None or got[k] is None:
            assert got[k] is None and want[k] is None, (what, k)
        else:
            assert got[k].dtype == want[k].dtype and torch.equal(got[k], want[k]), (what, k)


def step(gpu, k=0, warm=0, factor=None, mods=None):
    """The reference's step pattern (client_part.py:112-133, server_part.py:45-57) on batch k."""
    client, server, crit = mods or fresh(gpu, warm)
    x, y = batches(gpu)[k]
    act = client(x)
    ca = _leaf(act)
    out = server(ca)
    loss = crit(out, y)
    (loss if factor is None else factor * loss).backward()
    act.backward(ca.grad.clone())
    return _snap((client, server), act=act, logits=out, loss=loss, cut=ca.grad)


def canon(gpu, k=0, warm=0):
    if (k, warm) not in _CACHE:
        _CACHE[(k, warm)] = step(gpu, k, warm)
    return _CACHE[(k, warm)]


def scaled(c, f, exact=("act", "logits", "loss")):
    return {k: v if (v is None or k in exact) else v * f for k, v in c.items()}


GRADS = ["grad_conv1.weight", "grad_conv1.bias", "grad_conv2.weight", "grad_conv2.bias", "grad_conv3.weight",
         "grad_conv3.bias", "grad_fc.weight", "grad_fc.bias"]


def test_canonical_step_is_reproducible(gpu):
    c = canon(gpu)
    assert c["act"].dtype == c["cut"].dtype == torch.bfloat16 and sorted(k for k in c if k.startswith("grad_")) \
        == sorted(GRADS)
    assert_bitwise(step(gpu), c)
    assert not torch.equal(canon(gpu, 0, warm=1)["logits"], c["logits"])      # another forward count, another mask


@pytest.mark.parametrize("factor", [0.5, 4.0])
def test_scaled_loss(gpu, factor):
    assert_bitwise(step(gpu, factor=factor), scaled(canon(gpu), factor))


def test_accumulation_over_two_backward_passes(gpu):
    mods = fresh(gpu)
    first = step(gpu, 0, mods=mods)
    both = step(gpu, 1, mods=mods)                    # no zero_grad; the second forward is forward count 1
    c0, c1 = canon(gpu, 0), canon(gpu, 1, warm=1)
    assert_bitwise(first, c0)
    assert_bitwise(both, {k: (c0[k] + c1[k]) if k in GRADS else c1[k] for k in c1})
    assert counter(mods[1]) == 2


def test_retain_graph_backward_twice(gpu):
    client, server, crit = fresh(gpu)
    x, y = batches(gpu)[0]
    act = client(x)
    ca = _leaf(act)
    out = server(ca)
    loss = crit(out, y)
    loss.backward(retain_graph=True)
    cut = ca.grad.clone()
    loss.backward()
    act.backward(cut, retain_graph=True)
    act.backward(cut)
    got = _snap((client, server), act=act, logits=out, loss=loss, cut=ca.grad)
    assert_bitwise(got, scaled(canon(gpu), 2.0))       # g + g


@pytest.mark.parametrize("case", ["fc", "cut"])
def test_frozen_head_and_cut_without_grad(gpu, case):
    client, server, crit = fresh(gpu)
    x, y = batches(gpu)[0]
    if case == "fc":
        for p in server.parameters():
            p.requires_grad_(False)
    act = client(x)
    ca = _leaf(act, grad=case != "cut")
    out = server(ca)
    loss = crit(out, y)
    want = dict(canon(gpu))
    if case == "fc":
        loss.backward()
        act.backward(ca.grad.clone())
        want["grad_fc.weight"] = want["grad_fc.bias"] = None
    else:
        loss.backward()
        for k in ["cut"] + GRADS[:6]:
            want[k] = None
    assert_bitwise(_snap((client, server), act=act, logits=out, loss=loss, cut=ca.grad), want)


@pytest.mark.parametrize("order", [(0, 1), (1, 0)])
def test_two_training_forwards_before_their_backward_passes(gpu, order):
    """Each backward uses its own forward's dropout mask (the counter snapshot of that forward), whichever
    runs first; the counter advances by exactly one per training forward."""
    client, server, crit = fresh(gpu)
    st = []
    for k in (0, 1):
        x, y = batches(gpu)[k]
        act = client(x)
        ca = _leaf(act)
        out = server(ca)
        assert counter(server) == k + 1
        st.append((act, ca, out, crit(out, y)))
    for k in order:
        act, ca, out, loss = st[k]
        loss.backward()
        act.backward(ca.grad.clone())
        got = _snap((client, server), act=act, logits=out, loss=loss, cut=ca.grad)
        assert_bitwise(got, canon(gpu, k, warm=k), f"batch {k}")
        client.zero_grad(set_to_none=True)
        server.zero_grad(set_to_none=True)
    assert counter(server) == 2


def test_counter_advances_only_in_training_forwards(gpu):
    client, server, _ = fresh(gpu)
    x, _y = batches(gpu)[0]
    with torch.no_grad():
        cut = client(x)
        server(cut)                                    # a training forward, under no_grad or not
        assert counter(server) == 1
        server.eval()
        e1 = server(cut)
        assert counter(server) == 1
    e2 = server(_leaf(cut))                            # eval mode with grad
    assert counter(server) == 1
    assert torch.equal(e1, e2)
    server.train()
    t1 = server(cut)
    assert counter(server) == 2
    assert torch.equal(t1, canon(gpu, 0, warm=1)["logits"]) and not torch.equal(t1, e1)


def test_full_model_eval_and_back_to_train(gpu):
    """WideFullModel.eval() reaches the shared head (no dropout, no tick): bitwise the split modules' eval
    output; back in .train() the counter continues."""
    from splitcnn.wide import WideFullModel
    x, _y = batches(gpu)[0]
    client, server, _ = fresh(gpu)
    server.eval()
    with torch.no_grad():
        want_eval = server(client(x))
    torch.manual_seed(0)
    full = WideFullModel().to(gpu)
    head = full._head[0]
    t0 = full(x)
    assert counter(head) == 1 and torch.equal(t0, canon(gpu, 0)["logits"])
    full.eval()
    with torch.no_grad():
        e = full(x)
    assert not head.training and counter(head) == 1
    assert torch.equal(e, want_eval)
    e_grad = full(x)                                   # eval mode with grad: the same, still no tick
    assert counter(head) == 1 and torch.equal(e_grad, want_eval)
    full.train()
    t1 = full(x)
    assert head.training and counter(head) == 2
    assert torch.equal(t1, canon(gpu, 0, warm=1)["logits"])


def test_float32_gradient_into_the_bf16_cut(gpu):
    c = canon(gpu)
    client, _server, _ = fresh(gpu)
    act = client(batches(gpu)[0][0])
    g = c["cut"]
    assert g.dtype == torch.bfloat16
    act.backward(g.float())
    assert_bitwise(_snap((client,)), {k: c[k] for k in GRADS[:6]})


def test_eval_mode_head_vs_oracle(gpu, monkeypatch):
    """Eval mode is Dropout(p = 0): oracle.wide_step.server_step at P_DROP = 0 with an all-ones keep mask, on
    the GPU's own cut. Bounds: wide_ref64.grad_close (1e-5 of the tensor's max) for the f32 logits, loss and
    fc gradients, wide_ref64.bf16_close for the bf16 cut gradient."""
    client, server, crit = fresh(gpu)
    x, y = batches(gpu)[0]
    with torch.no_grad():
        cut = client(x)
    server.eval()
    ca = _leaf(cut)
    out = server(ca)
    loss = crit(out, y)
    loss.backward()
    f64 = lambda t: t.detach().float().cpu().numpy().astype(np.float64)  # noqa: E731
    monkeypatch.setattr(W, "P_DROP", 0.0)
    P = {k: f64(v) for k, v in server.state_dict().items()}
    sv = W.server_step(P, f64(cut), y.cpu().numpy(), np.ones((B, W.CUT_F), dtype=bool))
    grad_close(f64(out), sv["logits"])
    grad_close(f64(loss), sv["loss"])
    bf16_close(f64(ca.grad), sv["dcut"])
    grad_close(f64(server.fc.weight.grad), sv["grads"]["fc.weight"])
    grad_close(f64(server.fc.bias.grad), sv["grads"]["fc.bias"])
    assert counter(server) == 0


def test_loud_failures(gpu):
    from splitcnn.wide import WideFullModel
    client, server, crit = fresh(gpu)
    x, y = batches(gpu)[0]
    xg = x.clone().requires_grad_(True)
    act = client(xg)
    with pytest.raises(NotImplementedError, match="input images"):
        act.backward(torch.ones_like(act))
    full = WideFullModel().to(gpu)
    loss = crit(full(xg), y)
    with pytest.raises(NotImplementedError, match="input images"):
        loss.backward()
    assert xg.grad is None
    # a cut of any other shape raises before the head's kernels and before the tick
    for shape in ((B, 256, 8, 7), (B, 128, 8, 8), (B, 256, 64), (B, 16384)):
        with pytest.raises(ValueError, match="expected \\[B,256,8,8\\]"):
            server(torch.zeros(shape, dtype=torch.bfloat16, device=gpu, requires_grad=True))
    assert counter(server) == 0
