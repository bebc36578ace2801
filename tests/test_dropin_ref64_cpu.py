"""CPU pin of tests/dropin_ref64.py, the float64 autograd reference of the drop-in usage tests: with
float64's own routing code the gather-pool is F.max_pool2d exactly (logits and all six parameter gradients,
difference 0.0), and it reproduces the reference's golden fixtures within the bounds tests/test_gpu_parity.py
holds the kernels to (act 1e-5, logits / cut gradient 1e-4 of the tensor's max, loss 1e-5 relative, post-step
weights by weight_ok)."""
import pytest
import torch

import dropin_ref64 as R
import ref64
from conftest import PARAMS, load_fixture, rel_err, weight_ok

KEYS = {"W1": "conv1.weight", "b1": "conv1.bias", "W2": "conv2.weight", "b2": "conv2.bias",
        "W3": "fc1.weight", "b3": "fc1.bias"}


def _models(fx):
    a = R.load64(R.RefPartA(), {KEYS[k]: fx[f"init_{k}"] for k in ("W1", "b1")})
    b = R.load64(R.RefPartB(), {KEYS[k]: fx[f"init_{k}"] for k in ("W2", "b2", "W3", "b3")})
    return a, b


def _step(a, b, x, y, code_of):
    """The reference's step (client_part.py:112-133, server_part.py:45-57) without the optimizers."""
    act = a(x)
    ca = act.clone().detach().requires_grad_(True)
    out = b(ca, code_of(ca))
    loss = R.cross_entropy(out, y)
    loss.backward()
    act.backward(ca.grad.clone())
    return act, out, loss, ca.grad


def _own_code(b):
    def code_of(ca):
        with torch.no_grad():
            return ref64.routing64(R.conv2_relu(ca, b.conv2))[0]
    return code_of


@pytest.mark.parametrize("B", [3, 7])
def test_pool_by_code_is_max_pool2d_at_float64s_own_code(B):
    from splitcnn.data import SyntheticMNIST
    x, y = SyntheticMNIST(5).batch(B)
    x = x.double()
    torch.manual_seed(3)
    got_m = (R.RefPartA(), R.RefPartB())
    want_m = (R.RefPartA(), R.RefPartB())
    for g, w in zip(got_m, want_m):
        w.load_state_dict(g.state_dict())
    got = _step(*got_m, x, y, _own_code(got_m[1]))
    want = _step(*want_m, x, y, lambda ca: None)          # code None: F.max_pool2d
    for g, w in zip(got, want):
        assert (g - w).abs().max().item() == 0.0
    gp = [p.grad for m in got_m for p in m.parameters()]
    wp = [p.grad for m in want_m for p in m.parameters()]
    assert len(gp) == 6
    for g, w in zip(gp, wp):
        assert g.abs().max().item() > 0 and (g - w).abs().max().item() == 0.0
    # the unsplit module is the two halves chained
    full = R.load64(R.RefFull(), *want_m)
    with torch.no_grad():
        code = ref64.routing64(R.conv2_relu(want[0], full.conv2))[0]
    loss = R.cross_entropy(full(x, code), y)
    loss.backward()
    assert (loss - want[2]).abs().item() == 0.0
    for name, p in full.named_parameters():
        mod, attr = name.split(".")
        half = want_m[0] if mod == "conv1" else want_m[1]
        assert (p.grad - getattr(getattr(half, mod), attr).grad).abs().max().item() == 0.0, name


@pytest.mark.parametrize("name", ["split_step_b4.npz", "split_step_b13.npz"])
def test_helper_reproduces_the_reference_fixture(name):
    fx = load_fixture(name)
    a, b = _models(fx)
    x = torch.from_numpy(fx["x_1"]).double()
    y = torch.from_numpy(fx["y_1"])
    act, out, loss, cut = _step(a, b, x, y, _own_code(b))
    assert rel_err(act.detach().numpy(), fx["act_1"]) <= 1e-5
    assert rel_err(out.detach().numpy(), fx["logits_1"]) <= 1e-4
    assert abs(loss.item() - float(fx["loss_1"])) <= 1e-5 * abs(float(fx["loss_1"]))
    assert rel_err(cut.numpy(), fx["cut_grad_1"]) <= 1e-4
    params = {**dict(a.named_parameters()), **dict(b.named_parameters())}
    for k in PARAMS:
        p = params[KEYS[k]]
        assert rel_err(p.grad.numpy(), fx[f"grad_{k}_1"]) <= 1e-4, k
        post = (p.detach() - 0.01 * p.grad).numpy()      # SGD(lr=0.01), client_part.py:105 / server_part.py:17
        assert weight_ok(post, fx[f"post_{k}_1"], fx[f"init_{k}"]), k
