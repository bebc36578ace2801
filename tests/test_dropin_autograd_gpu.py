"""The K2 drop-in modules (ModelPartA / ModelPartB / FullModel / CrossEntropyLoss, splitcnn/model_def.py and
library.py) under autograd use BEYOND the reference's step: scaled losses, gradient accumulation, two graphs
alive, one logits tensor scored twice, retain_graph, frozen parameters, inference between a forward and its
backward, non-contiguous layouts, a pooled map feeding two heads, and the loud failures.

Every pattern is ONE function, run on the GPU modules and, identically, on the float64 autograd reference
(tests/dropin_ref64.py), which pools by the kernel's own routing code (taken from ops.conv2_fwd_pool(impl="x3")
on the same inputs and held to float64 by ref64.assert_routing_ties at its default bounds). Bounds against
float64 are the project's (tests/test_gpu_parity.py): rel_err <= 1e-4 for logits and every gradient, 1e-5
relative for the loss.

Every pattern runs on three execution paths, whose results must be bit-identical: the default one (eager
autograd.Functions, library._MEMO by-products), library._Memo.take patched to always miss, and
library._EAGER = False (the torch.library custom ops). That is what catches a wrong memo hit (a wrong x3 scale
costs precision or overflows f16; it is not an O(1) error). Where autograd's own arithmetic makes a pattern a
known function of the canonical step (the reference's step pattern on fresh modules with the same seeds) the
result is also held to that, bit for bit: a power-of-two loss scale is exact in every kernel (the x3 scales are
powers of two, tests/test_x3_gpu.py::test_x3_dgrad_scale_invariance), an accumulated .grad is the f32 sum.

Batches: B = 3 and B = 17 (17 crosses the fc head's 16-sample workgroup; both are ragged for every tile)."""
import contextlib

import pytest
import torch

import dropin_ref64 as R
import ref64
from conftest import rel_err

pytestmark = pytest.mark.gpu

BATCHES = [3, 17]
PATHS = ("default", "nomemo", "customop")
SEED_MODEL, SEED_DATA = 6, 31


@contextlib.contextmanager
def path(mode):
    """One of the three execution paths of the drop-in ops."""
    from splitcnn import library
    take, eager = library._Memo.take, library._EAGER
    try:
        if mode == "nomemo":
            library._Memo.take = lambda self, kind, t: None
        elif mode == "customop":
            library._EAGER = False
        else:
            assert mode == "default"
        yield
    finally:
        library._Memo.take, library._EAGER = take, eager


# ------------------------------------------------------------------------------------------- data and models
class Data:
    """Two batches, a second label set for batch 0, the initial parameters and the kernels' routing codes of
    both batches at these parameters (never modified once built)."""

    def __init__(self, gpu, B):
        from splitcnn import ops
        from splitcnn.data import SyntheticMNIST, init_models
        self.gpu, self.B = gpu, B
        gen = SyntheticMNIST(SEED_DATA + B)
        self.cpu = [gen.batch(B), gen.batch(B)]
        self.alt_cpu = (self.cpu[0][1] + 3) % 10
        a, b = init_models(seed=SEED_MODEL)
        self.state = {k: v.clone() for k, v in {**a.state_dict(), **b.state_dict()}.items()}
        g = torch.Generator().manual_seed(B)
        self.head2 = (torch.randn(10, 9216, generator=g) * 0.01, torch.randn(10, generator=g) * 0.01)
        self.hook_w = torch.ones(B, 1)
        self.hook_w[0, 0], self.hook_w[1, 0] = 64.0, 2.0 ** -12
        sd = {k: v.to(gpu) for k, v in self.state.items()}
        self.codes = []
        for x, _y in self.cpu:
            act = ops.conv1_fwd(x.to(gpu), sd["conv1.weight"], sd["conv1.bias"])
            _, code = ops.conv2_fwd_pool(act, sd["conv2.weight"], sd["conv2.bias"], impl="x3",
                                         act_amax=ops.row_amax(act))
            ref64.assert_routing_ties(act, sd["conv2.weight"], sd["conv2.bias"], code)
            self.codes.append(code.cpu())


class GpuEnv:
    kind = "gpu"

    def __init__(self, d, mode="default"):
        from splitcnn.model_def import CrossEntropyLoss, FullModel, ModelPartA, ModelPartB
        self.d, self.mode, dev = d, mode, d.gpu
        self.client_m, self.server_m, self.full_m = ModelPartA(), ModelPartB(), FullModel()
        for m in self.modules():
            m.load_state_dict({k: v for k, v in d.state.items() if k in m.state_dict()})
            m.to(dev)
        self.crit = CrossEntropyLoss()
        self.batches = [(x.to(dev), y.to(dev)) for x, y in d.cpu]
        self.alt = d.alt_cpu.to(dev)

    def modules(self):
        return (self.client_m, self.server_m, self.full_m)

    def t(self, cpu_tensor, grad=False):
        return cpu_tensor.to(self.d.gpu).clone().requires_grad_(grad)

    def client(self, x):
        return self.client_m(x)

    def server(self, ca, k):
        return self.server_m(ca)

    def full(self, x, k):
        return self.full_m(x)

    # the ops themselves: the eager Functions, or torch.ops.splitcnn on the custom-op path
    def conv2(self, act, W2, b2, k):
        from splitcnn import library
        if self.mode == "customop":
            return torch.ops.splitcnn.conv2_relu_pool(act, W2, b2)[0]
        return library.Conv2ReluPoolFn.apply(act, W2, b2)[0]

    def linear(self, flat, W3, b3):
        from splitcnn import library
        if self.mode == "customop":
            return torch.ops.splitcnn.linear(flat, W3, b3)
        return library.LinearFn.apply(flat, W3, b3)

    def xent(self, logits, y):
        from splitcnn import library
        if self.mode == "customop":
            return torch.ops.splitcnn.cross_entropy(logits, y)
        return library.CrossEntropyFn.apply(logits, y)


class RefEnv:
    kind = "ref"

    def __init__(self, d, mode=None):
        self.d = d
        self.client_m, self.server_m, self.full_m = R.RefPartA(), R.RefPartB(), R.RefFull()
        for m in self.modules():
            R.load64(m, {k: v for k, v in d.state.items() if k in m.state_dict()})
        self.crit = R.cross_entropy
        self.batches = [(x.double(), y.clone()) for x, y in d.cpu]
        self.alt = d.alt_cpu.clone()

    modules = GpuEnv.modules

    def t(self, cpu_tensor, grad=False):
        t = cpu_tensor.clone()
        return (t.double() if t.is_floating_point() else t).requires_grad_(grad)

    def client(self, x):
        return self.client_m(x)

    def server(self, ca, k):
        return self.server_m(ca, self.d.codes[k])

    def full(self, x, k):
        return self.full_m(x, self.d.codes[k])

    def conv2(self, act, W2, b2, k):
        return R.pool_by_code(torch.relu(torch.nn.functional.conv2d(act, W2, b2)), self.d.codes[k])

    def linear(self, flat, W3, b3):
        return torch.nn.functional.linear(flat, W3, b3)

    def xent(self, logits, y):
        return R.cross_entropy(logits, y)


_DATA, _CANON = {}, {}


def data(gpu, B):
    if B not in _DATA:
        _DATA[B] = Data(gpu, B)
    return _DATA[B]


def canon(gpu, B, k=0, alt=False):
    """The canonical step of batch k (alt: batch 0 with the second label set) on the default path, computed
    once per batch size and shared."""
    key = (B, k, alt)
    if key not in _CANON:
        _CANON[key] = canonical(GpuEnv(data(gpu, B)), k=k, alt=alt)
    return _CANON[key]


# ------------------------------------------------------------------------------------------- bookkeeping
def _leaf(act):
    return act.clone().detach().requires_grad_(True)


def _val(v):
    return None if v is None else v.detach().clone()


def _snap(env, mods, sfx="", **tensors):
    out = {k + sfx: _val(v) for k, v in tensors.items()}
    for m in mods:
        for n, p in m.named_parameters():
            out["grad_" + n + sfx] = _val(p.grad)
    return out


def _zero(mods, *leaves):
    for m in mods:
        m.zero_grad(set_to_none=True)
    for t in leaves:
        t.grad = None


def assert_bitwise(got, want, what=""):
    assert got.keys() == want.keys(), (what, sorted(got), sorted(want))
    for k in want:
        if want[k] is None or got[k] is None:
            assert got[k] is None and want[k] is None, (what, k)
        else:
            assert got[k].dtype == want[k].dtype and torch.equal(got[k], want[k]), (what, k)


def assert_close64(got, want):
    assert got.keys() == want.keys(), (sorted(got), sorted(want))
    for k, w in want.items():
        g = got[k]
        if w is None or g is None:
            assert g is None and w is None, k
        elif k.startswith("loss"):
            err = abs(g.item() - w.item()) / abs(w.item())
            print(f"{k}: relative {err:.3g}")
            assert err <= 1e-5, (k, err)
        else:
            err = rel_err(g.double().cpu().numpy(), w.numpy())
            print(f"{k}: rel_err {err:.3g}")
            assert err <= 1e-4, (k, err)


def run(gpu, B, pattern, **kw):
    """pattern on the three execution paths (bit-identical) and on float64 (the project's bounds); returns the
    default path's result."""
    d = data(gpu, B)
    res = {}
    for mode in PATHS:
        with path(mode):
            res[mode] = pattern(GpuEnv(d, mode), **kw)
    for mode in PATHS[1:]:
        assert_bitwise(res[mode], res["default"], mode)
    assert_close64(res["default"], pattern(RefEnv(d), **kw))
    return res["default"]


def scaled(c, f, exact=("act", "logits", "loss")):
    return {k: v if (v is None or k in exact) else v * f for k, v in c.items()}


def summed(c0, c1, keys):
    return {k: c0[k] + c1[k] for k in keys}


def pick(res, sfx, like):
    """The entries of res named like `like`'s with suffix sfx, under like's names."""
    return {k: res[k + sfx] for k in like}


# ------------------------------------------------------------------------------------------- the patterns
def canonical(env, k=0, alt=False, factor=None):
    """The reference's step pattern (client_part.py:112-133, server_part.py:45-57), optionally with a scaled
    loss."""
    x, y = env.batches[k]
    y = env.alt if alt else y
    act = env.client(x)
    ca = _leaf(act)
    out = env.server(ca, k)
    loss = env.crit(out, y)
    (loss if factor is None else factor * loss).backward()
    act.backward(ca.grad.clone())
    return _snap(env, (env.client_m, env.server_m), act=act, logits=out, loss=loss, cut=ca.grad)


def accumulation(env):
    res = {}
    for k in (0, 1):
        x, y = env.batches[k]
        act = env.client(x)
        ca = _leaf(act)
        env.crit(env.server(ca, k), y).backward()
        act.backward(ca.grad.clone())
        res[f"cut_{k}"] = _val(ca.grad)
    return _snap(env, (env.client_m, env.server_m), **res)


def two_graphs(env, order):
    """Both forwards and losses first; then the backwards in `order` (each result recorded, grads cleared
    between), or order = "sum": (l0 + l1).backward() in one pass."""
    mods = (env.client_m, env.server_m)
    st = []
    for k in (0, 1):
        x, y = env.batches[k]
        act = env.client(x)
        ca = _leaf(act)
        out = env.server(ca, k)
        st.append((act, ca, out, env.crit(out, y)))
    res = {}
    if order == "sum":
        (st[0][3] + st[1][3]).backward()
        for k in (0, 1):
            act, ca, out, loss = st[k]
            act.backward(ca.grad.clone())
            res.update(_snap(env, (), f"_{k}", act=act, logits=out, loss=loss, cut=ca.grad))
        res.update(_snap(env, mods))
        return res
    for k in order:
        act, ca, out, loss = st[k]
        loss.backward()
        act.backward(ca.grad.clone())
        res.update(_snap(env, mods, f"_{k}", act=act, logits=out, loss=loss, cut=ca.grad))
        _zero(mods)
    return res


def two_label_sets(env):
    """la = crit(out, ya); lb = crit(out, yb); la.backward(retain_graph=True); lb.backward(): the memo holds
    yb's dlogits when ya's backward runs."""
    mods = (env.client_m, env.server_m)
    x, ya = env.batches[0]
    act = env.client(x)
    ca = _leaf(act)
    out = env.server(ca, 0)
    la = env.crit(out, ya)
    lb = env.crit(out, env.alt)
    la.backward(retain_graph=True)
    act.backward(ca.grad.clone(), retain_graph=True)
    res = _snap(env, mods, "_a", act=act, logits=out, loss=la, cut=ca.grad)
    _zero(mods, ca)
    lb.backward()
    act.backward(ca.grad.clone())
    res.update(_snap(env, mods, "_b", act=act, logits=out, loss=lb, cut=ca.grad))
    return res


def retain_twice(env):
    x, y = env.batches[0]
    act = env.client(x)
    ca = _leaf(act)
    out = env.server(ca, 0)
    loss = env.crit(out, y)
    loss.backward(retain_graph=True)
    cut = ca.grad.clone()
    loss.backward()                       # the second pass finds the memo consumed
    act.backward(cut, retain_graph=True)
    act.backward(cut)
    return _snap(env, (env.client_m, env.server_m), act=act, logits=out, loss=loss, cut=ca.grad)


FROZEN = {"conv2": ("conv2",), "fc1": ("fc1",), "server": ("conv2", "fc1"), "cut": ()}


def frozen(env, case):
    for name in FROZEN[case]:
        for p in getattr(env.server_m, name).parameters():
            p.requires_grad_(False)
    x, y = env.batches[0]
    act = env.client(x)
    ca = act.clone().detach().requires_grad_(case != "cut")
    out = env.server(ca, 0)
    loss = env.crit(out, y)
    loss.backward()
    if case != "cut":
        act.backward(ca.grad.clone())
    return _snap(env, (env.client_m, env.server_m), act=act, logits=out, loss=loss, cut=ca.grad)


def inference_between(env):
    (x, y), (xv, yv) = env.batches
    act = env.client(x)
    ca = _leaf(act)
    out = env.server(ca, 0)
    loss = env.crit(out, y)
    with torch.no_grad():
        av = env.client(xv)
        ov = env.server(av, 1)
        lv = env.crit(ov, yv)
    env.client_m.eval()
    env.server_m.eval()
    with torch.no_grad():
        oe = env.server(env.client(xv), 1)
    env.client_m.train()
    env.server_m.train()
    loss.backward()
    act.backward(ca.grad.clone())
    return _snap(env, (env.client_m, env.server_m), act=act, logits=out, loss=loss, cut=ca.grad,
                 act_v=av, logits_v=ov, loss_v=lv, logits_e=oe)


def heads(env, n, hook):
    """The ops themselves: one pooled map feeding n linear heads (autograd sums the heads' dflat before the
    conv2 backward, which must not take either head's memoized max |dflat|); with `hook`, a gradient hook that
    rescales dflat IN PLACE per sample (same storage, new version: the memoized max no longer describes it)."""
    d = env.d
    x, ya = env.batches[0]
    act = _leaf(env.client(x))
    P = {k: env.t(d.state[k], True) for k in ("conv2.weight", "conv2.bias", "fc1.weight", "fc1.bias")}
    flat = env.conv2(act, P["conv2.weight"], P["conv2.bias"], 0).view(d.B, 9216)
    if hook:
        w = env.t(d.hook_w)

        def rescale_in_place(g):
            g.mul_(w)

        flat.register_hook(rescale_in_place)
    loss = env.xent(env.linear(flat, P["fc1.weight"], P["fc1.bias"]), ya)
    if n == 2:
        P["head2.weight"], P["head2.bias"] = (env.t(t, True) for t in d.head2)
        loss = loss + env.xent(env.linear(flat, P["head2.weight"], P["head2.bias"]), env.alt)
    loss.backward()
    return {"loss": _val(loss), "cut": _val(act.grad), **{"grad_" + k: _val(p.grad) for k, p in P.items()}}


def full_model(env, case):
    m = (env.full_m,)
    res = {}
    if case.startswith("scaled"):
        x, y = env.batches[0]
        out = env.full(x, 0)
        loss = env.crit(out, y)
        (float(case[6:]) * loss).backward()
        return _snap(env, m, logits=out, loss=loss)
    if case == "accumulation":
        for k in (0, 1):
            x, y = env.batches[k]
            env.crit(env.full(x, k), y).backward()
        return _snap(env, m)
    st = []
    for k in (0, 1):
        x, y = env.batches[k]
        out = env.full(x, k)
        st.append((out, env.crit(out, y)))
    if case == "sum":
        (st[0][1] + st[1][1]).backward()
        return _snap(env, m)
    for k in (1, 0):
        st[k][1].backward()
        res.update(_snap(env, m, f"_{k}", logits=st[k][0], loss=st[k][1]))
        _zero(m)
    return res


GRADS = ["grad_conv1.weight", "grad_conv1.bias", "grad_conv2.weight", "grad_conv2.bias", "grad_fc1.weight",
         "grad_fc1.bias"]


# ------------------------------------------------------------------------------------------- the tests
@pytest.mark.parametrize("B", BATCHES)
def test_canonical_step_three_paths_vs_float64(gpu, B):
    got = run(gpu, B, canonical)
    assert_bitwise(got, canon(gpu, B))
    run(gpu, B, canonical, k=1)
    run(gpu, B, canonical, alt=True)


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("factor", [0.5, 4.0, 3.0])
def test_scaled_loss(gpu, B, factor):
    """(f * loss).backward(): every gradient is f times the canonical one; bit for bit at the powers of two
    (exact in every kernel), against float64 only at f = 3."""
    got = run(gpu, B, canonical, factor=factor)
    if factor != 3.0:
        assert_bitwise(got, scaled(canon(gpu, B), factor))


@pytest.mark.parametrize("B", BATCHES)
def test_accumulation_over_two_backward_passes(gpu, B):
    got = run(gpu, B, accumulation)
    c0, c1 = canon(gpu, B, 0), canon(gpu, B, 1)
    assert_bitwise(got, {"cut_0": c0["cut"], "cut_1": c1["cut"], **summed(c0, c1, GRADS)})


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("order", [(0, 1), (1, 0), "sum"])
def test_two_graphs_alive(gpu, B, order):
    got = run(gpu, B, two_graphs, order=order)
    c = [canon(gpu, B, 0), canon(gpu, B, 1)]
    for k in (0, 1):
        like = c[k] if order != "sum" else {n: c[k][n] for n in ("act", "logits", "loss", "cut")}
        assert_bitwise(pick(got, f"_{k}", like), like, f"batch {k}")
    if order == "sum":
        assert_bitwise({n: got[n] for n in GRADS}, summed(c[0], c[1], GRADS))


@pytest.mark.parametrize("B", BATCHES)
def test_one_logits_tensor_two_label_sets(gpu, B):
    got = run(gpu, B, two_label_sets)
    ca, cb = canon(gpu, B, 0), canon(gpu, B, 0, alt=True)
    assert not torch.equal(ca["cut"], cb["cut"])
    assert_bitwise(pick(got, "_a", ca), ca, "first label set")
    assert_bitwise(pick(got, "_b", cb), cb, "second label set")


@pytest.mark.parametrize("B", BATCHES)
def test_retain_graph_same_loss_backward_twice(gpu, B):
    got = run(gpu, B, retain_twice)
    assert_bitwise(got, scaled(canon(gpu, B), 2.0))       # g + g


@pytest.mark.parametrize("mode", PATHS)
def test_labels_edited_in_place_before_backward_raise(gpu, mode):
    """As torch does for any saved tensor (F.cross_entropy, or an autograd.Function that saves its labels):
    RuntimeError at backward, never a gradient from the forward's stale dlogits."""
    d = data(gpu, 3)
    with path(mode):
        env = GpuEnv(d, mode)
        x, y = env.batches[0]
        y = y.clone()
        ca = _leaf(env.client(x))
        loss = env.crit(env.server(ca, 0), y)
        y.add_(1).remainder_(10)
        with pytest.raises(RuntimeError, match="modified by an inplace operation"):
            loss.backward()
        assert ca.grad is None


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("case", sorted(FROZEN))
def test_frozen_parameters(gpu, B, case):
    """conv2 frozen; fc1 frozen; every server parameter frozen with a cut that requires grad; a cut that does
    not require grad with trainable parameters: the remaining gradients are the canonical ones, the absent
    ones None."""
    got = run(gpu, B, frozen, case=case)
    want = dict(canon(gpu, B))
    for name in FROZEN[case]:
        want[f"grad_{name}.weight"] = want[f"grad_{name}.bias"] = None
    if case == "cut":
        want["cut"] = want["grad_conv1.weight"] = want["grad_conv1.bias"] = None
    assert_bitwise(got, want)


@pytest.mark.parametrize("B", BATCHES)
def test_inference_between_a_forward_and_its_backward(gpu, B):
    got = run(gpu, B, inference_between)
    c0, c1 = canon(gpu, B, 0), canon(gpu, B, 1)
    assert_bitwise({k: got[k] for k in c0}, c0)
    assert_bitwise({k: got[k] for k in ("act_v", "logits_v", "loss_v", "logits_e")},
                   {"act_v": c1["act"], "logits_v": c1["logits"], "loss_v": c1["loss"], "logits_e": c1["logits"]})


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("mode", PATHS)
def test_layouts(gpu, B, mode):
    """A batch taken as big[::2], a channels-last cut leaf and labels taken as a strided slice: the values of
    the contiguous run bit for bit (ca.grad whatever its strides)."""
    d = data(gpu, B)
    with path(mode):
        env = GpuEnv(d, mode)
        x, y = env.batches[0]
        big = torch.full((2 * B, 1, 28, 28), 7.0, device=gpu)
        big[::2] = x
        ybig = torch.full((2 * B,), 9, dtype=torch.int64, device=gpu)
        ybig[::2] = y
        xs, ys = big[::2], ybig[::2]
        assert not xs.is_contiguous() and not ys.is_contiguous()
        act = env.client(xs)
        ca = act.detach().clone(memory_format=torch.channels_last).requires_grad_(True)
        assert not ca.is_contiguous()
        out = env.server(ca, 0)
        loss = env.crit(out, ys)
        loss.backward()
        act.backward(ca.grad.clone())
        got = _snap(env, (env.client_m, env.server_m), act=act, logits=out, loss=loss, cut=ca.grad)
    assert_bitwise(got, canon(gpu, B))


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("n,hook", [(2, False), (1, True), (1, False)])
def test_pooled_map_feeding_linear_heads(gpu, B, n, hook):
    got = run(gpu, B, heads, n=n, hook=hook)
    if (n, hook) == (1, False):   # the modules are these ops
        c = canon(gpu, B)
        assert_bitwise(got, {k: c[k] for k in got})


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("case", ["scaled0.5", "scaled4", "scaled3", "accumulation", "order", "sum"])
def test_full_model(gpu, B, case):
    """FullModel: gradients equal those of the split modules chained by hand, bit for bit."""
    got = run(gpu, B, full_model, case=case)
    c0, c1 = canon(gpu, B, 0), canon(gpu, B, 1)
    if case.startswith("scaled"):
        f = float(case[6:])
        if f != 3.0:
            assert_bitwise(got, scaled({k: c0[k] for k in got}, f))
    elif case in ("accumulation", "sum"):
        assert_bitwise(got, summed(c0, c1, GRADS))
    else:
        for k, c in ((0, c0), (1, c1)):
            like = {n: c[n] for n in ["logits", "loss"] + GRADS}
            assert_bitwise(pick(got, f"_{k}", like), like, f"batch {k}")


# ------------------------------------------------------------------------------------------- loud failures
@pytest.mark.parametrize("mode", ["default", "customop"])
def test_input_gradient_raises_at_backward(gpu, mode):
    """The client's input gradient is not part of the split step: asking for it raises the documented
    NotImplementedError at backward (never a silent None)."""
    with path(mode):
        env = GpuEnv(data(gpu, 3), mode)
        x, y = env.batches[0]
        x = x.clone().requires_grad_(True)
        act = env.client(x)
        with pytest.raises(NotImplementedError, match="INPUT images"):
            act.backward(torch.ones_like(act))
        loss = env.crit(env.full(x, 0), y)
        with pytest.raises(NotImplementedError, match="INPUT images"):
            loss.backward()
        assert x.grad is None


@pytest.mark.parametrize("mode", ["default", "customop"])
def test_wrong_dtype_or_shape_raises_before_any_launch(gpu, mode):
    """ops._dev / ops.batch_of check dtype and shape before _lib.call: nothing here reaches a kernel."""
    with path(mode):
        env = GpuEnv(data(gpu, 3), mode)
        x, y = env.batches[0]
        with torch.no_grad():
            act = env.client(x)
            out = env.server(act, 0)
        for bad in (act.double(), act.half()):
            with pytest.raises(TypeError, match="expected torch.float32"):
                env.server(bad.requires_grad_(True), 0)
        for shape in ((3, 32, 26, 25), (3, 16, 26, 26), (3, 32, 26), (3, 32 * 26 * 26)):
            with pytest.raises(ValueError, match="expected shape"):
                env.server(torch.zeros(shape, device=gpu, requires_grad=True), 0)
        with pytest.raises(TypeError, match="expected torch.int64"):
            env.crit(out.clone().requires_grad_(True), y.int())
        with pytest.raises(ValueError, match="expected shape"):
            env.crit(out.clone().requires_grad_(True), y[:2])


@pytest.mark.parametrize("bad", [-100, -1, 10])
def test_labels_outside_the_classes_give_a_non_finite_loss(gpu, bad):
    """Unlike torch (IndexError, and ignore_index = -100 skipped), a label outside [0, 10) makes the mean loss
    NaN: the kernel writes NaN for such rows ("Supported autograd usage")."""
    env = GpuEnv(data(gpu, 3))
    x, y = env.batches[0]
    with torch.no_grad():
        out = env.server(env.client(x), 0)
        assert torch.isfinite(env.crit(out, y))
        y = y.clone()
        y[1] = bad
        assert not torch.isfinite(env.crit(out, y))
