"""CPU: tests/nonfinite_ref.py — the non-finite rule of include/slk.h as the GPU tests use it — pinned without a device.

  * the poison table covers what it says it covers;
  * predict()'s IEEE value equals plain elementwise float64 arithmetic on the poisoned operands;
  * rule_* and torch_* (F.conv2d / F.relu / F.max_pool2d in float64) differ exactly where clause 2 says: where the
    pre-activation is NaN (ReLU) and in the windows that hold one (pool) — nowhere else, a -inf included;
  * three wrong kernels are visible on the table: a NaN-propagating ReLU / pool, a multiplying mask, a NaN-counting
    maximum each give a pattern different from the rule's on at least one entry of every kernel family they touch;
  * must(P) is non-empty for every (family, operand, entry) the GPU tests use with it.
"""
import math

import pytest
import torch
import torch.nn.functional as F

import head_ref64 as R
import nonfinite_ref as N
from ref64 import route64
from test_x3_exact_gpu import _exact_case

B = 3
IDS = [e.name for e in N.TABLE]


@pytest.fixture(scope="module")
def k2():
    c = _exact_case("cpu", B, seed=7400 + B)
    x, W1, b1 = R.conv1_int_case(B, 7000 + B)
    return dict(c, x1=x, W1=W1, b1=b1, g=R.cut_grad_int(B, 7300 + B))


def test_table_covers_values_samples_pixels_channels():
    assert len(N.TABLE) == 9 and len({e.name for e in N.TABLE}) == 9
    for vals in (N.NAN_ENTRIES, N.PINF_ENTRIES, [e for e in N.TABLE if e.value == -N.INF]):
        assert {e.sample for e in vals} == {"first", "mid", "last"}
        assert {e.pixel for e in vals} == {"first", "last", "inner"}
        assert {e.channel for e in vals} == {"first", "last"}
    assert {(e.sample, e.pixel) for e in N.TABLE} == {(s, p) for s in ("first", "mid", "last")
                                                      for p in ("first", "last", "inner")}
    e = N.TABLE[2]   # nan-last-last-first
    assert N.place(e, (5, 32, 26, 26)) == (4, 0, 25, 25)
    assert N.place(e, (64, 32, 3, 3), batched=False) == (0, 31, 2, 2)
    assert N.place(e, (64,), batched=False) == (0,)
    assert N.place(N.TABLE[1], (5, 9216)) == (2, 0) and N.place(N.TABLE[1], (10, 9216), batched=False) == (9, 0)


@pytest.mark.parametrize("entry", N.TABLE, ids=IDS)
def test_predict_is_elementwise_ieee(k2, entry):
    """conv1's pre-activation by predict() == head_ref64.conv1_pre (shifted elementwise products, no BLAS) on the
    poisoned operands, NaN for NaN and infinity for infinity, for a poison in x and in W1."""
    x, W1, b1 = k2["x1"], k2["W1"], k2["b1"]
    for slot, t in ((0, x), (1, W1)):
        idx = N.place(entry, t.shape, batched=slot == 0)
        p = N.predict(N.conv1_lin, x, W1, slot, idx, entry.value)
        ops = [x.clone(), W1.clone()]
        ops[slot][idx] = entry.value
        want = R.conv1_pre(ops[0], ops[1], torch.zeros(32, dtype=torch.float64))
        assert torch.equal(torch.isnan(p.want), torch.isnan(want))
        assert torch.equal(torch.nan_to_num(p.want, nan=0.0), torch.nan_to_num(want, nan=0.0))
        assert torch.equal(N.nonfinite(p.want), p.may) and bool((p.must <= p.may).all()) and p.must.any()
        assert torch.equal(p.clean[~p.may], want[~p.may])


@pytest.mark.parametrize("entry", N.TABLE, ids=IDS)
def test_rule_and_torch_differ_exactly_at_nan(k2, entry):
    """conv1 + ReLU and conv2 + ReLU + pool with the poison in the input: torch's output is NaN exactly where IEEE's
    pre-activation is NaN (ReLU) or the window holds such a pixel (pool), where the rule writes +0 or the maximum of
    the window's other positive values; everywhere else, -inf and +inf included, the two are equal."""
    x, W1, b1 = k2["x1"], k2["W1"], k2["b1"]
    idx = N.place(entry, x.shape)
    pre = N.predict(N.conv1_lin, x, W1, 0, idx, entry.value).want + b1[None, :, None, None]
    t = F.relu(F.conv2d(N.plant(x, idx, entry.value), W1, b1))
    r = N.rule_relu(pre)
    assert torch.equal(torch.isnan(t), torch.isnan(pre)) and not torch.isnan(r).any()
    assert torch.equal(t[~torch.isnan(pre)], r[~torch.isnan(pre)])
    assert bool((r[torch.isnan(pre)] == 0).all())
    act, W2, b2 = k2["act"].double(), k2["W2"].double(), k2["b2"].double()
    idx = N.place(entry, act.shape)
    pre = N.predict(N.conv2_lin, act, W2, 0, idx, entry.value).want + b2[None, :, None, None]
    t = N.torch_pool(F.conv2d(N.plant(act, idx, entry.value), W2, b2))
    r, code = N.rule_pool(pre)
    holds_nan = F.max_pool2d(torch.isnan(pre).double(), 2) > 0
    assert torch.equal(torch.isnan(t), holds_nan) and not torch.isnan(r).any()
    assert torch.equal(t[~holds_nan], r[~holds_nan])
    assert bool((code <= N.CODE_NONE).all()) and torch.equal(code == N.CODE_NONE, r == 0)
    if math.isnan(entry.value):
        assert holds_nan.any() and bool((r[holds_nan] > 0).any())      # the rule keeps the window's other values
    elif entry.value > 0:
        assert bool(torch.isinf(r).any())                                # a +inf is kept, its code is its index
    wn, cn = N.nanpropagating_pool(pre)                                  # wrong variant 1 is visible where torch is
    assert torch.equal(torch.isnan(wn), holds_nan)


def _families(k2, entry):
    """(family, operand) -> Pred for the K2 families whose prediction passes a select or a maximum."""
    act, W2, dp, code = k2["act"].double(), k2["W2"].double(), k2["dp"].double(), k2["code"].clone()
    out = {}
    idx = N.place(entry, dp.shape)
    for tag, cd in (("routed", 2), ("blocked", N.CODE_NONE)):
        c = code.clone()
        c[idx] = cd
        dc = route64(dp, c)
        out["dgrad", tag] = (N.predict(N.conv2_dgrad_lin, dc, W2, 0, N.routed_index(idx, c), entry.value), c)
        out["wgrad", tag] = (N.predict(N.conv2_wgrad_lin, act, dc, 1, N.routed_index(idx, c), entry.value), c)
    return out, idx


@pytest.mark.parametrize("entry", N.TABLE, ids=IDS)
def test_multiplying_mask_is_visible(k2, entry):
    """Wrong variant 2: routing by multiplication lets a poison under CODE_NONE through (clause 5 forbids it) and
    spreads a routed one over its window. Its pattern differs from the rule's in both backward families on every
    entry; the same holds for conv1's ReLU mask."""
    fam, idx = _families(k2, entry)
    dp, W2, act = k2["dp"].double(), k2["W2"].double(), k2["act"].double()
    for tag in ("routed", "blocked"):
        pred, c = fam["dgrad", tag]
        wrong = N.route_multiply(N.plant(dp, idx, entry.value), c)
        nf = N.nonfinite(wrong)
        assert int(nf.sum()) == 4                                       # the whole window, whatever the code
        reach = N.conv2_dgrad_lin(nf.double(), torch.ones_like(W2)) != 0
        assert not torch.equal(reach, pred.may)
        # a weight gradient's columns are whole output channels: there the wrong routing shows under CODE_NONE only
        same_w = torch.equal(N.conv2_wgrad_lin(torch.ones_like(act), nf.double()) != 0, fam["wgrad", tag][0].may)
        assert same_w == (tag == "routed")
        if tag == "blocked":
            assert not pred.may.any() and not fam["wgrad", tag][0].may.any()
        else:
            assert pred.must.any() and fam["wgrad", tag][0].must.any()
    x, W1, b1, g = k2["x1"], k2["W1"], k2["b1"], k2["g"]
    act1 = R.conv1_relu(x, W1, b1)
    gi = N.place(entry, g.shape)
    blocked = (act1[gi[0], gi[1]] <= 0).nonzero()[0].tolist()
    gi = (gi[0], gi[1]) + tuple(blocked)
    gp = N.plant(g, gi, entry.value)
    rule = N.conv1_wgrad_lin(x, torch.where(act1 > 0, gp, torch.zeros_like(gp)))
    assert torch.isfinite(rule).all()
    assert not torch.isfinite(gp * (act1 > 0).double()).all()


@pytest.mark.parametrize("entry", N.NAN_ENTRIES, ids=[e.name for e in N.NAN_ENTRIES])
def test_nan_counting_maximum_is_visible(k2, entry):
    """Wrong variant 3: a per-sample maximum that returns NaN for a row holding one would make the x3 scale of the whole
    sample NaN, so every output of the sample non-finite; the rule keeps the sample's clean outputs."""
    act, dp = k2["act"].double(), k2["dp"].double()
    for t in (act, dp):
        idx = N.place(entry, t.shape)
        bad = N.plant(t, idx, entry.value)
        good, wrong = N.amax_ignoring_nan(bad), N.amax_counting_nan(bad)
        assert torch.isfinite(good).all() and torch.equal(good, N.amax_ignoring_nan(N.plant(t, idx, 0.0)))
        assert torch.isnan(wrong[idx[0]]) and int(torch.isnan(wrong).sum()) == 1
    idx = N.place(entry, act.shape)
    p = N.predict(N.conv2_lin, act, k2["W2"], 0, idx, entry.value)
    assert not p.may[idx[0]].all()          # the rule leaves clean outputs in the sample; the wrong maximum leaves none
    for v in (N.INF, -N.INF):
        assert torch.isinf(N.amax_ignoring_nan(N.plant(act, idx, v))[idx[0]])   # an infinity is kept (clause 3)


@pytest.mark.parametrize("entry", N.TABLE, ids=IDS)
def test_must_is_not_empty_where_the_gpu_tests_need_it(k2, entry):
    """Every (family, operand, entry) the GPU tests assert `must(P).any()` for: forwards (act, W2), dgrad (routed dp,
    W2), wgrad (act meeting a routed gradient, routed dp), fc (every operand). The +inf entries of the forwards are
    among them."""
    act, W2, dp, code = k2["act"].double(), k2["W2"].double(), k2["dp"].double(), k2["code"]
    for slot, t in ((0, act), (1, W2)):
        p = N.predict(N.conv2_lin, act, W2, slot, N.place(entry, t.shape, batched=slot == 0), entry.value)
        assert p.must.any() and bool((p.must <= p.may).all())
    fam, _ = _families(k2, entry)
    assert fam["dgrad", "routed"][0].must.any() and fam["wgrad", "routed"][0].must.any()
    dc = route64(dp, code)
    p = N.predict(N.conv2_dgrad_lin, dc, W2, 1, N.place(entry, W2.shape, batched=False), entry.value)
    assert p.must.any()
    pooled, W3, b3 = R.fc_int_case(B, 7900 + B)
    dl = R.dlogits_int(B, 7901 + B)
    for op, a, b_ in ((N.fc_lin, pooled, W3), (N.fc_dgrad_lin, dl, W3), (N.fc_wgrad_lin, dl, pooled)):
        for slot, t in ((0, a), (1, b_)):
            batched = t.shape[0] == B
            assert N.predict(op, a, b_, slot, N.place(entry, t.shape, batched=batched), entry.value).must.any()


def test_x3_pool_first_position_rule():
    """x3_pool: a NaN in the window's first position gives +0 / CODE_NONE, elsewhere it is skipped; on finite values it
    is rule_pool(raw + bias); x3_value turns an infinity into NaN and keeps everything else."""
    raw = torch.zeros(1, 64, 24, 24, dtype=torch.float64)
    raw[0, 0, 0, 0:2] = torch.tensor([N.NAN, 5.0])
    raw[0, 0, 2, 0:2] = torch.tensor([5.0, N.NAN])
    raw[0, 1, 0, 0:2] = torch.tensor([1.0, 7.0])
    b = torch.zeros(64, dtype=torch.float64)
    p, c = N.x3_pool(raw, b)
    assert p[0, 0, 0, 0] == 0 and c[0, 0, 0, 0] == N.CODE_NONE
    assert p[0, 0, 1, 0] == 5 and c[0, 0, 1, 0] == 0
    assert p[0, 1, 0, 0] == 7 and c[0, 1, 0, 0] == 1
    g = torch.Generator().manual_seed(1)
    raw = torch.randint(-9, 10, (2, 64, 24, 24), generator=g).double()
    b = torch.randint(-3, 4, (64,), generator=g).double()
    pr, cr = N.rule_pool(raw + b[None, :, None, None])
    p, c = N.x3_pool(raw, b)
    assert torch.equal(p, pr) and torch.equal(c, cr)
    assert math.isnan(N.x3_value(N.INF)) and math.isnan(N.x3_value(-N.INF)) and N.x3_value(3.0) == 3.0


# ----------------------------------------------------------------------------- step level
HIDDEN = {"x-nan", "x-pinf", "conv1.weight-nan", "conv1.bias-nan", "conv2.weight-nan", "conv2.bias-nan"}
# the tensors holding a non-finite value after EVERY one of the three steps under the rule (both presets)
RULE_BAD = {
    "clean": set(), "x-nan": {"conv1.weight"}, "x-pinf": {"conv1.weight", "conv2.weight"},
    "conv1.weight-nan": {"conv1.weight"}, "conv1.bias-nan": {"conv1.bias"},
    "conv2.weight-nan": {"conv2.weight", "conv1.weight", "conv1.bias"}, "conv2.bias-nan": {"conv2.bias"},
    "fc1.weight-nan": set(N.K2_TENSORS), "fc1.bias-nan": set(N.K2_TENSORS), "fc1.weight-pinf": set(N.K2_TENSORS),
}


@pytest.mark.parametrize("preset", ["x3", "f32"])
@pytest.mark.parametrize("scenario", list(N.SCENARIOS))
def test_step_table_rule_against_torch(scenario, preset):
    """Three plain-SGD steps of the reference model at the B = 4 fixture's inputs with the poison planted before step 1:
    torch logs NaN in step 1 of every poisoned scenario and leaves all six tensors NaN; under the rule the six HIDDEN
    scenarios log a finite loss in all three steps and keep the NaN in the tensors listed in RULE_BAD; a poison in fc1
    is reported by both. (tests/test_nonfinite_trainer_gpu.py holds SplitTrainer to the rule's column.)"""
    from conftest import load_fixture
    fx = load_fixture("split_step_b4.npz")
    params = {k: torch.from_numpy(fx["init_" + k]).clone() for k in N.K2_KEYS.values()}
    x, y = torch.from_numpy(fx["x_1"]).clone(), torch.from_numpy(fx["y_1"])
    name, v = N.SCENARIOS[scenario]
    xb = x.clone()
    if name == "x":
        xb[N.scenario_index("x", x.shape)] = v
    elif name is not None:
        params[N.K2_KEYS[name]][N.scenario_index(name, params[N.K2_KEYS[name]].shape)] = v
    batches = [(xb, y), (x, y), (x, y)]
    rule, _ = N.k2_steps(params, batches, preset=preset, rule=True)
    ref, _ = N.k2_steps(params, batches, preset=preset, rule=False)
    for r, t in zip(rule, ref):
        assert r["bad"] == RULE_BAD[scenario]
        if scenario == "clean":
            assert math.isfinite(r["loss"]) and math.isfinite(t["loss"]) and not t["bad"]
            assert abs(r["loss"] - t["loss"]) <= 1e-12 * abs(t["loss"])       # on finite values the rule IS torch
        else:
            assert math.isnan(t["loss"]) and t["bad"] == set(N.K2_TENSORS)     # the reference reports it in step 1
            assert math.isfinite(r["loss"]) == (scenario in HIDDEN)            # the rule hides these six


def test_clipped_step_model_spoils_the_whole_client():
    from conftest import load_fixture
    fx = load_fixture("split_step_b4.npz")
    params = {k: torch.from_numpy(fx["init_" + k]).clone() for k in N.K2_KEYS.values()}
    params["W2"][N.scenario_index("conv2.weight", params["W2"].shape)] = N.NAN
    batches = [(torch.from_numpy(fx["x_1"]), torch.from_numpy(fx["y_1"]))] * 2
    clip, _ = N.k2_steps(params, batches, rule=True, clip=1.0)
    plain, _ = N.k2_steps(params, batches, rule=True)
    assert clip[0]["whole"] == {"conv1.weight", "conv1.bias"} and plain[0]["whole"] == set()
    assert clip[0]["bad"] == plain[0]["bad"] == {"conv2.weight", "conv1.weight", "conv1.bias"}


@pytest.mark.parametrize("scenario", ["clean", "x-nan", "conv2.weight-nan", "conv3.bias-nan", "fc.weight-nan", "fc.weight-pinf"])
def test_k5_step_model_rule_against_torch(scenario):
    """One Adam step of the widened model at B = 2 (the model is the same function at B = 8; the CPU pays for float64
    convolutions): torch logs NaN for every poison; under the rule a poison below the head is hidden (finite loss, the
    poisoned tensor stays non-finite) and a poison in fc is reported."""
    from splitcnn.wide import SyntheticCIFAR, init_wide_models
    a, b = init_wide_models(seed=0)
    params = {k: t.detach().clone().double() for k, t in {**a.state_dict(), **b.state_dict()}.items()}
    x, y = SyntheticCIFAR(91).batch(2)
    name, v = N.K5_SCENARIOS[scenario]
    if name == "x":
        x[N.scenario_index("x", x.shape)] = v
    elif name is not None:
        params[name][N.scenario_index(name, params[name].shape)] = v
    (r,), (t,) = N.k5_steps(params, [(x, y)], rule=True), N.k5_steps(params, [(x, y)], rule=False)
    if scenario == "clean":
        assert not r["bad"] and not t["bad"] and abs(r["loss"] - t["loss"]) <= 1e-12 * abs(t["loss"])
        return
    assert math.isnan(t["loss"]) and t["bad"] == set(N.K5_TENSORS)
    assert math.isfinite(r["loss"]) == (not scenario.startswith("fc."))
    assert (name in r["bad"]) if name != "x" else ("conv1.weight" in r["bad"])
