"""GPU: what reaches the logged loss, and which parameters, when ONE value of a K2 SplitTrainer step is NaN or +inf — the
step-level face of the non-finite rule (include/slk.h "NaN and +-inf"), predicted by tests/nonfinite_ref.py's float64
model (k2_steps with rule=True: clause 2's selects, clause 3 for the x3 preset) and compared with plain torch
(rule=False), which tests/test_nonfinite_ref_cpu.py pins.

Three plain-SGD steps, one poison planted before step 1 (in a parameter, or in step 1's batch), on the B = 4 fixture's
inputs and on a B = 8 synthetic batch, for the default x3 preset and conv="f32", eager and graphed. The table the model
gives, and the GPU reproduces (F = the logged loss is finite, N = it is NaN; then the parameter tensors that hold a
non-finite value after the step; identical for the three steps, for both presets and both batches):

  scenario              torch (the reference)      this project (the rule)
  x pixel NaN           N at step 1, all six       F, F, F   conv1.weight               HIDDEN
  x pixel +inf          N at step 1, all six       F, F, F   conv1.weight, conv2.weight HIDDEN
  conv1.weight NaN      N at step 1, all six       F, F, F   conv1.weight               HIDDEN
  conv1.bias NaN        N at step 1, all six       F, F, F   conv1.bias                 HIDDEN
  conv2.weight NaN      N at step 1, all six       F, F, F   conv2.weight, conv1.weight, conv1.bias (from step 1)  HIDDEN
  conv2.bias NaN        N at step 1, all six       F, F, F   conv2.bias                 HIDDEN
  fc1.weight NaN        N at step 1, all six       N, N, N   all six                    reported
  fc1.bias NaN          N at step 1, all six       N, N, N   all six                    reported
  fc1.weight +inf       N at step 1, all six       N, N, N   all six                    reported

In the six HIDDEN scenarios the reference logs NaN in the first step and this project logs a finite loss for good:
clause 2 writes +0 for the NaN pre-activation, the channel goes dark and no gradient reaches the poisoned element. A
poisoned pixel does reach conv1.weight (the client's weight gradient forms 0 x NaN, clause 1), a poisoned conv2 weight
reaches conv1 through the cut gradient (0 x NaN again). check_finite() raises in exactly the scenarios and from exactly
the step where a parameter is non-finite, and names those tensors; it stays silent on a clean run. evaluate() on the
poisoned model reports a finite loss in the hidden parameter scenarios. Under optim.ClipNorm the stage whose gradient
holds a NaN goes wholly NaN (a NaN norm keeps a NaN coefficient), where plain SGD spoils single channels.

The second half of the file does the same for WideTrainer (K5, B = 8, three Adam steps, the dropout masks of those
steps) against nonfinite_ref.k5_steps; its table is in test_wide_trainer_steps' docstring.
"""
import math

import pytest
import torch

import nonfinite_ref as N
from conftest import load_fixture

pytestmark = pytest.mark.gpu

HIDDEN = {"x-nan", "x-pinf", "conv1.weight-nan", "conv1.bias-nan", "conv2.weight-nan", "conv2.bias-nan"}
REPORTED = {"fc1.weight-nan", "fc1.bias-nan", "fc1.weight-pinf"}


def _case(batch):
    """(params float32 by key, x, y) on the CPU: the fixture's weights; its B = 4 inputs or a synthetic B = 8 batch."""
    fx = load_fixture("split_step_b4.npz")
    params = {k: torch.from_numpy(fx["init_" + k]).clone() for k in N.K2_KEYS.values()}
    if batch == "fixture":
        return params, torch.from_numpy(fx["x_1"]).clone(), torch.from_numpy(fx["y_1"]).clone()
    from splitcnn.data import SyntheticMNIST
    x, y = SyntheticMNIST(77).batch(8)
    return params, x.clone(), y.clone()


def _poison(params, x, scenario):
    name, v = N.SCENARIOS[scenario]
    params, xb = {k: t.clone() for k, t in params.items()}, x.clone()
    if name == "x":
        xb[N.scenario_index("x", xb.shape)] = v
    elif name is not None:
        k = N.K2_KEYS[name]
        params[k][N.scenario_index(name, params[k].shape)] = v
    return params, xb


def _trainer(gpu, params, conv, graph, clip=None):
    from splitcnn.engine import SplitTrainer
    from splitcnn.model_def import ModelPartA, ModelPartB
    a, b = ModelPartA(), ModelPartB()
    a.load_state_dict({"conv1.weight": params["W1"], "conv1.bias": params["b1"]})
    b.load_state_dict({"conv2.weight": params["W2"], "conv2.bias": params["b2"], "fc1.weight": params["W3"],
                       "fc1.bias": params["b3"]})
    return SplitTrainer(a, b, device=gpu, graph=graph, conv=conv, clip=clip)


def _bad_tensors(tr):
    sd = {**tr.client.model.state_dict(), **tr.server.model.state_dict()}
    return {t for t in N.K2_TENSORS if not torch.isfinite(sd[t]).all()}, \
        {t for t in N.K2_TENSORS if not torch.isfinite(sd[t]).any()}


def _raised(tr):
    """The tensors check_finite() names, or None when it does not raise."""
    try:
        tr.check_finite()
    except FloatingPointError as e:
        msg = str(e)
        return {t for t in N.K2_TENSORS if f"{'client' if t.startswith('conv1') else 'server'}.{t}" in msg}
    return None


def _run(gpu, params, batches, conv, graph, clip=None):
    """Three steps -> per-step records (loss, bad, whole, raised) and the final parameter bits."""
    tr = _trainer(gpu, params, conv, graph, clip)
    recs = []
    for x, y in batches:
        tr.step(x.to(gpu), y.to(gpu))
        torch.cuda.synchronize()
        bad, whole = _bad_tensors(tr)
        recs.append(dict(bad=bad, whole=whole, raised=_raised(tr)))
    for r, (_, loss) in zip(recs, tr.loss_log.flush()):
        r["loss"] = loss
    bits = torch.cat([tr.client.params, tr.server.params]).view(torch.int32).cpu()
    return recs, bits


@pytest.mark.parametrize("batch", ["fixture", "synthetic8"])
@pytest.mark.parametrize("conv", ["x3", "f32"])
@pytest.mark.parametrize("scenario", list(N.SCENARIOS))
def test_split_trainer_steps(gpu, scenario, conv, batch):
    params, x, y = _case(batch)
    pp, xb = _poison(params, x, scenario)
    batches = [(xb, y), (x, y), (x, y)]
    want, _ = N.k2_steps(pp, batches, preset=conv, rule=True)
    ref, _ = N.k2_steps(pp, batches, preset=conv, rule=False)
    got = {g: _run(gpu, pp, batches, conv, g) for g in (False, True)}
    assert torch.equal(got[False][1], got[True][1]), "eager and graphed steps differ (bits, NaNs included)"
    for step, (w, t) in enumerate(zip(want, ref), 1):
        for g in (False, True):
            r = got[g][0][step - 1]
            what = f"{scenario} {conv} {batch} graph={g} step {step}"
            assert math.isfinite(r["loss"]) == math.isfinite(w["loss"]), f"{what}: logged loss {r['loss']}, rule {w['loss']}"
            assert r["bad"] == w["bad"], f"{what}: non-finite tensors {sorted(r['bad'])}, rule {sorted(w['bad'])}"
            assert r["raised"] == (r["bad"] or None), f"{what}: check_finite named {r['raised']}"
        assert got[False][0][step - 1]["loss"] == got[True][0][step - 1]["loss"] or \
            all(math.isnan(got[g][0][step - 1]["loss"]) for g in (False, True))
        if scenario in HIDDEN:          # the finding: the reference logs NaN, this project a finite loss
            assert math.isnan(t["loss"]) and math.isfinite(got[True][0][step - 1]["loss"])
        elif scenario in REPORTED:
            assert math.isnan(t["loss"]) and math.isnan(got[True][0][step - 1]["loss"])
        else:
            assert math.isfinite(t["loss"]) and got[True][0][step - 1]["raised"] is None


@pytest.mark.parametrize("conv", ["x3", "f32"])
@pytest.mark.parametrize("scenario", [s for s in N.SCENARIOS if not s.startswith("x-")])
def test_evaluate_and_predict_on_a_poisoned_model(gpu, scenario, conv):
    """evaluate() / predict() before any step, on the poisoned parameters and the clean fixture batch: the loss is finite
    exactly where the rule's forward says so (every hidden parameter scenario), the logits are finite in the same rows,
    and check_finite() already names the poisoned tensor."""
    params, x, y = _case("fixture")
    pp, _ = _poison(params, x, scenario)
    want = N.k2_eval_loss(pp, x, y, preset=conv, rule=True)
    for graph in (False, True):
        tr = _trainer(gpu, pp, conv, graph)
        res = tr.evaluate([(x.to(gpu), y.to(gpu))])
        assert math.isfinite(res.loss) == math.isfinite(want), (scenario, conv, graph, res.loss, want)
        _, logits = tr.predict(x.to(gpu), return_logits=True)
        with torch.no_grad():
            lw = N.k2_forward({k: v.double() for k, v in pp.items()}, x.double(), conv, True)
        assert torch.equal(torch.isfinite(logits).cpu(), torch.isfinite(lw))
        name = N.SCENARIOS[scenario][0]
        assert _raised(tr) == ({name} if name else None)
    if scenario in HIDDEN:
        assert math.isfinite(want) and math.isnan(N.k2_eval_loss(pp, x, y, preset=conv, rule=False))


@pytest.mark.parametrize("conv", ["x3", "f32"])
def test_clipped_step_spoils_the_whole_stage(gpu, conv):
    """conv2.weight NaN under optim.ClipNorm(1.0): the client's gradient holds NaN (0 x NaN through the cut gradient), its
    global norm is NaN, the coefficient stays NaN (slk_sgdm_clip_multi, as torch.clamp) and every client parameter is NaN
    after step 1; plain SGD leaves finite values in both client tensors. The server's gradient is finite, so its clipped
    step spoils nothing more than the poisoned element."""
    from splitcnn.optim import ClipNorm
    params, x, y = _case("fixture")
    pp, _ = _poison(params, x, "conv2.weight-nan")
    batches = [(x, y)] * 3
    want_clip, _ = N.k2_steps(pp, batches, preset=conv, rule=True, clip=1.0)
    want_plain, _ = N.k2_steps(pp, batches, preset=conv, rule=True)
    assert want_clip[0]["whole"] == {"conv1.weight", "conv1.bias"} and not want_plain[0]["whole"]
    for graph in (False, True):
        clipped, _ = _run(gpu, pp, batches, conv, graph, clip=ClipNorm(1.0))
        plain, _ = _run(gpu, pp, batches, conv, graph)
        for step in range(3):
            assert clipped[step]["whole"] == want_clip[step]["whole"], (step, clipped[step]["whole"])
            assert clipped[step]["bad"] == want_clip[step]["bad"]
            assert plain[step]["whole"] == want_plain[step]["whole"] == set()
            assert math.isfinite(clipped[step]["loss"]) and clipped[step]["raised"] == clipped[step]["bad"]


def test_check_finite_names_stage_block_and_tensor(gpu):
    """check_finite() on WideTrainer (Adam: m and v blocks; ema: the averaged block) and on its stages: silent on a fresh
    trainer; one NaN written into a parameter, an optimizer-state block or the averaged block is named by stage, tensor
    and block; the stage's own check_finite() reports the same tensor."""
    from splitcnn.optim import EMA, Adam
    from splitcnn.wide import WideTrainer, init_wide_models
    tr = WideTrainer(*init_wide_models(seed=0), device=gpu, graph=False, optim=Adam(1e-3), ema=EMA(0.999))
    tr.check_finite()
    tr.client.check_finite()
    tr.server.check_finite("server")
    n_c1 = tr.client.model.state_dict()["conv1.weight"].numel()
    for block, stage, off, want in (("params", tr.client, n_c1, "client.conv1.bias"),
                                    ("m", tr.client, 0, "client.conv1.weight (m)"),
                                    ("v", tr.server, tr.server.params.numel() - 1, "server.fc.bias (v)"),
                                    ("ema", tr.server, 0, "server.fc.weight (ema)")):
        flat = getattr(stage, block)
        keep = flat[off].clone()
        flat[off] = float("inf") if block == "v" else float("nan")
        with pytest.raises(FloatingPointError) as e:
            tr.check_finite()
        assert str(e.value).endswith("in " + want), str(e.value)
        with pytest.raises(FloatingPointError) as e:
            stage.check_finite(want.split(".")[0])
        assert str(e.value).endswith("in " + want), str(e.value)
        flat[off] = keep
        tr.check_finite()


# ============================================================================ WideTrainer (K5)
def _wide_trainer(gpu, scenario, graph):
    """A WideTrainer on seed-0 weights with the scenario's parameter poisoned, and the float64 copy of those weights."""
    from splitcnn.wide import WideTrainer, init_wide_models
    a, b = init_wide_models(seed=0)
    sd = {**a.state_dict(), **b.state_dict()}
    name, v = N.K5_SCENARIOS[scenario]
    if name not in (None, "x"):
        with torch.no_grad():
            sd[name][N.scenario_index(name, sd[name].shape)] = v
    params = {k: t.detach().clone().double() for k, t in sd.items()}       # the model runs on the CPU
    return WideTrainer(a, b, device=gpu, graph=graph, seed=0), params


def _wide_batches(gpu, scenario):
    from splitcnn.wide import SyntheticCIFAR
    data = SyntheticCIFAR(91)
    batches = [tuple(t.to(gpu) for t in data.batch(8)) for _ in range(3)]
    name, v = N.K5_SCENARIOS[scenario]
    if name == "x":
        x = batches[0][0].clone()
        x[N.scenario_index("x", x.shape)] = v
        batches[0] = (x, batches[0][1])
    return batches


def _wide_bad(tr):
    sd = {**tr.client.model.state_dict(), **tr.server.model.state_dict()}
    return {t for t in N.K5_TENSORS if not torch.isfinite(sd[t]).all()}


def _wide_raised(tr):
    try:
        tr.check_finite()
    except FloatingPointError as e:
        return {t for t in N.K5_TENSORS if f"{'server' if t.startswith('fc') else 'client'}.{t}" in str(e)}
    return None


@pytest.mark.parametrize("scenario", list(N.K5_SCENARIOS))
def test_wide_trainer_steps(gpu, scenario):
    """Three Adam steps of WideTrainer at B = 8 on seeded synthetic batches, one poison planted before step 1, eager and
    graphed, against nonfinite_ref.k5_steps (float64, the dropout masks of the three steps, clause 2's selects and
    dropout as a select). The model's table, which the GPU reproduces (the same in all three steps):

      x pixel NaN / +inf                    finite loss   HIDDEN    conv1.weight (+inf: see below)
      conv1 / conv2 / conv3 weight or bias  finite loss   HIDDEN    the poisoned tensor and what the cut gradient's
                                                                    0 x NaN reaches below it
      fc.weight NaN / +inf, fc.bias NaN     NaN loss      reported  every tensor

    torch (rule=False, pinned on the CPU) logs NaN in step 1 of every poisoned scenario. Asserted per step: the logged
    loss's finiteness, the set of non-finite parameter tensors, check_finite() naming exactly those, eager and graphed
    bit for bit. For the +inf pixel the activations hold +inf, and the 2:4-sparse weight gradients may or may not form
    its products with exact zeros of dY (clause 4): there the non-finite tensors are held to a subset of the dense
    model's that contains conv1.weight, and everything else is asserted as usual."""
    batches = _wide_batches(gpu, scenario)
    got = {}
    for graph in (False, True):
        tr, params = _wide_trainer(gpu, scenario, graph)
        recs = []
        for x, y in batches:
            tr.step(x, y)
            torch.cuda.synchronize()
            recs.append(dict(bad=_wide_bad(tr), raised=_wide_raised(tr)))
        for r, (_, loss) in zip(recs, tr.loss_log.flush()):
            r["loss"] = loss
        got[graph] = (recs, torch.cat([tr.client.params, tr.server.params]).view(torch.int32).clone())
    want = N.k5_steps(params, [(x.cpu(), y.cpu()) for x, y in batches], seed=0, rule=True)
    assert torch.equal(got[False][1], got[True][1]), "eager and graphed steps differ (bits, NaNs included)"
    hidden = scenario != "clean" and not scenario.startswith("fc.")
    for step, w in enumerate(want):
        for graph in (False, True):
            r = got[graph][0][step]
            what = f"{scenario} graph={graph} step {step + 1}"
            assert math.isfinite(r["loss"]) == math.isfinite(w["loss"]), f"{what}: logged loss {r['loss']}, rule {w['loss']}"
            if scenario == "x-pinf":
                assert "conv1.weight" in r["bad"] <= w["bad"], f"{what}: {sorted(r['bad'])} not within {sorted(w['bad'])}"
            else:
                assert r["bad"] == w["bad"], f"{what}: non-finite tensors {sorted(r['bad'])}, rule {sorted(w['bad'])}"
            assert r["raised"] == (r["bad"] or None), f"{what}: check_finite named {r['raised']}"
            assert math.isfinite(r["loss"]) == (hidden or scenario == "clean"), what


@pytest.mark.parametrize("scenario", [s for s in N.K5_SCENARIOS if not s.startswith("x-")])
def test_wide_evaluate_and_predict_on_a_poisoned_model(gpu, scenario):
    """WideTrainer.evaluate() / predict() before any step on the poisoned parameters (no dropout in evaluation): the
    loss and every logit are finite exactly where the rule's forward says, and check_finite() names the tensor."""
    batches = _wide_batches(gpu, "clean")
    x, y = batches[0]
    for graph in (False, True):
        tr, params = _wide_trainer(gpu, scenario, graph)
        with torch.no_grad():
            lw = N.k5_forward(params, x.cpu().double(), None, True)
            want = float(torch.nn.functional.cross_entropy(lw, y.cpu()))
        res = tr.evaluate([(x, y)])
        assert math.isfinite(res.loss) == math.isfinite(want), (scenario, graph, res.loss, want)
        _, logits = tr.predict(x, return_logits=True)
        assert torch.equal(torch.isfinite(logits).cpu(), torch.isfinite(lw))
        name = N.K5_SCENARIOS[scenario][0]
        assert _wide_raised(tr) == ({name} if name else None)
        assert math.isfinite(want) == (not scenario.startswith("fc."))


def test_check_finite_names_sgd_momentum(gpu):
    """check_finite() on a SplitTrainer with optim.SGD(momentum=0.9): a NaN written into the momentum buffer is reported
    as "client.conv1.bias (momentum)" by the trainer and by the stage; silent before and after."""
    from splitcnn.data import init_models
    from splitcnn.engine import SplitTrainer
    from splitcnn.optim import SGD
    tr = SplitTrainer(*init_models(seed=0), device=gpu, graph=False, optim=SGD(0.01, momentum=0.9))
    tr.check_finite()
    keep = tr.client.buf[300].clone()
    tr.client.buf[300] = float("nan")
    for check, stage in ((tr.check_finite, ()), (tr.client.check_finite, ("client",))):
        with pytest.raises(FloatingPointError) as e:
            check(*stage)
        assert str(e.value).endswith("in client.conv1.bias (momentum)"), str(e.value)
    tr.client.buf[300] = keep
    tr.check_finite()
