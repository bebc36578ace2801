"""The launches of one training step, for every optimizer recipe and stepping path, against
tests/golden/step_launches.json.

The layer between the trainers and the kernels (splitcnn/recipe.py, the stages' step methods) has one output: the
sequence of slk_* entry points it calls and what it passes by value. tools/record_step_launches.py defines the
configurations and the record format and wrote the golden; a change that alters launches on purpose regenerates
it with that tool, a refactor reproduces the one recorded on its parent commit. Per configuration two eager steps
run (K2 at B = 16, K5 at B = 8) and the second is compared: the first differs by lazily allocated buffers.
Also here: the construction rules of the K5 stages (their K2 twins need no device: tests/test_recipe_cpu.py)."""
import importlib.util
import json
import os

import pytest
import torch

from conftest import GOLDEN, ROOT
from splitcnn import optim

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location("record_step_launches",
                                               os.path.join(ROOT, "tools", "record_step_launches.py"))
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)

with open(os.path.join(GOLDEN, "step_launches.json")) as f:
    GOLD = json.load(f)

BUILDERS = {}
for table, build, batch in ((rec.K2_TRAINERS, rec.k2_trainer, rec.k2_batch), (rec.K2_STAGES, rec.K2Stages, rec.k2_batch),
                            (rec.K5_TRAINERS, rec.k5_trainer, rec.k5_batch), (rec.K5_STAGES, rec.K5Hub, rec.k5_batch)):
    for name, kw in table.items():
        BUILDERS[name] = (build, kw, batch)


def test_the_golden_covers_exactly_the_tools_configurations():
    assert sorted(GOLD["steps"]) == sorted(BUILDERS) and len(BUILDERS) == 27
    assert GOLD["batch"] == {"k2": rec.K2_B, "k5": rec.K5_B}
    assert len(GOLD["recorded_on_commit"]) == 40
    assert all(len(v) > 0 for v in GOLD["steps"].values())


@pytest.mark.parametrize("name", sorted(BUILDERS))
def test_second_step_launches_match_the_golden(gpu, name):
    build, kw, batch = BUILDERS[name]
    runner, (x, y) = build(gpu, **kw(gpu)), batch(gpu)
    runner.step(x, y)
    with rec.recording([]) as got:
        runner.step(x, y)
    torch.cuda.synchronize()
    want = GOLD["steps"][name]
    got = json.loads(json.dumps(got))   # as the file holds them
    assert [r[0] for r in got] == [r[0] for r in want]
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, (name, k)


# ------------------------------------------------------------------ construction rules, K5
def test_k5_construction_rules(gpu):
    from splitcnn.wide import BETA1, BETA2, EPS, LR, WideClientStage, WideServerStage

    def clipnorm():
        return optim.ClipNorm(1.0, device=gpu)

    for cls in (WideClientStage, WideServerStage):
        n = len(cls.PAIRS)
        plain = cls(device=gpu)
        for a in ("optim", "schedule", "clip", "clip_out", "trust_out", "ema", "ema_cfg"):
            assert getattr(plain, a) is None, a
        # the default Adam has its moments and its counter
        assert plain.m.shape == plain.v.shape == plain.params.shape and not plain.m.any() and not plain.v.any()
        assert plain.step_ctr.dtype == torch.int32 and plain.step_ctr.tolist() == [0] and plain.auto_tick
        assert (plain.lr, plain.betas, plain.eps) == (LR, (BETA1, BETA2), EPS)

        with pytest.raises(TypeError, match="splitcnn.optim.Adam"):
            cls(device=gpu, optim=optim.SGD(0.1))
        with pytest.raises(TypeError, match="ClipNorm"):
            cls(device=gpu, clip=1.0)
        with pytest.raises(TypeError, match="EMA"):
            cls(device=gpu, ema=0.999)
        with pytest.raises(ValueError, match="not combined with clip="):
            cls(device=gpu, optim=optim.LAMB(), clip=clipnorm())

        # schedule= / clip= alone imply optim.Adam(lr, betas, eps) at the stage's constants
        sched, clip = optim.LRSchedule.from_values([2e-3, 1e-3], gpu), clipnorm()
        for kw in (dict(schedule=sched), dict(clip=clip)):
            st = cls(device=gpu, lr=2e-3, betas=(0.8, 0.99), eps=1e-7, **kw)
            o = st.optim
            assert type(o) is optim.Adam and (o.lr, o.betas, o.eps) == (2e-3, (0.8, 0.99), 1e-7)
            assert (o.weight_decay, o.decoupled) == (0, True)
            assert st.schedule is sched if "schedule" in kw else st.schedule.values.tolist() == [pytest.approx(2e-3)]
            assert (st.clip is clip and st.clip_out.tolist() == [0, 0]) if "clip" in kw else st.clip is None
            assert st.trust_out is None and st.ema is None
        # ema= keeps the default Adam launches
        ema = optim.EMA(0.9, device=gpu)
        st = cls(device=gpu, ema=ema)
        assert st.optim is None and st.schedule is None and st.ema_cfg is ema
        assert torch.equal(st.ema, st.params) and st.ema.data_ptr() != st.params.data_ptr()

        cfg = optim.Adam(3e-3, betas=(0.8, 0.99), eps=1e-7, weight_decay=0.01)
        st = cls(device=gpu, optim=cfg)
        assert st.optim is cfg and (st.lr, st.betas, st.eps) == (3e-3, (0.8, 0.99), 1e-7)
        seg = st.seg(0, 8, torch.zeros(1, 8, device=gpu))
        assert [t.data_ptr() for t in seg.state] == [st.m.data_ptr(), st.v.data_ptr()] and seg.owner is None
        lamb = cls(device=gpu, optim=optim.LAMB())
        assert lamb.trust_out.shape == (2 * n, 3) and not lamb.trust_out.any() and lamb.clip_out is None
