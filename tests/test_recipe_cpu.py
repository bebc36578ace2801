"""splitcnn.recipe on CPU stages: everything the recipe layer decides before its first launch.

The K2 stages construct on device="cpu" (only a step needs the GPU), so the rules of construction, the typed
segments, the expansion of a whole-stage segment into [weight | bias] pairs, the groups' sizes and the refusal of
another stage's segment are checked here without a device. The K5 stages build bf16 shadows in their constructor;
their construction rules are in tests/test_step_launches_gpu.py."""
import pytest
import torch

from splitcnn import ops, optim
from splitcnn.engine import ClientStage, ServerStage
from splitcnn.recipe import Seg, StageRecipe


def clipnorm(v=1.0):
    return optim.ClipNorm(v, device="cpu")


def span(t, base):
    return t.storage_offset() - base.storage_offset(), t.numel()


# ------------------------------------------------------------------ pairs
def test_pairs_tile_every_stage_in_lo_hi_nw_form():
    from splitcnn import wide
    for cls, n in ((ClientStage, ops.CLIENT_NPARAM), (ServerStage, ops.SERVER_NPARAM),
                   (wide.WideClientStage, wide.CLIENT_NPARAM), (wide.WideServerStage, wide.SERVER_NPARAM)):
        assert issubclass(cls, StageRecipe)
        edge = 0
        for lo, hi, nw in cls.PAIRS:
            assert lo == edge and lo < lo + nw <= hi, (cls.__name__, lo, hi, nw)
            edge = hi
        assert edge == n, cls.__name__
        assert len(cls.TENSORS) == 2 * len(cls.PAIRS)


def test_a_whole_stage_segment_expands_into_its_pairs():
    s = ServerStage(device="cpu", optim=optim.LARS(0.1))
    slabs = torch.zeros(3, ops.SERVER_NPARAM)
    whole = s.seg(0, ops.SERVER_NPARAM, slabs)
    assert isinstance(whole, Seg) and whole.nw is None and whole.owner is None and len(whole.state) == 1
    partials, out, segs = s._trust_group([whole])
    assert out is s.trust_out and len(segs) == 2
    assert [span(g[0], s.params) for g in segs] == [(0, 18496), (18496, 92170)]
    assert [span(g[1], s.grads) for g in segs] == [(0, 18496), (18496, 92170)]
    assert [span(g[2], s.buf) for g in segs] == [(0, 18496), (18496, 92170)]
    assert [g[-1] for g in segs] == [18432, 92160]
    for g, (lo, hi, _) in zip(segs, s.PAIRS):
        sl = g[3]
        assert sl.shape == (3, hi - lo) and sl.data_ptr() == slabs[:, lo:hi].data_ptr() and sl.stride() == slabs.stride()
    assert s.trust_nblk == [ops.reduce_sqnorm_nblk(n, 3) for n in (18496, 92170)]
    assert partials.numel() == 4 * sum(s.trust_nblk) == ops.trust_partials_needed(segs)
    # the gradient block in place: no grad to write, one slab
    segs = s._trust_group([s.grads_segment()])[2]
    assert [g[1] for g in segs] == [None, None] and [tuple(g[3].shape) for g in segs] == [(1, 18496), (1, 92170)]
    assert segs[1][3].data_ptr() == s.grads[18496:].data_ptr()
    # one pair alone keeps its slabs, and a one-pair stage is its own pair
    one = s._trust_group([s.seg(18496, ops.SERVER_NPARAM, slabs[:, 18496:])])[2]
    assert len(one) == 1 and one[0][-1] == 92160 and s.trust_nblk == [ops.reduce_sqnorm_nblk(92170, 3)]
    c = ClientStage(device="cpu", optim=optim.LARS(0.1))
    cs = c._trust_group([c.optim_segment(torch.zeros(2, ops.CLIENT_NPARAM))])[2]
    assert len(cs) == 1 and cs[0][-1] == 288 and span(cs[0][0], c.params) == (0, 320)


@pytest.mark.parametrize("lo,hi", [(0, 18432), (18432, ops.SERVER_NPARAM), (1, ops.SERVER_NPARAM), (0, 18497)])
def test_a_segment_off_the_pairs_is_refused(lo, hi):
    s = ServerStage(device="cpu", optim=optim.LARS(0.1))
    with pytest.raises(ValueError, match=r"one \[weight \| bias\] pair"):
        s._trust_group([s.seg(lo, hi, torch.zeros(1, hi - lo))])


def test_a_clip_group_is_the_stages_own_partials_and_norm():
    s = ServerStage(device="cpu", optim=optim.SGD(0.1, momentum=0.9), clip=clipnorm())
    s2, s3 = torch.zeros(5, ops.CONV2_SLAB), torch.zeros(2, ops.FC_SLAB)
    partials, out, segs = s._clip_group(s._slab_segments(s2, s3))
    assert out is s.clip_out and [len(g) for g in segs] == [4, 4]
    assert [span(g[0], s.params) for g in segs] == [(0, 18496), (18496, 92170)]
    assert segs[0][3] is s2 and segs[1][3] is s3
    want = ops.reduce_sqnorm_nblk(ops.CONV2_SLAB, 5) + ops.reduce_sqnorm_nblk(ops.FC_SLAB, 2)
    assert s.clip_npart == want == partials.numel()
    assert s._buf.get("clip_partials", (want,), torch.float32, s.device) is partials


# ------------------------------------------------------------------ another stage's segment
def _unchanged_after_refusal(server, client, match):
    before = client.params.clone()
    seg = client.optim_segment(torch.zeros(1, ops.CLIENT_NPARAM))
    assert seg.owner is client and span(seg.param, client.params) == (0, ops.CLIENT_NPARAM)
    with pytest.raises(ValueError, match=match):
        server._sgdm([seg], multi=True)
    assert torch.equal(client.params, before)


def test_a_segment_of_a_stage_with_another_clip_setting_is_refused():
    cfg = optim.SGD(0.01, momentum=0.9)
    for s_clip, c_clip in ((clipnorm(), None), (None, clipnorm()), (clipnorm(), clipnorm())):
        _unchanged_after_refusal(ServerStage(device="cpu", optim=cfg, clip=s_clip),
                                 ClientStage(device="cpu", optim=cfg, clip=c_clip), "clip=")


def test_a_segment_of_a_stage_with_another_recipe_is_refused():
    for s_opt, c_opt in ((optim.LARS(0.1), optim.SGD(0.1, momentum=0.9)), (optim.SGD(0.1, momentum=0.9), optim.LARS(0.1))):
        _unchanged_after_refusal(ServerStage(device="cpu", optim=s_opt), ClientStage(device="cpu", optim=c_opt),
                                 "layer-wise")


def test_a_segment_under_the_shared_recipe_reaches_the_launch():
    """Nothing is refused when the stages share the recipe: the first thing to raise is the wrapper's device check."""
    clip = clipnorm()
    for kw in (dict(), dict(optim=optim.SGD(0.1, momentum=0.9)), dict(optim=optim.SGD(0.1), clip=clip),
               dict(optim=optim.LARS(0.1))):
        server, client = ServerStage(device="cpu", **kw), ClientStage(device="cpu", **kw)
        own = server._slab_segments(torch.zeros(1, ops.CONV2_SLAB), torch.zeros(1, ops.FC_SLAB))
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            server._sgdm([*own, client.optim_segment(torch.zeros(1, ops.CLIENT_NPARAM))], multi=True)


# ------------------------------------------------------------------ construction
@pytest.mark.parametrize("cls", [ClientStage, ServerStage])
def test_construction_rules(cls):
    n = len(cls.PAIRS)
    plain = cls(device="cpu", lr=0.02)
    for a in ("optim", "schedule", "clip", "clip_out", "trust_out", "ema", "ema_cfg", "buf", "step_ctr"):
        assert getattr(plain, a) is None, a
    assert plain.auto_tick and plain.lr == 0.02
    assert plain.seg(0, 4, torch.zeros(1, 4)).state == ()

    with pytest.raises(TypeError, match="splitcnn.optim.SGD"):
        cls(device="cpu", optim=optim.Adam())
    with pytest.raises(TypeError, match="ClipNorm"):
        cls(device="cpu", clip=1.0)
    with pytest.raises(TypeError, match="EMA"):
        cls(device="cpu", ema=0.999)
    with pytest.raises(ValueError, match="not combined with clip="):
        cls(device="cpu", optim=optim.LARS(0.1), clip=clipnorm())

    # schedule= / clip= / ema= alone imply optim.SGD(lr) at the stage's lr
    sched, clip, ema = optim.LRSchedule.from_values([0.02, 0.01], device="cpu"), clipnorm(), optim.EMA(0.9, device="cpu")
    for kw in (dict(schedule=sched), dict(clip=clip), dict(ema=ema)):
        st = cls(device="cpu", lr=0.02, **kw)
        o = st.optim
        assert type(o) is optim.SGD and (o.lr, o.momentum, o.dampening, o.weight_decay, o.nesterov) == (0.02, 0, 0, 0, False)
        assert st.buf.shape == st.params.shape and not st.buf.any()
        assert st.step_ctr.dtype == torch.int32 and st.step_ctr.tolist() == [0] and st.auto_tick
        assert st.schedule is sched if "schedule" in kw else st.schedule.values.tolist() == [pytest.approx(0.02)]
        if "clip" in kw:
            assert st.clip is clip and st.clip_out.tolist() == [0, 0]
        else:
            assert st.clip is None and st.clip_out is None
        assert st.trust_out is None
        if "ema" in kw:
            assert st.ema_cfg is ema and torch.equal(st.ema, st.params) and st.ema.data_ptr() != st.params.data_ptr()
        else:
            assert st.ema is None and st.ema_cfg is None

    cfg = optim.SGD(0.05, momentum=0.9)
    st = cls(device="cpu", lr=0.02, optim=cfg)
    assert st.optim is cfg and st.lr == 0.05 and st.clip is None and st.trust_out is None
    assert st.seg(0, 4, torch.zeros(1, 4)).state[0].data_ptr() == st.buf.data_ptr()
    lars = cls(device="cpu", optim=optim.LARS(0.1))
    assert lars.trust_out.shape == (2 * n, 3) and not lars.trust_out.any() and lars.clip_out is None
