"""CPU: tests/x3_split_ref.py pinned - the split, the shares that make its operand classes discriminate, the
exactness claim executed in float32, the image decoder, and five WRONG variants of the arithmetic that must each
change the expectation (which is what shows that tests/test_x3_lo_exact_gpu.py would fail on such a kernel)."""
import numpy as np
import pytest
import torch

from ref64 import route64
from x3_split_ref import (ACT16_SAMPLE, assert_exact, conv64, decode_act16, gen14, gen18, gen_both, gen_small,
                          gran_exp, kept_addends, split, split_np, three_term, x3_exp)

A_SHAPE, W_SHAPE, D_SHAPE = (2, 32, 26, 26), (64, 32, 3, 3), (2, 64, 12, 12)


def _g(seed):
    return torch.Generator().manual_seed(seed)


# ----------------------------------------------------------------------------- scale and split
def test_x3_exp():
    assert x3_exp(np.float32(1.0)) == 13 and x3_exp(np.float32(2 ** 13)) == 0 and x3_exp(np.float32(16383.0)) == 0
    assert x3_exp(np.float32(2 ** 14)) == -1 and x3_exp(np.float32(3e38)) == 14 - 128
    assert x3_exp(np.float32(0.0)) == 0 and x3_exp(np.float32(-1.0)) == 0
    assert x3_exp(np.float32("inf")) == 0 and x3_exp(np.float32("nan")) == 0
    assert [int(x3_exp(np.float32(2.0 ** -k))) for k in (112, 113, 114, 120)] == [125, 126, 126, 126]   # the clamp
    assert x3_exp(np.float32(1e-40)) == 126                                                            # a subnormal
    a = np.exp(np.random.default_rng(0).uniform(-60, 60, 4096)).astype(np.float32)
    scaled = a.astype(np.float64) * 2.0 ** x3_exp(a)
    assert (scaled >= 2 ** 13).all() and (scaled < 2 ** 14).all()


CLASSES = {"14-bit": gen14, "18-bit": gen18, "both-sided": gen_both}


@pytest.mark.parametrize("name", list(CLASSES))
@pytest.mark.parametrize("signed", [False, True])
def test_every_class_splits_without_a_remainder(name, signed):
    v = CLASSES[name](_g(1), (5, 32, 26, 26), 0.5, signed)
    h, l, rem = split(v)
    assert torch.equal(h + l, v.double()) and not rem.any()
    assert float(v.abs().max()) < 2 ** 14 and (signed == bool((v < 0).any()))
    # the torch and the numpy statement of the split agree bit for bit (scaled domain)
    s = x3_exp(v.flatten(1).abs().max(1).values.numpy())
    hn, ln = split_np(v.numpy(), s)
    un = (2.0 ** -s.astype(np.float64))[:, None, None, None]
    assert np.array_equal(hn.astype(np.float64) * un, h.numpy()) and np.array_equal(ln.astype(np.float64) * un, l.numpy())
    # per-sample and whole-tensor scales give the same halves: the split depends on the value alone here
    h1, l1, _ = split(v, per_sample=False)
    assert torch.equal(h1, h) and torch.equal(l1, l)
    # a loose scale bound (x 16) too
    h2, l2, _ = split(v, amax=v.flatten(1).abs().max(1).values * 16)
    assert torch.equal(h2, h) and torch.equal(l2, l)


def test_the_shares_that_make_the_classes_discriminate():
    v = gen14(_g(2), (5, 32, 26, 26), 0.5, True)
    h, l, _ = split(v)
    nz = v != 0
    assert 0.45 < float(nz.double().mean()) < 0.55
    assert float((l[nz] != 0).double().mean()) >= 0.80                      # measured 0.875
    tie = nz & (v.abs() % 8 == 4)
    assert float(tie.double().sum() / nz.sum()) >= 0.08                     # measured 0.125
    assert ((h[tie].abs() / 8) % 2 == 0).all() and (l[tie].abs() == 4).all()   # ties went to the EVEN neighbour
    assert (l[tie] * v[tie].sign() > 0).any() and (l[tie] * v[tie].sign() < 0).any()   # both up and down
    assert (h % 8 == 0).all() and float(l.abs().max()) == 4
    assert (l > 0).any() and (l < 0).any()
    v = gen18(_g(3), (5, 32, 26, 26), 0.5, False)
    h, l, _ = split(v)
    assert len(torch.unique(l)) >= 100                                      # measured 129
    assert float(l[l != 0].abs().min()) == 2.0 ** -4 and (l > 0).any() and (l < 0).any()
    v = gen_both(_g(4), (5, 32, 26, 26), 0.5, True)
    h, l, _ = split(v)
    assert set(torch.unique(h.abs()).tolist()) == {0.0, 4096.0, 6144.0} and set(torch.unique(l).tolist()) == {-1.0, 0.0, 1.0}


def test_truncation_is_a_different_split():
    for gen in (gen14, gen18, gen_both):
        v = gen(_g(5), (2, 32, 26, 26), 0.5, True)
        h, l, _ = split(v)
        ht, lt, rem = split(v, trunc=True)
        assert torch.equal(ht + lt, v.double()) and not rem.any()
        assert (ht.abs() <= v.abs().double()).all()
        assert float((ht != h).double().mean()) >= 0.1 and float((lt != l).double().mean()) >= 0.1
        s = x3_exp(v.flatten(1).abs().max(1).values.numpy())
        hn, ln = split_np(v.numpy(), s, trunc=True)
        un = (2.0 ** -s.astype(np.float64))[:, None, None, None]
        assert np.array_equal(hn.astype(np.float64) * un, ht.numpy()) and np.array_equal(ln.astype(np.float64) * un, lt.numpy())


def test_gran_exp():
    assert gran_exp(torch.tensor([8.0, 24.0, 0.0])) == 3 and gran_exp(torch.tensor([0.75, 4.0])) == -2
    assert gran_exp(torch.zeros(3)) is None and gran_exp(torch.tensor([-6144.0]), torch.tensor([5.0])) == 0


# ----------------------------------------------------------------------------- operands of the three operations
def _operands(op, cls, seed=10, trunc=False):
    """(a_h, a_l, b_h, b_l) of one operation and class at B = 2, as tests/test_x3_lo_exact_gpu.py builds them."""
    g = _g(seed)
    small_w = lambda: gen_small(g, W_SHAPE, 0.3, [1], True)                  # noqa: E731
    if op == "fwd":
        a = {"a14": lambda: gen14(g, A_SHAPE, 0.15, False), "a18": lambda: gen18(g, A_SHAPE, 0.15, False),
             "b14": lambda: gen_small(g, A_SHAPE, 0.15, [1, 2, 3], False),
             "both": lambda: gen_both(g, A_SHAPE, 0.15, False)}[cls]()
        b = {"a14": small_w, "a18": small_w, "b14": lambda: gen14(g, W_SHAPE, 1.0, True),
             "both": lambda: gen_both(g, W_SHAPE, 0.3, True)}[cls]()
        ah, al, _ = split(a, trunc=trunc)
        bh, bl, _ = split(b, per_sample=False, trunc=trunc)
        return ah, al, bh, bl
    code = torch.randint(0, 5, D_SHAPE, generator=g).to(torch.uint8)
    if op == "dgrad":
        a = {"a14": lambda: gen14(g, D_SHAPE, 0.3, True), "a18": lambda: gen18(g, D_SHAPE, 0.3, True),
             "b14": lambda: gen_small(g, D_SHAPE, 0.3, [1, 2, 3], True),
             "both": lambda: gen_both(g, D_SHAPE, 0.3, True)}[cls]()
        b = {"a14": small_w, "a18": small_w, "b14": lambda: gen14(g, W_SHAPE, 1.0, True),
             "both": lambda: gen_both(g, W_SHAPE, 0.3, True)}[cls]()
        ah, al, _ = split(a, trunc=trunc)
        bh, bl, _ = split(b, per_sample=False, trunc=trunc)
        return route64(ah, code), route64(al, code), bh, bl
    a = {"a14": lambda: gen14(g, A_SHAPE, 0.15, False), "a18": lambda: gen18(g, A_SHAPE, 0.15, False),
         "b14": lambda: gen_small(g, A_SHAPE, 0.15, [1, 2, 3], False),
         "both": lambda: gen_both(g, A_SHAPE, 0.15, False)}[cls]()
    b = {"a14": lambda: gen_small(g, D_SHAPE, 0.3, [1], True), "a18": lambda: gen_small(g, D_SHAPE, 0.3, [1], True),
         "b14": lambda: gen14(g, D_SHAPE, 0.3, True), "both": lambda: gen_both(g, D_SHAPE, 0.3, True)}[cls]()
    ah, al, _ = split(a, trunc=trunc)
    bh, bl, _ = split(b, trunc=trunc)
    return ah, al, route64(bh, code), route64(bl, code)


OPS = ["fwd", "dgrad", "wgrad"]
ALL = ["a14", "a18", "b14", "both"]      # l in operand a (14- and 18-bit), l in operand b, both-sided


@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("cls", ALL)
def test_one_sided_classes_are_plain_float64_and_the_both_sided_class_is_not(op, cls):
    ah, al, bh, bl = _operands(op, cls)
    assert_exact(ah, al, bh, bl, op)
    full = three_term(ah + al, torch.zeros_like(al), bh + bl, torch.zeros_like(bl), op)     # float64's sum a b
    got = three_term(ah, al, bh, bl, op)
    if cls != "both":
        assert torch.equal(got, full)
        return
    share = float((got != full).double().mean())
    # measured 0.83 / 0.77 / 0.81 of the outputs: asserted at about half
    assert share >= {"fwd": 0.4, "dgrad": 0.38, "wgrad": 0.4}[op], share
    assert torch.equal(three_term(ah, al, bh, bl, op, add_ll=True), full)     # the dropped term is all that differs


def test_both_sided_forward_routes_differently_in_some_windows():
    """The three-term forward differs from float64's in pooled values window by window (the GPU test compares
    those): measured 0.74 of the windows at these densities; asserted at about half."""
    ah, al, bh, bl = _operands("fwd", "both")
    pool = lambda y: y.clamp_min(0).reshape(2, 64, 12, 2, 12, 2).amax(dim=(3, 5))     # noqa: E731
    share = float((pool(three_term(ah, al, bh, bl, "fwd")) != pool(conv64(ah + al, bh + bl))).double().mean())
    print(f"both-sided forward: {share:.3f} of the windows differ from float64")
    assert share >= 0.37, share


# ----------------------------------------------------------------------------- the exactness claim, executed
def _f32_sum(x):
    acc = np.float32(0)
    for t in x:
        acc = np.float32(acc + t)
    return acc


def _f32_tree(x):
    x = list(x)
    while len(x) > 1:
        x = [np.float32(x[i] + x[i + 1]) if i + 1 < len(x) else x[i] for i in range(0, len(x), 2)]
    return x[0]


@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("cls", ALL)
def test_float32_sums_in_any_order_equal_the_model(op, cls):
    """All kept addends of an output, added in float32 in shuffled, sorted, chunked and tree orders, give the
    float64 model's value bit for bit: the bound means what it says."""
    ah, al, bh, bl = _operands(op, cls)
    assert_exact(ah, al, bh, bl, op)
    model = three_term(ah, al, bh, bl, op)
    rng = np.random.default_rng(7)
    flat = model.reshape(-1)
    busy = torch.nonzero(flat).reshape(-1)
    picks = busy[torch.from_numpy(rng.choice(len(busy), size=6, replace=False))].tolist() + [int(flat.abs().argmax())]
    for k in picks:
        idx = tuple(int(i) for i in np.unravel_index(k, tuple(model.shape)))
        add = kept_addends(ah, al, bh, bl, op, idx).numpy()
        add = add[add != 0]
        a32 = add.astype(np.float32)
        assert np.array_equal(a32.astype(np.float64), add) and len(add) >= 1
        want = float(flat[k])
        assert float(add.sum()) == want
        orders = [rng.permutation(len(a32)) for _ in range(5)]
        orders += [np.argsort(np.abs(a32)), np.argsort(-np.abs(a32)), np.argsort(a32)]
        for o in orders:
            assert float(_f32_sum(a32[o])) == want
            assert float(_f32_tree(a32[o])) == want
            # partial chains summed afterwards (the kernels' separate cross-term chain, K shares, slabs)
            parts = [_f32_sum(c) for c in np.array_split(a32[o], 4)]
            assert float(_f32_sum(parts)) == want


def test_the_bound_refuses_what_is_not_exact():
    g = _g(20)
    v = torch.randint(2 ** 17, 2 ** 18, A_SHAPE, generator=g).float() * 2.0 ** -4
    a = torch.where(torch.rand(A_SHAPE, generator=g) < 0.9, v, torch.zeros(A_SHAPE))     # dense 18-bit: too much
    ah, al, _ = split(a)
    bh, bl, _ = split(gen_small(g, W_SHAPE, 0.9, [1], True), per_sample=False)
    with pytest.raises(AssertionError, match="not exact"):
        assert_exact(ah, al, bh, bl, "fwd")


# ----------------------------------------------------------------------------- images
def encode_act16(h, l, swizzle_l=True):
    """numpy encoder of the act16 layout: (h, l) float16 [B, 32, 26, 26] -> uint8 [B * 86,528]. swizzle_l = False is
    the WRONG variant that stores the l plane's chunks unswizzled."""
    B = h.shape[0]
    img = np.zeros((B, 2, 676, 4, 8), dtype=np.float16)
    for pl, v, swz in ((0, h, True), (1, l, swizzle_l)):
        for y in range(26):
            for x in range(26):
                for c8 in range(4):
                    slot = c8 ^ (x & 2) if swz else c8
                    img[:, pl, 26 * y + x, slot] = v[:, 8 * c8:8 * c8 + 8, y, x]
    out = img.reshape(-1).view(np.uint8)
    assert out.size == B * ACT16_SAMPLE
    return out


def test_decode_act16_inverts_the_encoder():
    rng = np.random.default_rng(3)
    h = rng.standard_normal((3, 32, 26, 26)).astype(np.float16)
    l = rng.standard_normal((3, 32, 26, 26)).astype(np.float16)
    l[0, 5, 3, 2] = np.float16(-0.0)
    img = encode_act16(h, l)
    gh, gl = decode_act16(img, 3)
    assert gh.shape == gl.shape == (3, 32, 26, 26) and gh.dtype == np.float64
    assert np.array_equal(gh.astype(np.float16).view(np.uint16), h.view(np.uint16))
    assert np.array_equal(gl.astype(np.float16).view(np.uint16), l.view(np.uint16))
    # where each element lives, stated once more by hand: sample 1, l plane, pixel (y 4, x 7), channel 21
    off = 1 * 86528 + 43264 + (26 * 4 + 7) * 64 + ((2 ^ (7 & 2)) * 16) + 2 * (21 - 16)
    assert img[off:off + 2].view(np.float16)[0] == l[1, 21, 4, 7]
    off = 2 * 86528 + (26 * 25 + 25) * 64 + ((3 ^ (25 & 2)) * 16) + 2 * (31 - 24)      # the last element of an h plane
    assert img[off:off + 2].view(np.float16)[0] == h[2, 31, 25, 25] and off == 2 * 86528 + 43264 - 2
    # the unswizzled l plane decodes to other values at every pixel with x & 2, and to the same ones elsewhere
    _, bl = decode_act16(encode_act16(h, l, swizzle_l=False), 3)
    x2 = (np.arange(26) & 2) != 0
    assert np.array_equal(bl[..., ~x2], gl[..., ~x2]) and (bl[..., x2] != gl[..., x2]).mean() > 0.99


# ----------------------------------------------------------------------------- the five wrong variants
def _applies(variant, cls):
    return {"drop lh": cls in ("a14", "a18", "both"), "drop hl": cls in ("b14", "both"), "fourth term": cls == "both",
            "truncation": cls == "both", "l swizzle": cls in ("a14", "a18", "both")}[variant]


@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("cls", ALL)
@pytest.mark.parametrize("variant", ["drop lh", "drop hl", "fourth term", "truncation", "l swizzle"])
def test_wrong_variants_change_the_expectation(op, cls, variant):
    """l_a h_b dropped, h_a l_b dropped, the fourth term added, the halves made by truncation, the l plane's slot
    swizzle left out: each changes the model's output on every class it applies to (a variant does not apply where
    the l it touches is zero; truncation leaves h + l, hence a one-sided product, unchanged and shows in the
    both-sided class, through the dropped term, and in the images). The swizzle variant needs an image operand:
    the forward and the weight gradient."""
    if not _applies(variant, cls) or (variant == "l swizzle" and op == "dgrad"):
        ah, al, bh, bl = _operands(op, cls)
        good = three_term(ah, al, bh, bl, op)
        if variant in ("drop lh", "drop hl", "fourth term"):      # and where it does not apply it changes nothing
            kw = {"drop lh": dict(drop=("lh",)), "drop hl": dict(drop=("hl",)), "fourth term": dict(add_ll=True)}[variant]
            assert torch.equal(three_term(ah, al, bh, bl, op, **kw), good)
        return
    ah, al, bh, bl = _operands(op, cls)
    good = three_term(ah, al, bh, bl, op)
    if variant == "drop lh":
        bad = three_term(ah, al, bh, bl, op, drop=("lh",))
    elif variant == "drop hl":
        bad = three_term(ah, al, bh, bl, op, drop=("hl",))
    elif variant == "fourth term":
        bad = three_term(ah, al, bh, bl, op, add_ll=True)
    elif variant == "truncation":
        bad = three_term(*_operands(op, cls, trunc=True), op)
    else:
        s = x3_exp((ah + al).flatten(1).abs().max(1).values.numpy())
        sc = (2.0 ** s.astype(np.float64))[:, None, None, None]
        h16, l16 = (ah.numpy() * sc).astype(np.float16), (al.numpy() * sc).astype(np.float16)
        gh, gl = decode_act16(encode_act16(h16, l16, swizzle_l=False), ah.shape[0])
        assert np.array_equal(gh / sc, ah.numpy())
        bad = three_term(ah, torch.from_numpy(gl / sc), bh, bl, op)
    share = float((bad != good).double().mean())
    assert share >= 0.05, f"{variant} on {op} {cls}: only {share:.4f} of the outputs change"
