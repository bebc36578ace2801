"""TEST INFRASTRUCTURE: an independent numpy restatement of the whole batch slk_image_batch_blend builds.

Nothing here is imported from the package under test. The hash chain, the crop draws, the source-pixel rule and the
label packing are tests/cutmix_ref.py's (test infrastructure as well, typed in from include/slk.h); what is new is
stated here from the header's rule:

  h3..h7 of the PRIMARY sample:  apply = h3 < prob * 2^32
                                 cut   = both tables ? h4 < switch * 2^32 : (cut_table is given)
                                 k     = h5 >> 22;  cy = (h6 * H) >> 32;  cx = (h7 * W) >> 32
  CutMix sample (apply and cut):     side = (cut_table[k] * H) >> 32, then cutmix_ref's box, selection and label
  MixUp sample  (apply and not cut): wb = lam_table[k]; per pixel, in float32 with every operation rounded on its own,
                                     f = (1 - wb) * (pa / 255) + wb * (pb / 255);  x = (f - mean) / std
                                     y = a | b << 8 | bits(wb) << 32 if wb > 0 else a
  otherwise:                         sample i alone, the plain label

numpy's float32 array arithmetic rounds every elementwise operation on its own, which is the rule. The three WRONG
variants a kernel could compute instead (an fma, the lerp form, a blend after Normalize) are here too, so that the CPU
tests can show the GPU comparison's inputs tell them apart."""
import numpy as np

import cutmix_ref as M

TABLE = 1024
DENORMAL = np.float32(1e-42)
BELOW_ONE = np.nextafter(np.float32(1), np.float32(0))
HAND_VALUES = np.array([0.0, DENORMAL, np.float32(1) / np.float32(3), 0.2, 0.5, 0.9, BELOW_ONE, 1.0], dtype=np.float32)


def hand_table():
    """The hand-made lam_table of the GPU tests: entry k holds HAND_VALUES[k % 8], so every sample draws one of them."""
    return HAND_VALUES[np.arange(TABLE) % len(HAND_VALUES)].copy()


def draw_one(i, epoch, seed, H, W, prob, switch, cut_table, lam_table):
    """(mode, k, y1, y2, x1, x2, area, wb) of dataset index i; mode is 'cut', 'blend' or 'plain'. The box is empty
    and area 0 unless mode is 'cut'; wb is the label weight (np.float32)."""
    assert cut_table is not None or lam_table is not None
    h = M.chain(i, epoch, seed, 8)
    apply = h[3] < int(prob * 4294967296.0)
    cut = h[4] < int(switch * 4294967296.0) if (cut_table is not None and lam_table is not None) else cut_table is not None
    k = h[5] >> 22
    cy, cx = (h[6] * H) >> 32, (h[7] * W) >> 32
    if apply and cut:
        side = (int(cut_table[k]) * H) >> 32
        half = side // 2
        y1, y2 = M.clip(cy - half, 0, H), M.clip(cy + half, 0, H)
        x1, x2 = M.clip(cx - half, 0, W), M.clip(cx + half, 0, W)
        area = (y2 - y1) * (x2 - x1)
        return "cut", k, y1, y2, x1, x2, area, np.float32(area) / np.float32(H * W)
    if apply:
        return "blend", k, 0, 0, 0, 0, 0, np.float32(lam_table[k])
    return "plain", k, 0, 0, 0, 0, 0, np.float32(0)


def shown(img, draws, pad):
    """The u8 image [C,H,W] sample `img` shows under its (dy, dx, flip), pixel by pixel."""
    C, H, W = img.shape
    out = np.zeros((C, H, W), dtype=np.uint8)
    for yo in range(H):
        for xo in range(W):
            for c in range(C):
                out[c, yo, xo] = M.source_pixel(img, c, yo, xo, draws[0], draws[1], draws[2], pad)
    return out


def blend(pa, pb, wb):
    """THE RULE: float32 (1 - wb) * (pa / 255) + wb * (pb / 255), each operation rounded on its own."""
    wb = np.float32(wb)
    fa = pa.astype(np.float32) / np.float32(255)
    fb = pb.astype(np.float32) / np.float32(255)
    om = np.float32(1) - wb
    return (om * fa).astype(np.float32) + (wb * fb).astype(np.float32)


def blend_contracted(pa, pb, wb):
    """WRONG: fma(om, fa, wb * fb), what a contracting compiler makes of the rule (the product om * fa is exact in
    float64, so one float64 sum and one rounding to float32 is the fma up to a double rounding)."""
    wb = np.float32(wb)
    fa = pa.astype(np.float32) / np.float32(255)
    fb = pb.astype(np.float32) / np.float32(255)
    om = np.float32(1) - wb
    p = (wb * fb).astype(np.float32)
    return (om.astype(np.float64) * fa.astype(np.float64) + p.astype(np.float64)).astype(np.float32)


def blend_lerp(pa, pb, wb):
    """WRONG: fa + wb * (fb - fa)."""
    wb = np.float32(wb)
    fa = pa.astype(np.float32) / np.float32(255)
    fb = pb.astype(np.float32) / np.float32(255)
    return fa + (wb * (fb - fa)).astype(np.float32)


def normalize(f, mean, std):
    m = np.asarray(mean, dtype=np.float32).reshape(-1, 1, 1)
    sd = np.asarray(std, dtype=np.float32).reshape(-1, 1, 1)
    return ((f.astype(np.float32) - m) / sd).astype(np.float32)


def blend_after_normalize(pa, pb, wb, mean, std):
    """WRONG: Normalize each source, then blend."""
    wb = np.float32(wb)
    xa = normalize(pa.astype(np.float32) / np.float32(255), mean, std)
    xb = normalize(pb.astype(np.float32) / np.float32(255), mean, std)
    return ((np.float32(1) - wb) * xa).astype(np.float32) + (wb * xb).astype(np.float32)


def batch(images, labels, idx, idx2, mean, std, cut_table=None, lam_table=None, prob=1.0, switch=0.5, pad=0,
          flip=False, seed=0, epoch=0, info=None):
    """(x f32 [B,C,H,W], y i64 [B]) of slk_image_batch_blend; `info` (a list) receives each position's draw_one."""
    if images.ndim == 3:
        images = images[:, None]
    _, C, H, W = images.shape
    x = np.zeros((len(idx), C, H, W), dtype=np.float32)
    y = np.zeros(len(idx), dtype=np.int64)
    for s, (i, i2) in enumerate(zip(idx, idx2)):
        i, i2 = int(i), int(i2)
        mode, k, y1, y2, x1, x2, area, wb = d = draw_one(i, epoch, seed, H, W, prob, switch, cut_table, lam_table)
        if info is not None:
            info.append(d)
        pa = shown(images[i], M.crop_one(i, epoch, seed, pad, flip), pad)
        a, b = int(labels[i]), int(labels[i2])
        if mode == "plain":
            x[s], y[s] = normalize(pa.astype(np.float32) / np.float32(255), mean, std), a
            continue
        pb = shown(images[i2], M.crop_one(i2, epoch, seed, pad, flip), pad)
        if mode == "cut":
            u8 = pa.copy()
            for yo in range(y1, y2):
                for xo in range(x1, x2):
                    u8[:, yo, xo] = pb[:, yo, xo]
            x[s] = normalize(u8.astype(np.float32) / np.float32(255), mean, std)
            y[s] = M.pack(a, b, wb) if area > 0 else a
        else:
            x[s] = normalize(blend(pa, pb, wb), mean, std)
            y[s] = M.pack(a, b, wb) if wb > 0 else a
    return x, y


def all_pairs():
    """pa, pb u8 [1, 256, 256]: every (pa, pb) pair once."""
    v = np.arange(256, dtype=np.uint8)
    return np.repeat(v, 256).reshape(1, 256, 256), np.tile(v, 256).reshape(1, 256, 256)


# ------------------------------------------------------------------------------------ what the GPU tests run on
N = 2048          # synthetic dataset rows; rows 0 and N - 1 are all 0 / all 255
B = 33            # batch: more than one block and a ragged tail in both instantiations
SHAPES = {"cifar": dict(shape=(3, 32, 32), pad=4, mean=(0.4914, 0.4822, 0.4465), std=(0.2470, 0.2435, 0.2616)),
          "mnist": dict(shape=(1, 28, 28), pad=2, mean=(0.1307,), std=(0.3081,))}


def dataset(name):
    img, lbl = M.synthetic(N, SHAPES[name]["shape"], 21)
    img[0], img[N - 1] = 0, 255
    return img, lbl


def draws(H, W, pad, epoch=0, seed=0, prob=1.0, switch=0.5, cut_table=None, lam_table=None, flip=True, n=N):
    """The draws of dataset rows 0 .. n-1 as arrays: mode ('cut' / 'blend' / 'plain'), k, y1, y2, x1, x2, area, wb,
    and the crop's dy, dx, fl."""
    rows = [draw_one(i, epoch, seed, H, W, prob, switch, cut_table, lam_table) for i in range(n)]
    crops = np.array([M.crop_one(i, epoch, seed, pad, flip) for i in range(n)], dtype=np.int64)
    d = {name: np.array([r[j] for r in rows]) for j, name in
         enumerate(("mode", "k", "y1", "y2", "x1", "x2", "area", "wb"))}
    d["wb"] = d["wb"].astype(np.float32)
    d.update(dy=crops[:, 0], dx=crops[:, 1], fl=crops[:, 2])
    return d


def fill(idx, idx2):
    """Both lists padded to a multiple of B (at least two batches) with ordinary rows."""
    n = max(2 * B, -(-len(idx) // B) * B) - len(idx)
    return np.concatenate([idx, np.arange(100, 100 + n)]).astype(np.int64), \
        np.concatenate([idx2, np.arange(300, 300 + n)]).astype(np.int64)


def pick_cut(d, W):
    """(idx, idx2) for case (a): every reachable (x1 % 4, x2 % 4) of a non-empty box under every (flip_i, flip_i2),
    a box on each border, an empty applied box, and dataset rows 0 and N - 1 on both sides. Asserts the coverage."""
    allidx = np.arange(N)
    full = (d["mode"] == "cut") & (d["area"] > 0)
    x1, x2, y1, y2, fl = d["x1"], d["x2"], d["y1"], d["y2"], d["fl"]
    H = W
    pairs = {(int(a) % 4, int(b) % 4) for a, b in zip(x1[full], x2[full])}
    want = {(p, q) for p in range(4) for q in range(4) if p % 2 == q % 2} | {(0, 1), (0, 3), (1, W % 4), (3, W % 4)}
    assert pairs == want and len(want) == 12, sorted(pairs)
    by_flip = {f: [int(i) for i in allidx[fl == f]] for f in (0, 1)}
    idx, idx2, k = [], [], 0
    for p, q in sorted(want):
        for fi in (0, 1):
            for f2 in (0, 1):
                c = allidx[full & (x1 % 4 == p) & (x2 % 4 == q) & (fl == fi)]
                assert len(c), f"no sample with box columns ({p}, {q}) mod 4 and flip {fi}"
                idx.append(int(c[k % len(c)]))
                idx2.append(by_flip[f2][(7 * k + 3) % len(by_flip[f2])])
                k += 1
    for cond in (full & (y1 == 0), full & (y2 == H), full & (x1 == 0), full & (x2 == W), (d["mode"] == "cut") & ~full):
        assert cond.sum() >= 1
        idx.append(int(allidx[cond][0]))
        idx2.append(int(allidx[cond][-1]))
    idx += [0, N - 1, 5, 6]
    idx2 += [9, 10, 0, N - 1]
    cases = {(int(x1[i]) % 4, int(x2[i]) % 4, int(fl[i]), int(fl[j])) for i, j in zip(idx, idx2) if full[i]}
    assert len(cases) == 48
    return fill(idx, idx2)


def pick_blend(d, pad):
    """(idx, idx2) for case (b), on a table made by hand_table(): every hand value under every (flip_i, flip_i2),
    every crop offset dx and dy of the primary and of the partner (so, at pad = 4, quads and rows that lie wholly in
    either source's padding), and dataset rows 0 and N - 1 on both sides. Asserts the coverage."""
    allidx = np.arange(N)
    assert (d["mode"] == "blend").all()
    fl, dx, dy, wb = d["fl"], d["dx"], d["dy"], d["wb"]
    by_flip = {f: allidx[fl == f] for f in (0, 1)}
    idx, idx2, k = [], [], 0
    for v in HAND_VALUES:
        for fi in (0, 1):
            for f2 in (0, 1):
                c = allidx[(wb.view(np.uint32) == np.float32(v).view(np.uint32)) & (fl == fi)]
                assert len(c), f"no sample drawing {v} with flip {fi}"
                idx.append(int(c[k % len(c)]))
                idx2.append(int(by_flip[f2][(7 * k + 3) % len(by_flip[f2])]))
                k += 1
    telling = np.isin(wb.view(np.uint32), HAND_VALUES[[2, 3, 5]].view(np.uint32))   # 1/3, 0.2, 0.9
    for j in range(2 * pad + 1):         # offsets: the primary runs up, the partner down, in x and then in y
        for key in (dx, dy):
            c, c2 = allidx[telling & (key == j)], allidx[key == 2 * pad - j]
            assert len(c) and len(c2)
            idx.append(int(c[j % len(c)]))
            idx2.append(int(c2[(3 * j + 1) % len(c2)]))
    idx += [0, N - 1, 5, 6]
    idx2 += [9, 10, 0, N - 1]
    got = {(int(wb[i].view(np.uint32)), int(fl[i]), int(fl[j])) for i, j in zip(idx, idx2)}
    assert len({g for g in got if g[0] in set(HAND_VALUES.view(np.uint32).tolist())}) >= 32
    for key in (dx, dy):
        assert {int(key[i]) for i in idx} == set(range(2 * pad + 1)) == {int(key[j]) for j in idx2}
    return fill(idx, idx2)


def pick_switch(d):
    """(idx, idx2) for case (c): each of the three modes under all four flip pairs, filled to one batch of B."""
    allidx = np.arange(N)
    fl = d["fl"]
    idx, idx2, k = [], [], 0
    for mode in ("cut", "blend", "plain"):
        for fi in (0, 1):
            for f2 in (0, 1):
                ok = (d["mode"] == mode) & (fl == fi)
                if mode == "cut":
                    ok &= d["area"] > 0
                c, c2 = allidx[ok], allidx[fl == f2]
                assert len(c) >= 100, (mode, fi, len(c))
                idx.append(int(c[(5 * k + 1) % len(c)]))
                idx2.append(int(c2[(7 * k + 3) % len(c2)]))
                k += 1
    cases = {(str(d["mode"][i]), int(fl[i]), int(fl[j])) for i, j in zip(idx, idx2)}
    assert len(cases) == 12
    rest = allidx[200:200 + B - len(idx)]
    return np.array(idx + list(rest)), np.array(idx2 + list(np.roll(rest, 1)))
