"""CPU: the arithmetic behind the batches of tests/test_steady_exact_gpu.py. Every statement its docstring makes
about a batch - how many workgroups walk how many units, how many samples a range spans, which ring slots are
refilled, which K5 shares own a third tile - is computed here from tests/unit_partition.py (the launch code's
partitions restated) and asserted literally, so that docstring rests on executed arithmetic."""
import pytest

import unit_partition as P


# ----------------------------------------------------------------------------- K2: ranges by length
@pytest.mark.parametrize("B,per,counts", [
    (130, 2, {2: 195, 0: 61}),                 # where the older exact tests stop
    (171, 3, {3: 171, 0: 85}),
    (258, 4, {4: 193, 2: 1, 0: 62}),
    (342, 5, {5: 205, 1: 1, 0: 50}),
    (512, 6, {6: 256}),
    (513, 7, {7: 219, 6: 1, 0: 36}),
])
def test_x3_ranges_by_length(B, per, counts):
    """Forward (x3, x3s, x3i, x3p), dgrad pairs and the images-fed weight gradient share one partition from
    B = 43 on (min(3 B, 256) = min(6 B, 256) = 256)."""
    for f in (P.x3_fwd, P.x3_dgrad, P.x3_wgrad_images):
        got_per, ranges = f(B)
        assert got_per == per and len(ranges) == 256
        assert P.length_counts(ranges) == counts
        assert sum(u1 - u0 for u0, u1 in ranges) == 3 * B
        assert all(a[1] == b[0] for a, b in zip(ranges, ranges[1:]) if b[1] > b[0])      # contiguous, in order


@pytest.mark.parametrize("B,per,counts", [
    (130, 4, {4: 97, 2: 1, 0: 30}),
    (171, 5, {5: 102, 3: 1, 0: 25}),
    (258, 7, {7: 110, 4: 1, 0: 17}),
    (342, 9, {9: 114, 0: 14}),
])
def test_x3_wgrad_f32_ranges(B, per, counts):
    got_per, ranges = P.x3_wgrad_f32(B)
    assert got_per == per and len(ranges) == 128
    assert P.length_counts(ranges) == counts


@pytest.mark.parametrize("B,per,counts", [
    (130, 3, {3: 130}),
    (171, 3, {3: 171}),
    (258, 6, {6: 129, 0: 127}),     # NOT "per = 6 in two workgroups": every busy workgroup takes two whole samples
    (342, 6, {6: 171, 0: 85}),
    (512, 6, {6: 256}),
])
def test_x3_amax_forward_ranges(B, per, counts):
    got_per, ranges = P.x3_fwd_amax(B)
    assert got_per == per and len(ranges) == min(B, 256)
    assert P.length_counts(ranges) == counts
    assert all(u0 % 3 == 0 and u1 % 3 == 0 for u0, u1 in ranges)                         # whole samples


# ----------------------------------------------------------------------------- K2: sample spans
@pytest.mark.parametrize("B,images,f32", [(130, 2, 2), (171, 1, 3), (258, 2, 3), (342, 3, 3)])
def test_sample_spans(B, images, f32):
    """The largest number of samples one K share touches: three distinct dY scales meet in one share of the
    images-fed weight gradient (its LDS table sbt holds three entries) first at per = 5, B = 342; the f32-act
    kernel's shares (128 of them) span three samples from B = 171."""
    assert P.sample_span(P.x3_wgrad_images(B)[1]) == images
    assert P.sample_span(P.x3_wgrad_f32(B)[1]) == f32
    if B == 342:                                # the share that the issue names: units 5..9 = samples 1, 2, 3
        assert P.x3_wgrad_images(B)[1][1] == (5, 10)
    if B == 171:                                # f32 act: units 5..9 too
        assert P.x3_wgrad_f32(B)[1][1] == (5, 10)


def test_a_four_unit_range_never_spans_three_samples():
    assert P.sample_span(P.x3_fwd(258)[1]) == 2 and P.sample_span(P.x3_fwd(512)[1]) == 2


# ----------------------------------------------------------------------------- K2: buffers and ring
@pytest.mark.parametrize("B,refills,workgroups", [
    (130, [], 195), (171, [], 171),
    (258, [0], 193),                            # the first real refill: slot 0, read again at position 3
    (342, [0, 1], 205),
    (512, [0, 1, 2], 256),                      # every slot refilled once: the ring's full turn
])
def test_x3i_ring_refills(B, refills, workgroups):
    got = P.x3i_refills([r for r in P.x3_fwd(B)[1] if r[1] > r[0]])                     # the busy workgroups
    assert sum(1 for r in got if r == refills) == workgroups
    assert max(got, key=len) == refills


@pytest.mark.parametrize("B,third", [(130, 0), (171, 171), (258, 193), (342, 205), (512, 256)])
def test_two_slot_buffers_are_reused_from_the_third_unit(B, third):
    """dgrad's x / ReLU-bit and mask-word buffers ((q + 1) & 1), the forward's raw rows (k & 1) and the images-fed
    weight gradient's image buffers (k & 1): the unit at position 2 is the first to read a refilled buffer."""
    ranges = P.x3_dgrad(B)[1]
    assert sum(1 for u0, u1 in ranges if u1 - u0 >= 3) == third
    a, b = P.lag_pairs(ranges, lags=(2,))
    assert (len(a) > 0) == (third > 0)
    assert all(x - y == 2 for x, y in zip(a, b))


def test_lag_pairs_stay_inside_a_range():
    ranges = P.x3_fwd(258)[1]
    a, b = P.lag_pairs(ranges)
    owner = {u: i for i, (u0, u1) in enumerate(ranges) for u in range(u0, u1)}
    assert all(owner[x] == owner[y] and x - y in (2, 3) for x, y in zip(a, b))
    assert len(a) == 193 * (2 + 1)              # a range of 4: positions 2 and 3 look back 2, position 3 looks back 3


# ----------------------------------------------------------------------------- direct and Winograd presets
@pytest.mark.parametrize("B,samples,super_units", [
    (130, {1: 130}, {1: 195}),
    (258, {2: 2, 1: 254}, {2: 131, 1: 125}),            # the Winograd forward: at most two super-units
    (513, {3: 1, 2: 255}, {4: 2, 3: 254}),              # sample 512 is workgroup 0's third; 770 super-units
])
def test_strided_presets(B, samples, super_units):
    assert P.length_counts(P.strided(B, 256)) == samples
    assert P.length_counts(P.wino_fwd(B)) == super_units


# ----------------------------------------------------------------------------- K5 weight gradients
def test_wgcfg_constants():
    assert (P.wg_rb(P.WG2), P.wg_ksplit(P.WG2)) == (8, 256)
    assert (P.wg_rb(P.WG3), P.wg_ksplit(P.WG3)) == (2, 64)
    # tile slots per group of 8 images
    assert 8 * P.wg_rb(P.WG2) == 64 and 8 * P.wg_rb(P.WG3) == 16


@pytest.mark.parametrize("cfg", [P.WG2, P.WG3])
def test_tile_of_covers_every_image_row_block_once(cfg):
    B = 24
    seen = [P.tile_of(cfg, t) for t in range(3 * 8 * P.wg_rb(cfg))]
    assert sorted(seen) == [(n, rb) for n in range(B) for rb in range(P.wg_rb(cfg))]


K5_CASES = [(P.WG2, 9), (P.WG2, 37), (P.WG2, 65), (P.WG2, 131), (P.WG2, 261),
            (P.WG3, 9), (P.WG3, 37), (P.WG3, 131), (P.WG3, 261)]


@pytest.mark.parametrize("cfg,B", K5_CASES)
def test_share_slots_are_valid_then_invalid(cfg, B):
    """The kernel stops at a share's first invalid slot; that loses no tile only if validity is monotone along
    the share's slot list. Every (image, row block) is then walked exactly once."""
    K = P.wg_ksplit(cfg)
    rounds = P.ceil_div(8 * P.ceil_div(B, 8) * P.wg_rb(cfg), K) + 2
    walked = []
    for ks in range(K):
        v = P.share_slots(cfg, ks, B, rounds)
        assert v == sorted(v, reverse=True), (ks, v)
        tiles = P.share_tiles(cfg, ks, B)
        assert len(tiles) == sum(v)
        walked += [P.tile_of(cfg, t) for t in tiles]
    assert sorted(walked) == [(n, rb) for n in range(B) for rb in range(P.wg_rb(cfg))]


@pytest.mark.parametrize("cfg,B,counts", [
    (P.WG2, 9, {0: 184, 1: 72}), (P.WG2, 37, {1: 216, 2: 40}),                    # the older exact cases: <= 2 tiles
    (P.WG3, 9, {0: 46, 1: 18}), (P.WG3, 37, {1: 54, 2: 10}),
    (P.WG2, 65, {2: 248, 3: 8}),
    (P.WG2, 131, {4: 232, 5: 24}), (P.WG2, 261, {8: 216, 9: 40}),
    (P.WG3, 131, {4: 58, 5: 6}), (P.WG3, 261, {8: 54, 9: 10}),
])
def test_tiles_per_share(cfg, B, counts):
    K = P.wg_ksplit(cfg)
    assert P.length_counts([(0, len(P.share_tiles(cfg, ks, B))) for ks in range(K)]) == counts


def test_conv2_third_tile_at_65():
    """B = 65: image 64 alone opens the third round; its 8 row blocks are slots 512, 520, ..., 568, i.e. shares
    0, 8, ..., 56: the only ones whose `valid(t + 2 * KSPLIT)` is ever true."""
    third = [ks for ks in range(256) if len(P.share_tiles(P.WG2, ks, 65)) == 3]
    assert third == list(range(0, 64, 8))
    assert [P.tile_of(P.WG2, ks + 512) for ks in third] == [(64, rb) for rb in range(8)]
    assert all(len(P.share_tiles(P.WG2, ks, 64)) == 2 for ks in range(256))       # B = 64: no third tile anywhere
