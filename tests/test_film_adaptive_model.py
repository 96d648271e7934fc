"""tests/film_adaptive_model.py against itself, against tests/film_model.py and against the C ABI's host helpers (no GPU)."""
import ctypes as C

import numpy as np
import pytest

import film_adaptive_model as am
import film_model as fm

f32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


# ------------------------------------------------------------------------------------------------ tile map, packed order
def test_the_tile_map_of_72x40_in_16x16_tiles():
    t = am.Tiling(72, 40, 16, 16)
    assert (t.tiles_x, t.tiles_y, t.n_tiles) == (5, 3, 15)
    assert t.rect(0) == (0, 0, 16, 16) and t.rect(4) == (64, 0, 8, 16) and t.rect(10) == (0, 32, 16, 8) and t.rect(14) == (64, 32, 8, 8)
    assert sum(len(t.pixels(k)) for k in range(15)) == 72 * 40
    everything = t.pixel_map(range(15))
    assert sorted(everything) == list(range(72 * 40))          # every pixel once
    assert list(t.pixels(14)[:9]) == [32 * 72 + 64 + i for i in range(8)] + [33 * 72 + 64]   # row-major inside the clipped tile
    m = t.pixel_map([3, 14])
    assert np.array_equal(m, np.concatenate([t.pixels(3), t.pixels(14)])) and len(m) == 256 + 64
    assert not t.check_list([]) and not t.check_list([3, 3]) and not t.check_list([4, 3]) and not t.check_list([15])
    assert t.check_list([0]) and t.check_list([0, 7, 14])


@pytest.mark.parametrize("shape", ((72, 40, 16, 16), (70, 50, 32, 8), (64, 48, 0, 0), (33, 17, 8, 32)))
def test_pt_tiles_pixel_map_is_the_models(pta, shape):
    """The host helper through the C ABI (no GPU work): every list the model accepts, and the refusals."""
    w, h, tw, th = shape
    t = am.Tiling(w, h, tw or 32, th or 32)
    prof, opts = pta.Profile.make(w, h, 1, 1), pta.Opts.make(tile_w=tw, tile_h=th)
    rng = np.random.default_rng(w * h)
    lists = [[0], [t.n_tiles - 1], list(range(0, t.n_tiles, 2)), list(range(t.n_tiles))]
    lists += [sorted(rng.choice(t.n_tiles, size=min(t.n_tiles, 3), replace=False).tolist())]
    for tiles in lists:
        want = t.pixel_map(tiles)
        assert pta.tiles_pixel_count(prof, tiles, opts) == len(want), tiles
        assert np.array_equal(pta.tiles_pixel_map(prof, tiles, opts), want), tiles
    assert np.array_equal(pta.tiles_pixel_map(prof, range(t.n_tiles), opts)[np.argsort(t.pixel_map(range(t.n_tiles)))],
                          np.arange(w * h))
    lib = pta.gpu_lib()
    out = np.full(w * h, 0xA5A5A5A5, np.uint32)
    for bad in ([], [t.n_tiles], [0, 0], [1, 0]):
        arr = np.asarray(bad, np.uint32)
        assert pta.tiles_pixel_count(prof, bad, opts) == 0, bad
        assert lib.pt_tiles_pixel_map(C.byref(prof), C.byref(opts), arr.ctypes.data, len(arr), out.ctypes.data) == pta.PT_ERR_INVALID
    one = np.zeros(1, np.uint32)
    assert lib.pt_tiles_pixel_map(C.byref(prof), C.byref(opts), None, 1, out.ctypes.data) == pta.PT_ERR_INVALID
    assert lib.pt_tiles_pixel_map(C.byref(prof), C.byref(opts), one.ctypes.data, 1, None) == pta.PT_ERR_INVALID
    sharded = pta.Opts.make(tile_w=tw, tile_h=th, shard_count=2)
    assert lib.pt_tiles_pixel_map(C.byref(prof), C.byref(sharded), one.ctypes.data, 1, out.ctypes.data) == pta.PT_ERR_INVALID
    assert (out == 0xA5A5A5A5).all()


# ------------------------------------------------------------------------------------------------ scatter-merge
def test_the_merge_touches_the_listed_tiles_only():
    t = am.Tiling(72, 40, 16, 16)
    n = t.n_pixels
    acc, mom = fm.synthetic_planes(n, 6, 1)
    counts = np.full(n, 6, np.uint32)
    tiles = [1, 4, 14]
    where = t.pixel_map(tiles)
    p_acc, p_mom = fm.synthetic_planes(len(where), 12, 2)
    acc2, mom2, cnt2 = am.merge_tiles(t, acc, mom, counts, tiles, p_acc, p_mom, 12)
    rest = np.setdiff1d(np.arange(n), where)
    assert np.array_equal(bits(acc2[rest]), bits(acc[rest])) and np.array_equal(bits(mom2[rest]), bits(mom[rest]))
    assert (cnt2[rest] == 6).all() and (cnt2[where] == 18).all()
    assert np.array_equal(bits(acc2[where]), bits(fm.merge(acc[where], p_acc)))
    assert np.array_equal(bits(mom2[where]), bits(fm.merge(mom[where], p_mom)))
    # a pass that lists every tile is film_model's merge, pixel for pixel
    every = t.pixel_map(range(t.n_tiles))
    f_acc, f_mom = fm.synthetic_planes(n, 12, 3)
    acc3, mom3, cnt3 = am.merge_tiles(t, acc, mom, counts, range(t.n_tiles), f_acc[every], f_mom[every], 12)
    assert np.array_equal(bits(acc3), bits(fm.merge(acc, f_acc))) and np.array_equal(bits(mom3), bits(fm.merge(mom, f_mom)))
    assert (cnt3 == 18).all()


# ------------------------------------------------------------------------------------------------ the tile-noise tree
def test_a_full_tile_of_256_is_the_block_tree_bit_for_bit():
    rng = np.random.default_rng(7)
    for _ in range(20):
        err = rng.uniform(0, 3, 256).astype(f32) * f32(10.0) ** rng.integers(-6, 3, 256).astype(f32)
        s, m = am.tile_tree(err)
        bs, bm = fm.blocks(err)
        assert bits(s) == bits(bs[0]) and bits(m) == bits(bm[0])
    # ... and a 16 x 16 tile of an image: the tile's pixels in the order j are the block's packed pixels
    t = am.Tiling(72, 40, 16, 16)
    _, mom = fm.synthetic_planes(t.n_pixels, 14, 9)
    err = fm.pixel_error(mom, 14)
    assert np.array_equal(bits(am.pixel_error(mom, np.full(t.n_pixels, 14, np.uint32))), bits(err))
    tsum, tmax = am.tile_arrays(t, err)
    for k in (0, 6, 8):
        bs, bm = fm.blocks(err[t.pixels(k)])
        assert bits(tsum[k]) == bits(bs[0]) and bits(tmax[k]) == bits(bm[0])


@pytest.mark.parametrize("P", (64, 128, 1024))
def test_clipped_and_large_tiles(P):
    """P < 256: the threads beyond P hold 0.f, the tree adds it.  P = 1024: every thread adds four errors, in the order j,
    before the tree - not what a tree over 1024 leaves gives."""
    rng = np.random.default_rng(P)
    err = (rng.uniform(0, 2, P).astype(f32) * f32(10.0) ** rng.integers(-5, 2, P).astype(f32)).astype(f32)
    s, m = am.tile_tree(err)
    v = np.zeros(256, f32)
    for i in range(256):
        for j in range(i, P, 256):
            v[i] = f32(v[i] + err[j])
    stride = 128
    while stride:
        for i in range(stride):
            v[i] = f32(v[i] + v[i + stride])
        stride //= 2
    assert bits(s) == bits(v[0]) and bits(m) == bits(err.max())
    if P < 256:
        bs, _ = fm.blocks(err)     # a clipped tile is a partial block: the padding is the same 0.f
        assert bits(s) == bits(bs[0])
    assert abs(float(s) - float(err.astype(np.float64).sum())) <= 1e-5 * float(err.sum())


def test_the_statistics_are_f64_over_the_tiles():
    t = am.Tiling(72, 40, 16, 16)
    _, mom = fm.synthetic_planes(t.n_pixels, 14, 4)
    counts = np.full(t.n_pixels, 14, np.uint32)
    counts[t.pixels(7)] = 30
    st, err, tsum, tmax = am.tile_noise(t, mom, counts, 0.3)
    means = [float(tsum[k]) / len(t.pixels(k)) for k in range(15)]
    assert st["max_tile_error"] == max(means) and st["over_tiles"] == sum(m > 0.3 for m in means)
    assert st["mean_error"] == sum(float(x) for x in tsum) / (72 * 40)
    assert st["samples"] == 30 and st["pixel_samples"] == 14 * (72 * 40 - 256) + 30 * 256
    assert st["converged"] == int(st["over_tiles"] == 0) and st["n_tiles"] == 15
    # a pixel's error depends on its own count
    other = am.pixel_error(mom, np.full(t.n_pixels, 14, np.uint32))
    inside = t.pixels(7)
    assert not np.array_equal(bits(err[inside]), bits(other[inside]))
    assert np.array_equal(bits(np.delete(err, inside)), bits(np.delete(other, inside)))
    assert np.array_equal(bits(err[inside]), bits(fm.pixel_error(mom[inside], 30)))


# ------------------------------------------------------------------------------------------------ candidates, dilation
def test_dilation_at_the_corners_and_edges():
    t = am.Tiling(72, 40, 16, 16)   # 5 x 3 tiles
    assert am.dilate(t, [0]) == [0, 1, 5, 6]
    assert am.dilate(t, [4]) == [3, 4, 8, 9]
    assert am.dilate(t, [10]) == [5, 6, 10, 11]
    assert am.dilate(t, [14]) == [8, 9, 13, 14]
    assert am.dilate(t, [7]) == [1, 2, 3, 6, 7, 8, 11, 12, 13]
    assert am.dilate(t, [2]) == [1, 2, 3, 6, 7, 8]
    assert am.dilate(t, [0, 14]) == [0, 1, 5, 6, 8, 9, 13, 14]
    assert am.dilate(t, [0, 14], 0) == [0, 14] and am.dilate(t, []) == []
    assert am.dilate(am.Tiling(16, 16, 16, 16), [0]) == [0]
    tsum = np.zeros(15, f32)
    tsum[14] = f32(64 * 0.04)      # the 8 x 8 corner tile: a mean of 0.04 over its 64 pixels
    tsum[7] = f32(256 * 0.02)
    assert am.candidates(t, tsum, 0.03) == [14] and am.candidates(t, tsum, 0.01) == [7, 14]
    assert am.candidates(t, tsum, float(tsum[14]) / 64) == []     # strictly above
    assert am.next_active(t, tsum, 0.03, 1) == [8, 9, 13, 14] and am.next_active(t, tsum, 0.03, 0) == [14]


# ------------------------------------------------------------------------------------------------ the schedule
def test_the_schedule_stops_for_budget_or_converged():
    t = am.Tiling(72, 40, 16, 16)
    every = list(range(15))

    def noise(levels):
        """tile_sum after pass k: tile 7 and the corner tile 14 stay above 0.03 for levels[k] = 2, tile 7 alone for 1."""
        def after(k, samples, tiles):
            s = np.zeros(15, f32)
            if levels[k] >= 1:
                s[7] = f32(256 * 0.05)
            if levels[k] >= 2:
                s[14] = f32(64 * 0.05)
            return s
        return after
    # never clean: 8, 16, 32 fit 56, the fourth pass (64) does not
    made, why = am.render_until_adaptive(t, noise([2, 2, 1, 1]), 8, 8, 0, 0.03, 56)
    assert why == "budget" and [m[0] for m in made] == [8, 16, 32] == fm.schedule(8, 56)
    assert [m[1] for m in made] == [every, [7, 14], [7, 14]]
    made, why = am.render_until_adaptive(t, noise([2, 2, 1, 1]), 8, 8, 1, 0.03, 56)
    assert [m[1] for m in made] == [every, am.dilate(t, [7, 14]), am.dilate(t, [7, 14])]
    # clean after the second pass
    made, why = am.render_until_adaptive(t, noise([2, 0]), 8, 8, 0, 0.03, 1 << 30)
    assert why == "converged" and [m[0] for m in made] == [8, 16] and made[1][1] == [7, 14]
    # every tile until the largest count reaches uniform_samples: 8 and 8 + 16 = 24 are below 25
    made, why = am.render_until_adaptive(t, noise([2, 2, 2, 1, 0]), 8, 25, 0, 0.03, 1 << 30)
    assert why == "converged" and [m[1] for m in made] == [every, every, every, [7, 14], [7]]
    # clean at once; no pass fits
    assert am.render_until_adaptive(t, noise([0]), 8, 8, 1, 0.03, 56) == ([(8, every)], "converged")
    assert am.render_until_adaptive(t, noise([0]), 8, 8, 1, 0.03, 7) == ([], "budget")
    # the cap of 2^24 holds whatever max_samples says
    made, why = am.render_until_adaptive(t, noise([1] * 40), 1 << 22, 0, 0, 0.03, 1 << 40)
    assert why == "budget" and [m[0] for m in made] == [1 << 22, 1 << 23]
