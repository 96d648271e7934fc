"""Sharded films without a GPU: tests/film_shard_model.py against pt_local_pixel_map, the model's lock-step loop
against the model's unsharded loop, and what the command line refuses around --film-devices.  pt_film_select_tiles is a pure
host function, but it takes a film, and a film lives on a device: that one test is marked gpu."""
import subprocess

import numpy as np
import pytest

import film_adaptive_model as am
import film_model as fm
import film_shard_model as sm
from conftest import ROOT, SCENES

f32 = np.float32
SHAPES = ((72, 40, 16, 16), (70, 50, 32, 8))   # 5 x 3 tiles with a clipped last column and row; 3 x 7 tiles of 32 x 8
EXE = ROOT / "path-tracer_amd" / "path-tracer"
SCENE = SCENES / "cube" / "scene.isf"


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, f32), np.ascontiguousarray(b, f32)
    return a.shape == b.shape and bool((a.view(np.uint32) == b.view(np.uint32)).all())


def test_the_rule_restated():
    assert [sm.rank_stride(n) for n in (1, 2, 3, 4, 5, 6, 8, 9, 15)] == [1, 1, 5, 3, 3, 5, 3, 5, 7]
    t = am.Tiling(72, 40, 16, 16)
    assert [sm.tile_rank(t, k, 2) for k in range(15)] == [(k % 5 + k // 5) % 2 for k in range(15)]
    assert [sm.tile_rank(t, k, 3) for k in range(15)] == [(k % 5 + 5 * (k // 5)) % 3 for k in range(15)]


@pytest.mark.parametrize("shape", SHAPES, ids=("72x40 in 16x16", "70x50 in 32x8"))
@pytest.mark.parametrize("count", (1, 2, 3, 8))
def test_the_models_map_is_pt_local_pixel_map(pta, shape, count):
    w, h, tw, th = shape
    t = am.Tiling(w, h, tw, th)
    seen = np.zeros(t.n_pixels, np.uint32)
    owners = []
    for rank in range(count):
        s = sm.Shard(t, rank, count)
        opts = pta.Opts.make(tile_w=tw, tile_h=th, shard_rank=rank, shard_count=count)
        want = pta.local_pixel_map(pta.Profile.make(w, h, 1, 2), opts)
        assert np.array_equal(s.map, want), (count, rank)
        seen[s.map] += 1
        owners.append(s.tiles)
        # packed offsets: a tile's pixels sit at base + j in the order j = y * cw + x
        if count > 1:
            for k in s.tiles:
                assert np.array_equal(s.map[s.base(k):s.base(k) + len(t.pixels(k))], t.pixels(k))
            assert s.offsets[-1] == s.n_local and all(s.base(k) is None for k in range(t.n_tiles) if k not in s.tiles)
    assert (seen == 1).all() and sorted(k for o in owners for k in o) == list(range(t.n_tiles))   # every tile, whole, once


@pytest.mark.parametrize("shape", SHAPES, ids=("72x40 in 16x16", "70x50 in 32x8"))
def test_packed_merge_and_noise_are_the_image_order_ones(shape):
    w, h, tw, th = shape
    t = am.Tiling(w, h, tw, th)
    n = t.n_pixels
    acc, mom = fm.synthetic_planes(n, 6, n)
    counts = np.full(n, 6, np.uint32)
    tiles = [0, 1, 4, t.n_tiles - 1]
    p_acc, p_mom = fm.synthetic_planes(n, 12, n + 1)   # a whole frame in image order; a pass takes its listed pixels
    where = t.pixel_map(tiles)
    w_acc, w_mom, w_cnt = am.merge_tiles(t, acc, mom, counts, tiles, p_acc[where], p_mom[where], 12)
    _, w_err, w_sum, w_max = am.tile_noise(t, w_mom, w_cnt, 0.05)
    for count in (2, 3):
        sums, maxes = [], []
        for rank in range(count):
            s = sm.Shard(t, rank, count)
            lp = s.list_pixels(tiles)
            a, m, c = sm.merge_tiles(s, acc[s.map], mom[s.map], counts[s.map], tiles, p_acc[lp], p_mom[lp], 12)
            assert same_bits(a, w_acc[s.map]) and same_bits(m, w_mom[s.map]) and np.array_equal(c, w_cnt[s.map])
            err, tsum, tmax = sm.tile_noise(s, m, c)
            assert same_bits(err, w_err[s.map])
            other = [k for k in range(t.n_tiles) if k not in s.tiles]
            assert not tsum[other].view(np.uint32).any() and not tmax[other].view(np.uint32).any()   # +0.f exactly
            assert same_bits(tsum[s.tiles], w_sum[s.tiles]) and same_bits(tmax[s.tiles], w_max[s.tiles])
            sums.append(tsum)
            maxes.append(tmax)
        assert same_bits(sm.combine(sums), w_sum) and same_bits(sm.combine(maxes), w_max)
        assert same_bits(np.maximum.reduce(sums), w_sum)   # sum, max, the owner's: the same bits


def synthetic_frames(tiling):
    """frame(samples): a seeded whole frame whose noise falls with the samples and differs between tiles - some tiles meet a
    target long before others."""
    n = tiling.n_pixels
    tile_of = np.zeros(n, np.int64)
    for k in range(tiling.n_tiles):
        tile_of[tiling.pixels(k)] = k
    # relative deviation of one sample, per tile column: the columns drop out one after the other, left to right
    # (the last row at half the deviation, so that the active sets are not whole columns)
    rel = np.array([0.05, 0.08, 0.15, 0.3, 0.6])[(tile_of % tiling.tiles_x) % 5] * np.where(tile_of // tiling.tiles_x == 2, 0.5, 1.0)

    def frame(samples):
        rng = np.random.default_rng(samples)
        lum = np.clip(1.0 + rel[None, :] * rng.standard_normal((samples, n)), 0.0, None)
        mom = np.stack([lum.sum(0), (lum * lum).sum(0)], axis=1).astype(f32)
        return np.repeat(mom[:, :1], 3, axis=1).astype(f32), mom
    return frame


@pytest.mark.parametrize("dilate", (0, 1))
@pytest.mark.parametrize("count", (2, 3, 8))
def test_the_lockstep_loop_is_the_unsharded_loop(count, dilate):
    t = am.Tiling(72, 40, 16, 16)
    frame = synthetic_frames(t)
    args = (frame, 8, 8, dilate, 0.04, 250)
    one, made1, why1, sums1 = sm.render_until_adaptive_lockstep(t, 1, *args)
    many, made, why, sums = sm.render_until_adaptive_lockstep(t, count, *args)
    assert made == made1 and why == why1 and same_bits(sums, sums1)
    # the selection bites: a later pass renders fewer tiles than the first, and the ranks' shares of some pass differ
    assert len(made) > 2 and len(made[-1][1]) < len(made[0][1]) == t.n_tiles
    # (three ranks share every whole column of a three-row image equally, and dilation makes the active sets whole columns)
    assert (count == 3 and dilate == 1) or any(len({len(f.shard.own(tiles)) for f in many}) > 1 for _, tiles in made)
    a1, m1, c1 = sm.assemble(one)
    a, m, c = sm.assemble(many)
    assert same_bits(a, a1) and same_bits(m, m1) and np.array_equal(c, c1)
    assert all(f.tile_count == one[0].tile_count for f in many)
    assert am.statistics(t, sums, c, 0.04) == am.statistics(t, sums1, c1, 0.04)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=("72x40 in 16x16", "70x50 in 32x8"))
def test_select_tiles_is_candidates_and_dilate(pta, shape):
    w, h, tw, th = shape
    t = am.Tiling(w, h, tw, th)
    film = pta.Film(pta.Profile.make(w, h, 1, 2), pta.Opts.make(tile_w=tw, tile_h=th))
    pixels = np.array([t.rect(k)[2] * t.rect(k)[3] for k in range(t.n_tiles)], np.float64)
    rng = np.random.default_rng(5)
    target = 0.25
    for trial in range(20):
        mean = rng.uniform(0.0, 0.5, t.n_tiles)
        sums = (mean * pixels).astype(f32)
        # a tile exactly at the target is not selected (0.25 * P is exact in f32); the corners make the clipped borders work
        at = [0, t.tiles_x - 1, t.n_tiles - 1, int(rng.integers(t.n_tiles))][trial % 4]
        sums[at] = f32(target * pixels[at])
        if trial % 5 == 0:
            sums[:] = 0
            sums[t.n_tiles - 1] = f32(pixels[-1])   # only the clipped corner tile is above
        for dilate in (0, 1):
            want = am.dilate(t, am.candidates(t, sums, target), dilate)
            got = film.select_tiles(sums, target, dilate)
            assert got.tolist() == want, (trial, dilate)
            if dilate == 0:
                assert at not in want or trial % 5 == 0
    assert film.select_tiles(np.zeros(t.n_tiles, f32), target).size == 0
    import ctypes as C
    n = C.c_uint32()
    out = np.zeros(t.n_tiles, np.uint32)
    z = np.zeros(t.n_tiles, f32)
    assert film.lib.pt_film_select_tiles(film.handle, z.ctypes.data, target, 2, out.ctypes.data, C.byref(n)) == pta.PT_ERR_INVALID
    assert film.lib.pt_film_select_tiles(film.handle, z.ctypes.data, -1.0, 1, out.ctypes.data, C.byref(n)) == pta.PT_ERR_INVALID
    assert film.lib.pt_film_select_tiles(film.handle, None, target, 1, out.ctypes.data, C.byref(n)) == pta.PT_ERR_INVALID
    film.close()


# ------------------------------------------------------------------------------------------------ the command line
def run(*args):
    return subprocess.run([str(EXE), "render", str(SCENE), *[str(a) for a in args]], capture_output=True, text=True, timeout=300)


def test_cli_refuses_before_any_gpu_work(tmp_path):
    prof = tmp_path / "p.yml"
    prof.write_text("resolution:\n  width: 33\n  height: 17\nsamples: 12\nbounces: 3\n")
    out = tmp_path / "never.png"
    base = ("-q", "-p", prof, "-o", out)
    ok = ("--noise-target", 0.05, "--adaptive")
    cases = [
        (("--film-devices", "0,0"), "'--film-devices <A,B,..>' needs '--noise-target <T>'"),
        (("--noise-target", 0.05, "--film-devices", "0,0"), "needs '--adaptive' or '--window-samples <W>'"),
        ((*ok, "--film-devices", "0,0", "--devices", "0,1"), "'--film-devices <A,B,..>' cannot be used with '--devices <A,B,..>'"),
        ((*ok, "--film-devices", "0,0", "--film-denoise", "variance", "--filtered-target"),
         "'--film-devices <A,B,..>' cannot be used with '--filtered-target'"),
        ((*ok, "--film-devices", "0,0", "--denoise"), "'--film-devices <A,B,..>' cannot be used with '--denoise'"),
        ((*ok, "--film-devices", "0,0", "--light-mixer"), "'--film-devices <A,B,..>' cannot be used with '--light-mixer'"),
        ((*ok, "--film-devices", "0,0", "--camera-path", tmp_path / "c.json"),
         "'--film-devices <A,B,..>' cannot be used with '--camera-path <CAMERAS>'"),
        ((*ok, "--film-devices", "0,0", "--keyframes", tmp_path / "k.json"),
         "'--film-devices <A,B,..>' cannot be used with '--keyframes <FRAMES>'"),
        ((*ok, "--film-devices="), "invalid value '' for '--film-devices <A,B,..>'"),
        ((*ok, "--film-devices", "0,,1"), "invalid value '0,,1' for '--film-devices <A,B,..>'"),
        ((*ok, "--film-devices", "0,"), "invalid value '0,' for '--film-devices <A,B,..>'"),
        ((*ok, "--film-devices", "a,b"), "invalid value 'a,b' for '--film-devices <A,B,..>'"),
        ((*ok, "--film-devices", "0,-1"), "invalid value '0,-1' for '--film-devices <A,B,..>'"),
        ((*ok, "--film-devices"), "a value is required"),
        # --devices keeps its refusals
        ((*ok, "--devices", "0,1"), "more than one device"),
        (("--noise-target", 0.05, "--window-samples", 5, "--devices", "0,1"), "more than one device"),
    ]
    for args, message in cases:
        r = run(*base, *args)
        assert r.returncode == 2 and message in r.stderr, (args, r.returncode, r.stderr)
        assert not out.exists()
