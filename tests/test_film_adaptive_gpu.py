"""The adaptive film on the GPU: k_film_merge_tiles and k_film_tile_noise against tests/film_adaptive_model.py bit
for bit, tile passes against the whole frames of pt_render_moments, the resolve with counts, pt_film_render_until_adaptive
against the model's run over the planes read back after every pass, what a non-uniform film refuses, and a film that never
takes a tile pass."""
import ctypes as C

import numpy as np
import pytest

import film_adaptive_model as am
import film_model as fm
from conftest import SCENES

pytestmark = pytest.mark.gpu

f32 = np.float32
W, H, TILE, BOUNCES = 72, 40, 16, 2   # 5 x 3 tiles, a last column 8 wide, a last row 8 high
TILING = am.Tiling(W, H, TILE, TILE)
EVERY = list(range(15))


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def same_bits(a, b):
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    return a.shape == b.shape and bool((bits(a) == bits(b)).all())


def host(pta, name):
    return pta.HostScene.load_isf(SCENES / name / "scene.isf")


def make_film(pta, samples=1, w=W, h=H, tw=TILE, th=TILE):
    return pta.Film(pta.Profile.make(w, h, samples, BOUNCES), pta.Opts.make(tile_w=tw, tile_h=th))


def parent_device_bytes(n_local):
    """What pt_film_create allocates: accum, moments, the pass buffers, err, the block arrays - 64-float strides."""
    up = lambda floats: (floats + 63) & ~63   # noqa: E731
    return 4 * (2 * (up(3 * n_local) + up(2 * n_local)) + up(n_local) + 2 * up((n_local + 255) // 256))


# ------------------------------------------------------------------------------------------------ kernels against the model
@pytest.mark.parametrize("shape", ((W, H, TILE, TILE), (70, 50, 32, 8)), ids=("72x40 in 16x16", "70x50 in 32x8"))
def test_merge_and_tile_noise_equal_the_model_bit_for_bit(pta, shape):
    w, h, tw, th = shape
    t = am.Tiling(w, h, tw, th)
    n = t.n_pixels
    film = make_film(pta, 1, w, h, tw, th)
    acc, mom = fm.synthetic_planes(n, 6, n)
    film.add_planes(acc, mom, 6)
    counts = np.full(n, 6, np.uint32)
    ai = film.adaptive_info
    assert (ai.uniform, ai.tile_w, ai.tile_h, ai.tiles_x, ai.tiles_y, ai.n_tiles) == (1, tw, th, t.tiles_x, t.tiles_y, t.n_tiles)
    assert (ai.min_samples, ai.max_samples, ai.pixel_samples) == (6, 6, 6 * n)

    def check_noise(label):
        for lum_floor, target in ((0.01, 0.05), (0.5, 0.0), (1e-3, 10.0)):
            want, w_err, w_sum, w_max = am.tile_noise(t, mom, counts, target, lum_floor)
            st, err, tsum, tmax = film.tile_noise(target, lum_floor, want_planes=True)
            assert same_bits(err, w_err), (label, lum_floor)
            assert same_bits(tsum, w_sum), (label, lum_floor)
            assert same_bits(tmax, w_max), (label, lum_floor)
            assert st.as_dict() == want, (label, lum_floor, target)
            assert film.tile_noise(target, lum_floor).as_dict() == want   # (without the err plane: the same figures)
    # a uniform film: film_model's edge cases (zero variance, a mean below the floor, e2 < mu*mu, a black pixel) sit in tile 0,
    # and every pixel's error is pt_film_noise's
    check_noise("uniform")
    assert same_bits(film.tile_noise(0.05, want_planes=True)[1], film.noise(0.05, want_planes=True)[1])
    assert film.adaptive_info.uniform == 1 and (film.read_counts() == 6).all()
    # tile passes as planes: counts that differ between tiles, the edge cases again in tile 0 (the planted values add up
    # exactly: 6 L + 12 L = 18 L), magnitudes that make every other addition round
    lists = ([0, 1, t.n_tiles - 1], [0, t.n_tiles - 1])
    for samples, tiles in zip((12, 1 << 20), lists):
        where = t.pixel_map(tiles)
        p_acc, p_mom = fm.synthetic_planes(len(where), samples, samples + n)
        film.add_tile_planes(p_acc, p_mom, samples, tiles)
        acc, mom, counts = am.merge_tiles(t, acc, mom, counts, tiles, p_acc, p_mom, samples)
        got = film.read()
        assert same_bits(got[0], acc) and same_bits(got[1], mom), tiles
        assert np.array_equal(film.read_counts(), counts), tiles
        check_noise(tiles)
    info, ai = film.info, film.adaptive_info
    assert (info.samples, info.passes, info.last_pass_samples) == (6 + 12 + (1 << 20), 3, 1 << 20)
    assert (ai.uniform, ai.tile_passes, ai.min_samples, ai.max_samples) == (0, 2, 6, 6 + 12 + (1 << 20))
    assert ai.pixel_samples == int(counts.astype(np.uint64).sum()) and len(set(counts.tolist())) == 3
    # the rules of a pass hold for tile planes too, and a refusal changes nothing
    lib = film.lib
    one = np.asarray([0], np.uint32)
    args = (one.ctypes.data, 1, p_acc.ctypes.data, p_mom.ctypes.data)
    assert lib.pt_film_add_tile_planes(film.handle, (1 << 21) - 1, *args) == pta.PT_ERR_INVALID     # not twice the last pass
    assert lib.pt_film_add_tile_planes(film.handle, 1 << 24, *args) == pta.PT_ERR_INVALID           # above 2^24 in all
    assert lib.pt_film_add_tile_planes(film.handle, 1 << 21, None, 1, p_acc.ctypes.data, p_mom.ctypes.data) == pta.PT_ERR_INVALID
    assert lib.pt_film_add_tile_planes(film.handle, 1 << 21, one.ctypes.data, 0, p_acc.ctypes.data, p_mom.ctypes.data) == pta.PT_ERR_INVALID
    bad = np.asarray([1, 1], np.uint32)
    assert lib.pt_film_add_tile_planes(film.handle, 1 << 21, bad.ctypes.data, 2, p_acc.ctypes.data, p_mom.ctypes.data) == pta.PT_ERR_INVALID
    far = np.asarray([t.n_tiles], np.uint32)
    assert lib.pt_film_add_tile_planes(film.handle, 1 << 21, far.ctypes.data, 1, p_acc.ctypes.data, p_mom.ctypes.data) == pta.PT_ERR_INVALID
    assert lib.pt_film_add_tile_planes(film.handle, 1 << 21, one.ctypes.data, 1, None, p_mom.ctypes.data) == pta.PT_ERR_INVALID
    got = film.read()
    assert same_bits(got[0], acc) and same_bits(got[1], mom) and np.array_equal(film.read_counts(), counts)
    # the measurement entry runs the three kernels and leaves the film as it was
    film.adaptive_kernel_times(reps=2)
    got = film.read()
    assert same_bits(got[0], acc) and same_bits(got[1], mom) and np.array_equal(film.read_counts(), counts)
    film.close()


def test_tile_noise_needs_two_samples_in_every_pixel(pta):
    film = make_film(pta)
    acc, mom = fm.synthetic_planes(W * H, 1, 3)
    out = pta.FilmTileStats()
    film.add_planes(acc, mom, 1)
    assert film.lib.pt_film_tile_noise(film.handle, 0.01, 0.1, C.byref(out), None, None, None) == pta.PT_ERR_INVALID
    where = TILING.pixel_map([3])
    p_acc, p_mom = fm.synthetic_planes(len(where), 2, 4)
    film.add_tile_planes(p_acc, p_mom, 2, [3])        # tile 3 has three samples now, every other tile one
    assert film.lib.pt_film_tile_noise(film.handle, 0.01, 0.1, C.byref(out), None, None, None) == pta.PT_ERR_INVALID
    for lum_floor, target in ((0.0, 0.1), (np.nan, 0.1), (0.01, -1.0), (0.01, np.inf)):
        assert film.lib.pt_film_tile_noise(film.handle, lum_floor, target, C.byref(out), None, None, None) == pta.PT_ERR_INVALID
    assert film.lib.pt_film_tile_noise(film.handle, 0.01, 0.1, None, None, None, None) == pta.PT_ERR_INVALID
    planes = pta.Film.from_planes(acc, mom, 4)         # no profile: no tiling
    assert planes.lib.pt_film_tile_noise(planes.handle, 0.01, 0.1, C.byref(out), None, None, None) == pta.PT_ERR_INVALID
    one = np.asarray([0], np.uint32)
    assert planes.lib.pt_film_add_tile_planes(planes.handle, 8, one.ctypes.data, 1, p_acc.ctypes.data, p_mom.ctypes.data) == pta.PT_ERR_INVALID
    sharded = pta.Film(pta.Profile.make(W, H, 1, BOUNCES), pta.Opts.make(tile_w=TILE, tile_h=TILE, shard_rank=0, shard_count=2))
    assert sharded.lib.pt_film_add_tile_planes(sharded.handle, 8, one.ctypes.data, 1, p_acc.ctypes.data, p_mom.ctypes.data) == pta.PT_ERR_INVALID
    assert sharded.info.samples == 0
    for f in (film, planes, sharded):
        f.close()


# ------------------------------------------------------------------------------------------------ passes
A_TILES, B_TILES = [1, 2, 6, 7, 9, 14], [2, 7, 14]


@pytest.fixture(scope="module")
def frames(pta):
    """The whole frames of pt_render_moments, rendered once per scene by a scene of their own."""
    cache = {}

    def get(name):
        if name not in cache:
            ref = pta.GpuScene(host(pta, name))
            o = pta.Opts.make(tile_w=TILE, tile_h=TILE)
            cache[name] = {n: ref.render_moments(pta.Profile.make(W, H, n, BOUNCES), o) for n in (2, 4, 8, 16)}
            ref.close()
        return cache[name]
    return get


@pytest.mark.parametrize("name", ("cube", "spheres"))
def test_tile_passes_are_the_whole_frames_pixels_added_in_order(pta, frames, name):
    fr = frames(name)
    g = pta.GpuScene(host(pta, name))
    film = make_film(pta, 999)
    film.add_pass(g, 2)
    assert film.adaptive_info.uniform == 1 and film.info.device_bytes == parent_device_bytes(W * H)
    acc, mom = fr[2][1].copy(), fr[2][2].copy()
    counts = np.full(W * H, 2, np.uint32)
    assert same_bits(film.read()[0], acc) and same_bits(film.read()[1], mom)
    for samples, tiles in ((4, A_TILES), (8, B_TILES)):
        film.add_tile_pass(g, samples, tiles)
        where = TILING.pixel_map(tiles)
        before = (acc, mom)
        acc, mom, counts = am.merge_tiles(TILING, acc, mom, counts, tiles, fr[samples][1][where], fr[samples][2][where], samples)
        got = film.read()
        assert same_bits(got[0], acc) and same_bits(got[1], mom), (name, samples)
        assert np.array_equal(film.read_counts(), counts), (name, samples)
        rest = np.setdiff1d(np.arange(W * H), where)     # pixels outside the pass keep their bits
        assert same_bits(got[0][rest], before[0][rest]) and same_bits(got[1][rest], before[1][rest])
    # every pixel: the left-to-right sum of the frames it took part in, its count the sum of their samples
    in_a, in_b = np.zeros(W * H, bool), np.zeros(W * H, bool)
    in_a[TILING.pixel_map(A_TILES)] = True
    in_b[TILING.pixel_map(B_TILES)] = True
    for plane, got in ((1, acc), (2, mom)):
        want = fr[2][plane].copy()
        want[in_a] = (want[in_a] + fr[4][plane][in_a]).astype(f32)
        want[in_b] = (want[in_b] + fr[8][plane][in_b]).astype(f32)
        assert same_bits(got, want)
    assert np.array_equal(counts, 2 + 4 * in_a.astype(np.uint32) + 8 * in_b.astype(np.uint32))
    assert sorted(set(counts.tolist())) == [2, 6, 14] and np.abs(acc).max() > 0
    info, ai = film.info, film.adaptive_info
    assert (info.samples, info.passes, info.last_pass_samples) == (14, 3, 8)
    assert (ai.uniform, ai.tile_passes, ai.min_samples, ai.max_samples, ai.pixel_samples) == (0, 2, 2, 14, int(counts.sum()))
    assert info.device_bytes > parent_device_bytes(W * H) and ai.device_bytes == info.device_bytes
    # the noise of rendered planes, held to the model as well
    want, w_err, w_sum, w_max = am.tile_noise(TILING, mom, counts, 0.03)
    st, err, tsum, tmax = film.tile_noise(0.03, want_planes=True)
    assert same_bits(err, w_err) and same_bits(tsum, w_sum) and same_bits(tmax, w_max) and st.as_dict() == want, name
    # a whole pass on a non-uniform film: the tile pass that lists every tile
    film.add_pass(g, 16)
    where = TILING.pixel_map(EVERY)
    acc, mom, counts = am.merge_tiles(TILING, acc, mom, counts, EVERY, fr[16][1][where], fr[16][2][where], 16)
    got = film.read()
    assert same_bits(got[0], acc) and same_bits(got[1], mom) and np.array_equal(film.read_counts(), counts)
    assert same_bits(acc, fm.merge(before_whole(fr, in_a, in_b, 1), fr[16][1]))
    assert (film.info.samples, film.info.passes, film.adaptive_info.tile_passes) == (30, 4, 3)
    # refusals of a tile pass leave the film as it was
    lib = film.lib
    t = np.asarray(B_TILES, np.uint32)
    assert lib.pt_film_add_tile_pass(film.handle, g.handle, 31, t.ctypes.data, 3) == pta.PT_ERR_INVALID
    assert lib.pt_film_add_tile_pass(film.handle, None, 32, t.ctypes.data, 3) == pta.PT_ERR_INVALID
    assert lib.pt_film_add_tile_pass(None, g.handle, 32, t.ctypes.data, 3) == pta.PT_ERR_INVALID
    assert lib.pt_film_add_tile_pass(film.handle, g.handle, 32, None, 3) == pta.PT_ERR_INVALID
    assert lib.pt_film_add_tile_pass(film.handle, g.handle, 32, t.ctypes.data, 0) == pta.PT_ERR_INVALID
    down = np.asarray([7, 2], np.uint32)
    assert lib.pt_film_add_tile_pass(film.handle, g.handle, 32, down.ctypes.data, 2) == pta.PT_ERR_INVALID
    got = film.read()
    assert same_bits(got[0], acc) and same_bits(got[1], mom) and np.array_equal(film.read_counts(), counts) and film.info.passes == 4
    film.close()
    g.close()


def before_whole(fr, in_a, in_b, plane):
    want = fr[2][plane].copy()
    want[in_a] = (want[in_a] + fr[4][plane][in_a]).astype(f32)
    want[in_b] = (want[in_b] + fr[8][plane][in_b]).astype(f32)
    return want


# ------------------------------------------------------------------------------------------------ resolve
def test_resolve_divides_every_pixel_by_its_own_count(pta, frames):
    import torch
    fr = frames("spheres")
    film = make_film(pta)
    film.add_planes(fr[2][1], fr[2][2], 2)
    for samples, tiles in ((4, A_TILES), (8, B_TILES)):
        where = TILING.pixel_map(tiles)
        film.add_tile_planes(fr[samples][1][where], fr[samples][2][where], samples, tiles)
    acc, mom = film.read()
    counts = film.read_counts()
    assert sorted(set(counts.tolist())) == [2, 6, 14]
    n, guard = W * H * 3, 64
    for tm in ("FILMIC", "ACES"):
        rgb, col = film.resolve(tm, want_color=True)
        d_rgb = torch.full((n + guard,), 0xA5, dtype=torch.uint8, device="cuda")
        d_col = torch.full((n + guard,), -7.0, dtype=torch.float32, device="cuda")
        film.resolve_device(tm, d_rgb.data_ptr(), d_col.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        h_rgb, h_col = d_rgb.cpu().numpy(), d_col.cpu().numpy()
        assert (h_rgb[n:] == 0xA5).all() and (h_col[n:] == f32(-7.0)).all()
        assert np.array_equal(h_rgb[:n].reshape(-1, 3), rgb) and same_bits(h_col[:n].reshape(-1, 3), col)
        assert np.array_equal(film.resolve(tm), rgb)
        for c in (2, 6, 14):
            uniform = pta.Film.from_planes(acc, mom, c)
            want_rgb, want_col = uniform.resolve(tm, want_color=True)
            uniform.close()
            sel = counts == c
            assert np.array_equal(rgb[sel], want_rgb[sel]), (tm, c)
            assert same_bits(col[sel], want_col[sel]), (tm, c)
            assert same_bits(col[sel], fm.resolve_color(acc[sel], c))
    assert (rgb[counts == 2] != film_uniform_rgb(pta, acc, mom, 14)[counts == 2]).any()   # (the count matters)
    film.close()


def film_uniform_rgb(pta, acc, mom, c):
    f = pta.Film.from_planes(acc, mom, c)
    rgb = f.resolve("ACES")
    f.close()
    return rgb


# ------------------------------------------------------------------------------------------------ render_until_adaptive
@pytest.mark.parametrize("dilate", (0, 1))
def test_render_until_adaptive_makes_the_models_passes(pta, dilate):
    g = pta.GpuScene(host(pta, "cube"))
    film = make_film(pta)
    target, lum_floor = 0.03, 0.01
    params = pta.FilmAdaptiveParams.default(target=target, lum_floor=lum_floor, first_pass_samples=8, uniform_samples=8,
                                            dilate=dilate, max_samples=56)
    seen = []

    def on_pass(info, noise):
        seen.append({"info": (info.passes, info.last_pass_samples, info.samples), "noise": noise.as_dict(),
                     "planes": film.read(), "counts": film.read_counts()})
    out = film.render_until_adaptive(g, params, on_pass)
    assert seen
    # every pass: which tiles it rendered (their counts moved, by the pass's samples), and the model's figures over the planes
    rendered, stats, sums = [], [], []
    counts = np.zeros(W * H, np.uint32)
    for s in seen:
        moved = s["counts"] != counts
        tiles = [k for k in EVERY if moved[TILING.pixels(k)].any()]
        assert (s["counts"][moved] - counts[moved] == s["info"][1]).all() and all(moved[TILING.pixels(k)].all() for k in tiles)
        counts = s["counts"]
        st, _, tsum, _ = am.tile_noise(TILING, s["planes"][1], counts, target, lum_floor, active_tiles=len(tiles))
        rendered.append(tiles)
        stats.append(st)
        sums.append(tsum)
        assert s["noise"] == {"mean_error": st["mean_error"], "max_block_error": st["max_tile_error"],
                              "fraction_over": st["over_tiles"] / 15, "samples": st["samples"], "n_blocks": 15,
                              "converged": st["converged"]}
        assert s["info"][2] == st["samples"] == int(counts.max())
    made, why = am.render_until_adaptive(TILING, lambda k, samples, tiles: sums[k], 8, 8, dilate, target, 56)
    assert [m[0] for m in made] == [s["info"][1] for s in seen]
    assert [m[1] for m in made] == rendered
    assert out.as_dict() == stats[-1] and bool(out.converged) == (why == "converged")
    assert [s["info"][0] for s in seen] == list(range(1, len(made) + 1))
    # what makes this a test of the adaptive path (from the model, not hard-coded): the first pass leaves some tiles above the
    # target and some below it, and the last pass renders fewer tiles than the first
    first = am.candidates(TILING, sums[0], target)
    assert 0 < len(first) < 15, first
    assert rendered[0] == EVERY and len(rendered[-1]) < len(rendered[0])
    assert rendered[1] == am.dilate(TILING, first, dilate)
    ai = film.adaptive_info
    assert ai.uniform == 0 and ai.pixel_samples == int(counts.sum()) == out.pixel_samples < W * H * film.info.samples
    # every pixel is still the sum of the whole frames' pixels it took part in
    ref = pta.GpuScene(host(pta, "cube"))
    o = pta.Opts.make(tile_w=TILE, tile_h=TILE)
    acc, mom = np.zeros((W * H, 3), f32), np.zeros((W * H, 2), f32)
    cnt = np.zeros(W * H, np.uint32)
    for (samples, tiles) in made:
        fr = ref.render_moments(pta.Profile.make(W, H, samples, BOUNCES), o)
        where = TILING.pixel_map(tiles)
        acc, mom, cnt = am.merge_tiles(TILING, acc, mom, cnt, tiles, fr[1][where], fr[2][where], samples)
    assert same_bits(seen[-1]["planes"][0], acc) and same_bits(seen[-1]["planes"][1], mom) and np.array_equal(cnt, counts)
    # refusals
    lib = film.lib
    none = C.cast(None, pta.FILM_PASS_FN)
    ts = pta.FilmTileStats()
    for change in ({"first_pass_samples": 1}, {"dilate": 2}, {"lum_floor": 0.0}, {"target": -1.0}, {"target": float("nan")}):
        p = pta.FilmAdaptiveParams.default(**change)
        assert lib.pt_film_render_until_adaptive(film.handle, g.handle, C.byref(p), none, None, C.byref(ts)) == pta.PT_ERR_INVALID
    assert lib.pt_film_render_until_adaptive(film.handle, None, C.byref(params), none, None, C.byref(ts)) == pta.PT_ERR_INVALID
    assert lib.pt_film_render_until_adaptive(film.handle, g.handle, None, none, None, C.byref(ts)) == pta.PT_ERR_INVALID
    assert lib.pt_film_render_until_adaptive(film.handle, g.handle, C.byref(params), none, None, None) == pta.PT_ERR_INVALID
    assert np.array_equal(film.read_counts(), counts)
    # called again with the same budget: the film measures what it holds and renders nothing
    again = film.render_until_adaptive(g, params)
    assert np.array_equal(film.read_counts(), counts) and again.as_dict() == dict(stats[-1], active_tiles=0)
    film.close()
    g.close()
    ref.close()


def test_a_generous_target_keeps_the_film_uniform(pta):
    g = pta.GpuScene(host(pta, "cube"))
    film = make_film(pta)
    out = film.render_until_adaptive(g, pta.FilmAdaptiveParams.default(target=1e9, first_pass_samples=4, max_samples=60))
    assert out.converged == 1 and out.active_tiles == 15 and film.info.samples == 4 and film.adaptive_info.uniform == 1
    # target 0 with every pass whole (uniform_samples above the budget): pt_film_render_until's passes, and still uniform
    film.reset()
    out = film.render_until_adaptive(g, pta.FilmAdaptiveParams.default(target=0.0, first_pass_samples=4, max_samples=60,
                                                                       uniform_samples=1000))
    other = make_film(pta)
    other.render_until(g, 4, 60, 0.0)
    assert film.info.samples == other.info.samples == sum(fm.schedule(4, 60)) == 60 and film.adaptive_info.uniform == 1 and not out.converged
    assert same_bits(film.read()[0], other.read()[0]) and same_bits(film.read()[1], other.read()[1])
    assert film.info.device_bytes - parent_device_bytes(W * H) == 15 * 8     # (the tile arrays of the tile noise, nothing else)
    for f in (film, other):
        f.close()
    g.close()


# ------------------------------------------------------------------------------------------------ non-uniform films
def test_what_a_non_uniform_film_refuses_and_reset(pta, frames):
    fr = frames("cube")
    g = pta.GpuScene(host(pta, "cube"))
    film = make_film(pta)
    film.add_planes(fr[2][1], fr[2][2], 2)
    where = TILING.pixel_map(B_TILES)
    film.add_tile_planes(fr[4][1][where], fr[4][2][where], 4, B_TILES)
    before, counts = film.read(), film.read_counts()
    lib, UNSUPPORTED = film.lib, pta.PT_ERR_UNSUPPORTED

    def unchanged():
        now, i = film.read(), film.info
        return (same_bits(now[0], before[0]) and same_bits(now[1], before[1]) and np.array_equal(film.read_counts(), counts)
                and (i.samples, i.passes, i.last_pass_samples) == (6, 2, 4) and film.adaptive_info.uniform == 0)
    out = pta.FilmNoise()
    a, m = C.c_void_p(), C.c_void_p()
    assert lib.pt_film_noise(film.handle, 0.01, 0.1, C.byref(out), None, None, None) == UNSUPPORTED
    assert lib.pt_film_add_planes(film.handle, 8, fr[8][1].ctypes.data, fr[8][2].ctypes.data) == UNSUPPORTED
    assert lib.pt_film_planes_device(film.handle, C.byref(a), C.byref(m)) == UNSUPPORTED and not a.value and not m.value
    assert lib.pt_film_render_until(film.handle, g.handle, 2, 100, 0.01, 0.1, C.cast(None, pta.FILM_PASS_FN), None, C.byref(out)) == UNSUPPORTED
    assert unchanged()
    film.reset()     # uniform and empty again
    info, ai = film.info, film.adaptive_info
    assert (info.samples, info.passes, info.last_pass_samples, ai.uniform, ai.tile_passes) == (0, 0, 0, 1, 0)
    assert not film.read()[0].any() and not film.read()[1].any() and not film.read_counts().any()
    film.add_planes(fr[2][1], fr[2][2], 2)
    film.add_planes(fr[4][1], fr[4][2], 4)
    want = fm.noise(fm.merge(fr[2][2], fr[4][2]), 6, 0.05)[0]
    assert film.noise(0.05).as_dict() == want
    assert film.planes_device()[0] and (film.read_counts() == 6).all()
    film.close()
    g.close()


def test_a_film_that_never_takes_a_tile_pass_allocates_nothing_new(pta):
    g = pta.GpuScene(host(pta, "cube"))
    for w, h in ((W, H), (64, 48)):
        film = pta.Film(pta.Profile.make(w, h, 1, BOUNCES))
        assert film.info.device_bytes == parent_device_bytes(w * h)
        film.render_until(g, 2, 14, 0.0)
        film.noise(0.05, want_planes=True)
        film.resolve(want_color=True)
        assert film.info.device_bytes == parent_device_bytes(w * h) == film.adaptive_info.device_bytes
        assert film.adaptive_info.uniform == 1 and (film.read_counts() == 14).all()
        film.close()
    g.close()
