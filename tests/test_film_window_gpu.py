"""Windowed films on the GPU: whole-frame windows against pt_render_moments of the enumeration, tile windows -
k_film_gather_tiles, the carry of the tile-list window frames, k_film_scatter_tiles - and pt_film_render_until_windowed against
tests/film_window_model.py driven by the sample planes, bit for bit; what the two kinds of film refuse of each other; a
pt_film_create film that behaves as before; the film filter on a non-uniform windowed film.

33 x 17 in 16 x 16 tiles (pt_opts refuses 8 x 8): 3 x 2 tiles, a last column 1 pixel wide, a last row 1 pixel high."""
import ctypes as C

import numpy as np
import pytest

import denoise_var_model as dvm
import film_adaptive_model as am
import film_denoise_model as fdm
import film_window_model as wm
from conftest import SCENES

pytestmark = pytest.mark.gpu

f32 = np.float32
W, H, N, BOUNCES, TILE = 33, 17, 12, 3, 16
TILING = am.Tiling(W, H, TILE, TILE)
EVERY = list(range(TILING.n_tiles))
NAMES = ("cube", "alpha_transparency")


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def same_bits(a, b):
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    return a.shape == b.shape and bool((bits(a) == bits(b)).all())


def host(pta, name):
    return pta.HostScene.load_isf(SCENES / name / "scene.isf")


def tiled(pta, **more):
    return pta.Opts.make(tile_w=TILE, tile_h=TILE, **more)


def windowed(pta, n=N, opts=None):
    return pta.Film.windowed(pta.Profile.make(W, H, n, BOUNCES), opts or tiled(pta))


@pytest.fixture(scope="module")
def refs(pta):
    """Per scene, rendered once by a scene of its own and left unchanged: pt_render_moments(N) and the N sample planes."""
    out = {}
    for name in NAMES:
        g = pta.GpuScene(host(pta, name))
        prof = pta.Profile.make(W, H, N, BOUNCES)
        frame, planes = g.render_moments(prof, tiled(pta)), g.render_samples(prof, tiled(pta))
        g.close()
        for a in frame + (planes,):
            a.setflags(write=False)
        out[name] = {"frame": frame, "planes": planes}
    return out


def assert_film_is(film, model, label):
    acc, mom = film.read()
    assert same_bits(acc, model.accum) and same_bits(mom, model.moments), label
    assert np.array_equal(film.read_counts(), model.counts), label


# ------------------------------------------------------------------------------------------------ whole-frame windows
@pytest.mark.parametrize("name", NAMES)
def test_whole_frame_windows_end_as_the_render_of_the_enumeration(pta, refs, name):
    want, planes = refs[name]["frame"], refs[name]["planes"]
    g = pta.GpuScene(host(pta, name))
    film = windowed(pta)
    wi = film.window_info
    assert (wi.windowed, wi.enumeration, wi.windows, wi.tile_windows) == (1, N, 0, 0)
    for rounds in range(2):
        total = 0
        for samples in (5, 3, 4):
            film.add_window(g, samples)
            total += samples
            acc, mom = film.read()
            w_acc, w_mom = dvm.moments_of(planes[:total])
            assert same_bits(acc, w_acc) and same_bits(mom, w_mom), (name, total)
            assert (film.info.samples, film.info.last_pass_samples) == (total, samples)
        acc, mom = film.read()
        assert same_bits(acc, want[1]) and same_bits(mom, want[2]), name
        assert np.array_equal(film.resolve(), want[0]), name
        assert film.adaptive_info.uniform == 1 and (film.read_counts() == N).all()
        assert (film.window_info.windows, film.info.passes) == (3, 3)
        # the film is full: one more sample is refused and changes nothing
        assert film.lib.pt_film_add_window(film.handle, g.handle, 1) == pta.PT_ERR_INVALID
        assert same_bits(film.read()[0], want[1]) and film.info.samples == N
        film.reset()                                                   # ... and reset starts over
        assert (film.info.samples, film.info.passes, film.window_info.windows, film.window_info.windowed) == (0, 0, 0, 1)
    # a window that would pass N, a window of no samples, null arguments
    film.add_window(g, 7)
    before = film.read()
    for samples in (6, 0, 1 << 30):
        assert film.lib.pt_film_add_window(film.handle, g.handle, samples) == pta.PT_ERR_INVALID
    assert film.lib.pt_film_add_window(film.handle, None, 2) == pta.PT_ERR_INVALID
    assert film.lib.pt_film_add_window(None, g.handle, 2) == pta.PT_ERR_INVALID
    assert same_bits(film.read()[0], before[0]) and same_bits(film.read()[1], before[1]) and film.info.samples == 7
    film.add_window(g, 5)
    assert same_bits(film.read()[0], want[1])
    film.close()
    g.close()


def test_a_sharded_windowed_film(pta, refs):
    want = refs["cube"]["frame"]
    g = pta.GpuScene(host(pta, "cube"))
    o = pta.Opts.make(shard_rank=1, shard_count=3, tile_w=8, tile_h=32)
    prof = pta.Profile.make(W, H, N, BOUNCES)
    where = pta.local_pixel_map(prof, o)
    film = pta.Film.windowed(prof, o)
    for samples in (2, 9, 1):
        film.add_window(g, samples)
    acc, mom = film.read()
    assert 0 < len(where) < W * H and same_bits(acc, want[1][where]) and same_bits(mom, want[2][where])
    assert np.array_equal(film.resolve(), want[0][where])
    t = np.asarray([0], np.uint32)
    film.reset()
    assert film.lib.pt_film_add_tile_window(film.handle, g.handle, 2, t.ctypes.data, 1) == pta.PT_ERR_INVALID    # unsharded only
    assert film.info.samples == 0
    film.close()
    g.close()


# ------------------------------------------------------------------------------------------------ tile windows
@pytest.mark.parametrize("name", NAMES)
def test_tile_windows_leave_every_pixel_a_prefix_of_its_own_samples(pta, refs, name):
    planes = refs[name]["planes"]
    g = pta.GpuScene(host(pta, name))
    film = windowed(pta)
    model = wm.WindowFilm(TILING, planes)
    # tile 3 is dropped after the first window and comes back in the last call, which spans the counts 2, 5 and 7
    schedule = ((2, None), (3, [0, 1, 2, 4]), (2, [0, 1]), (4, [0, 2, 3]))
    for samples, tiles in schedule:
        before = film.read() + (film.read_counts(),)
        if tiles is None:
            film.add_window(g, samples)
            assert model.add_window(samples)
            assert film.adaptive_info.uniform == 1
        else:
            film.add_tile_window(g, samples, tiles)
            assert model.add_tile_window(samples, tiles)
            rest = np.setdiff1d(np.arange(W * H), TILING.pixel_map(tiles))      # pixels outside the list keep their bits
            got = film.read()
            assert same_bits(got[0][rest], before[0][rest]) and same_bits(got[1][rest], before[1][rest])
            assert np.array_equal(film.read_counts()[rest], before[2][rest])
            assert film.adaptive_info.uniform == 0
        assert_film_is(film, model, (name, samples, tiles))
    assert model.tile_count == [11, 7, 9, 6, 5, 2]
    assert model.frames[-3:] == [(2, 6, [3]), (5, 9, [2]), (7, 11, [0])]
    acc, mom = film.read()
    counts = film.read_counts()
    for c in sorted(set(counts.tolist())):
        where = np.flatnonzero(counts == c)
        w_acc, w_mom = dvm.moments_of(planes[:c, where])
        assert same_bits(acc[where], w_acc) and same_bits(mom[where], w_mom), (name, c)
    info, ai, wi = film.info, film.adaptive_info, film.window_info
    assert (info.samples, info.passes, info.last_pass_samples) == (11, 4, 4)
    assert (ai.tile_passes, ai.min_samples, ai.max_samples, ai.pixel_samples) == (3, 2, 11, int(counts.sum()))
    assert (wi.windows, wi.tile_windows) == (1, 3)
    # the noise and the resolve read the counts as on any non-uniform film
    want, w_err, w_sum, w_max = am.tile_noise(TILING, mom, counts, 0.03)
    st, err, tsum, tmax = film.tile_noise(0.03, want_planes=True)
    assert same_bits(err, w_err) and same_bits(tsum, w_sum) and same_bits(tmax, w_max) and st.as_dict() == want
    rgb = film.resolve()
    for c in sorted(set(counts.tolist())):
        uniform = pta.Film.from_planes(acc, mom, c)
        assert np.array_equal(rgb[counts == c], uniform.resolve("FILMIC")[counts == c]), c
        uniform.close()
    # refusals: a listed tile would pass N (tile 0 stands at 11), bad lists, null arguments - the film as it was
    lib = film.lib
    u32 = lambda *v: np.asarray(v, np.uint32)   # noqa: E731
    for samples, t in ((2, u32(0, 5)), (11, u32(5)), (0, u32(5)), (1, u32(5, 4)), (1, u32(6)), (1, u32(3, 3))):
        assert lib.pt_film_add_tile_window(film.handle, g.handle, samples, t.ctypes.data, len(t)) == pta.PT_ERR_INVALID, (samples, t)
    one = u32(5)
    assert lib.pt_film_add_tile_window(film.handle, g.handle, 1, None, 1) == pta.PT_ERR_INVALID
    assert lib.pt_film_add_tile_window(film.handle, g.handle, 1, one.ctypes.data, 0) == pta.PT_ERR_INVALID
    assert lib.pt_film_add_tile_window(film.handle, None, 1, one.ctypes.data, 1) == pta.PT_ERR_INVALID
    assert lib.pt_film_add_window(film.handle, g.handle, 2) == pta.PT_ERR_INVALID       # (every tile: tile 0 would pass N)
    assert_film_is(film, model, "after the refusals")
    assert film.info.passes == 4
    # a whole-frame window on a non-uniform film is the tile window that lists every tile
    film.add_window(g, 1)
    assert model.add_window(1)
    assert_film_is(film, model, "a whole window on a non-uniform film")
    # the measurement entry runs the two kernels and leaves the film as it was
    film.window_kernel_times(reps=2)
    assert_film_is(film, model, "after the kernel times")
    film.close()
    g.close()


# ------------------------------------------------------------------------------------------------ the loop
@pytest.mark.parametrize("adaptive,dilate", ((0, 1), (1, 0), (1, 1)))
def test_render_until_windowed_makes_the_models_windows(pta, refs, adaptive, dilate):
    planes = refs["cube"]["planes"]
    g = pta.GpuScene(host(pta, "cube"))
    film = windowed(pta)
    target, lum_floor, window = 0.03, 0.01, 5
    params = pta.FilmWindowParams.default(target=target, lum_floor=lum_floor, window_samples=window, adaptive=adaptive,
                                          uniform_samples=4, dilate=dilate)
    seen = []

    def on_pass(info, noise):
        seen.append({"info": (info.passes, info.last_pass_samples, info.samples), "noise": noise.as_dict(),
                     "planes": film.read(), "counts": film.read_counts()})
    out = film.render_until_windowed(g, params, on_pass)
    model = wm.WindowFilm(TILING, planes)
    made, why = wm.render_until_windowed(model, window, adaptive, 4, dilate, target, lum_floor)
    assert len(seen) == len(made) > 0
    counts = np.zeros(W * H, np.uint32)
    replay = wm.WindowFilm(TILING, planes)
    for s, (samples, tiles, st) in zip(seen, made):
        moved = s["counts"] != counts
        assert [k for k in EVERY if moved[TILING.pixels(k)].any()] == tiles           # the active set
        assert (s["counts"][moved] - counts[moved] == samples).all() and s["info"][1] == samples
        counts = s["counts"]
        assert replay.add_tile_window(samples, tiles)
        assert same_bits(s["planes"][0], replay.accum) and same_bits(s["planes"][1], replay.moments)
        assert np.array_equal(counts, replay.counts)
        assert s["noise"] == {"mean_error": st["mean_error"], "max_block_error": st["max_tile_error"],
                              "fraction_over": st["over_tiles"] / len(EVERY), "samples": st["samples"], "n_blocks": len(EVERY),
                              "converged": st["converged"]}
    assert out.as_dict() == made[-1][2] and bool(out.converged) == (why == "converged")
    assert_film_is(film, model, (adaptive, dilate))
    assert [s["info"][0] for s in seen] == list(range(1, len(made) + 1))
    assert made[0][1] == EVERY and out.pixel_samples == int(counts.sum())
    if adaptive and not dilate:
        # what makes this a test of the adaptive path (from the model): the first window leaves some tiles above the target and
        # some below it, so a later window renders fewer tiles than the first.  (With dilation the neighbours of two tiles are
        # all 3 x 2 tiles of this image: that case holds the loop to the model's dilation, and the film stays uniform.)
        first = am.candidates(TILING, am.tile_noise(TILING, seen[0]["planes"][1], seen[0]["counts"], target, lum_floor)[2], target)
        assert 0 < len(first) < len(EVERY) and made[1][1] == first
        assert film.adaptive_info.uniform == 0 and out.pixel_samples < W * H * film.info.samples
    else:
        assert all(m[1] == EVERY for m in made) and film.adaptive_info.uniform == 1
    # a second call starts with the noise of what the film holds: the same selection, so nothing is left to render
    again = film.render_until_windowed(g, params)
    assert_film_is(film, model, "a second call")
    assert again.as_dict() == dict(made[-1][2], active_tiles=0) and film.info.passes == len(made)
    # refusals
    lib = film.lib
    none = C.cast(None, pta.FILM_PASS_FN)
    ts = pta.FilmTileStats()
    for change in ({"window_samples": 0}, {"dilate": 2}, {"adaptive": 2}, {"lum_floor": 0.0}, {"target": -1.0}, {"target": float("nan")}):
        p = pta.FilmWindowParams.default(**change)
        assert lib.pt_film_render_until_windowed(film.handle, g.handle, C.byref(p), none, None, C.byref(ts)) == pta.PT_ERR_INVALID
    assert lib.pt_film_render_until_windowed(film.handle, None, C.byref(params), none, None, C.byref(ts)) == pta.PT_ERR_INVALID
    assert lib.pt_film_render_until_windowed(film.handle, g.handle, None, none, None, C.byref(ts)) == pta.PT_ERR_INVALID
    assert lib.pt_film_render_until_windowed(film.handle, g.handle, C.byref(params), none, None, None) == pta.PT_ERR_INVALID
    empty = windowed(pta)
    p = pta.FilmWindowParams.default(window_samples=1)                  # (a sample variance needs two)
    assert lib.pt_film_render_until_windowed(empty.handle, g.handle, C.byref(p), none, None, C.byref(ts)) == pta.PT_ERR_INVALID
    assert empty.info.samples == 0
    empty.close()
    film.close()
    g.close()


@pytest.mark.parametrize("name", NAMES)
def test_a_target_of_zero_ends_as_the_render_of_the_enumeration(pta, refs, name):
    want = refs[name]["frame"]
    g = pta.GpuScene(host(pta, name))
    film = windowed(pta)
    windows = []
    out = film.render_until_windowed(g, pta.FilmWindowParams.default(target=0.0, window_samples=5, adaptive=0),
                                     lambda info, noise: windows.append(info.last_pass_samples))
    assert windows == [5, 5, 2] and not out.converged and out.samples == N       # 12 % 5 != 0: the last window is clipped
    acc, mom = film.read()
    assert same_bits(acc, want[1]) and same_bits(mom, want[2]) and np.array_equal(film.resolve(), want[0])
    assert film.adaptive_info.uniform == 1 and film.window_info.windows == 3
    film.close()
    g.close()


# ------------------------------------------------------------------------------------------------ the two kinds of film
def test_the_two_kinds_of_film_refuse_each_others_calls(pta, refs):
    INVALID = pta.PT_ERR_INVALID
    g = pta.GpuScene(host(pta, "cube"))
    lib = g.lib
    none = C.cast(None, pta.FILM_PASS_FN)
    one = np.asarray([0], np.uint32)
    n = W * H
    acc, mom = np.ones((n, 3), f32), np.ones((n, 2), f32)
    ts, ns = pta.FilmTileStats(), pta.FilmNoise()
    # a windowed film
    film = windowed(pta)
    film.add_window(g, 4)
    before = film.read()
    ap, fp = pta.FilmAdaptiveParams.default(), pta.FilmFilteredParams.default()
    assert lib.pt_film_add_pass(film.handle, g.handle, 8) == INVALID
    assert lib.pt_film_add_tile_pass(film.handle, g.handle, 8, one.ctypes.data, 1) == INVALID
    assert lib.pt_film_add_planes(film.handle, 8, acc.ctypes.data, mom.ctypes.data) == INVALID
    assert lib.pt_film_add_tile_planes(film.handle, 8, one.ctypes.data, 1, acc.ctypes.data, mom.ctypes.data) == INVALID
    assert lib.pt_film_render_until(film.handle, g.handle, 8, 64, 0.01, 0.02, none, None, C.byref(ns)) == INVALID
    assert lib.pt_film_render_until_adaptive(film.handle, g.handle, C.byref(ap), none, None, C.byref(ts)) == INVALID
    bytes_before = film.info.device_bytes
    assert lib.pt_film_render_until_filtered(film.handle, g.handle, C.byref(fp), none, None, C.byref(ts)) == INVALID
    assert film.info.device_bytes == bytes_before                       # (refused before the filter's scratch is made)
    assert same_bits(film.read()[0], before[0]) and same_bits(film.read()[1], before[1])
    assert (film.info.samples, film.info.passes, film.adaptive_info.uniform) == (4, 1, 1)
    film.add_window(g, 8)                                               # ... and it goes on as if nothing had been asked
    assert same_bits(film.read()[0], refs["cube"]["frame"][1])
    film.close()
    # a film that is not windowed
    classic = pta.Film(pta.Profile.make(W, H, 1, BOUNCES), tiled(pta))
    wi = classic.window_info
    assert (wi.windowed, wi.enumeration, wi.windows, wi.tile_windows) == (0, 0, 0, 0)
    classic.add_pass(g, 2)
    before = classic.read()
    wp = pta.FilmWindowParams.default()
    assert lib.pt_film_add_window(classic.handle, g.handle, 2) == INVALID
    assert lib.pt_film_add_tile_window(classic.handle, g.handle, 2, one.ctypes.data, 1) == INVALID
    assert lib.pt_film_render_until_windowed(classic.handle, g.handle, C.byref(wp), none, None, C.byref(ts)) == INVALID
    assert same_bits(classic.read()[0], before[0]) and (classic.info.samples, classic.info.passes) == (2, 1)
    classic.add_pass(g, 4)
    assert classic.info.samples == 6
    classic.close()
    # what pt_film_create_windowed refuses: an enumeration below 2 or above 2^24, and what pt_film_create refuses
    h = C.c_void_p()
    o = tiled(pta)
    for samples in (0, 1, (1 << 24) + 1):
        p = pta.Profile.make(W, H, samples, BOUNCES)
        assert lib.pt_film_create_windowed(0, C.byref(p), C.byref(o), C.byref(h)) == INVALID and not h.value
    p = pta.Profile.make(W, H, N, BOUNCES)
    assert lib.pt_film_create_windowed(0, None, C.byref(o), C.byref(h)) == INVALID
    assert lib.pt_film_create_windowed(0, C.byref(p), C.byref(o), None) == INVALID
    bad = pta.Opts.make(tile_w=12, tile_h=16)
    assert lib.pt_film_create_windowed(0, C.byref(p), C.byref(bad), C.byref(h)) == INVALID
    assert lib.pt_film_get_window_info(None, C.byref(pta.FilmWindowInfo())) == INVALID
    g.close()


def test_a_classic_film_runs_the_adaptive_loop_as_before(pta):
    """A pt_film_create film through pt_film_render_until_adaptive: the model's passes over the planes read back after every
    pass, and every pixel the sum of the whole frames it took part in - the contract of tests/test_film_adaptive_gpu.py."""
    g, ref = pta.GpuScene(host(pta, "cube")), pta.GpuScene(host(pta, "cube"))
    film = pta.Film(pta.Profile.make(W, H, 1, BOUNCES), tiled(pta))
    target, lum_floor, budget = 0.03, 0.01, 14
    params = pta.FilmAdaptiveParams.default(target=target, lum_floor=lum_floor, first_pass_samples=2, uniform_samples=2,
                                            dilate=0, max_samples=budget)
    seen = []
    out = film.render_until_adaptive(g, params, lambda info, noise: seen.append(
        {"samples": info.last_pass_samples, "planes": film.read(), "counts": film.read_counts()}))
    sums, rendered = [], []
    counts = np.zeros(W * H, np.uint32)
    for s in seen:
        moved = s["counts"] != counts
        rendered.append([k for k in EVERY if moved[TILING.pixels(k)].any()])
        counts = s["counts"]
        st, _, tsum, _ = am.tile_noise(TILING, s["planes"][1], counts, target, lum_floor, active_tiles=len(rendered[-1]))
        sums.append(tsum)
    made, why = am.render_until_adaptive(TILING, lambda k, samples, tiles: sums[k], 2, 2, 0, target, budget)
    assert [m[0] for m in made] == [s["samples"] for s in seen] == [2, 4, 8][:len(made)]
    assert [m[1] for m in made] == rendered
    assert out.as_dict() == st and bool(out.converged) == (why == "converged")
    acc, mom = np.zeros((W * H, 3), f32), np.zeros((W * H, 2), f32)
    cnt = np.zeros(W * H, np.uint32)
    for samples, tiles in made:
        fr = ref.render_moments(pta.Profile.make(W, H, samples, BOUNCES), tiled(pta))
        where = TILING.pixel_map(tiles)
        acc, mom, cnt = am.merge_tiles(TILING, acc, mom, cnt, tiles, fr[1][where], fr[2][where], samples)
    assert same_bits(seen[-1]["planes"][0], acc) and same_bits(seen[-1]["planes"][1], mom) and np.array_equal(cnt, counts)
    assert film.window_info.windowed == 0
    for x in (film, g, ref):
        x.close()


# ------------------------------------------------------------------------------------------------ the film filter
def test_the_film_filter_on_a_non_uniform_windowed_film(pta, oracle, refs):
    g = pta.GpuScene(host(pta, "cube"))
    film = windowed(pta)
    film.add_window(g, 3)
    film.add_tile_window(g, 4, [0, 1, 4])
    film.add_tile_window(g, 5, [1, 2])
    acc, mom = film.read()
    counts = film.read_counts()
    assert sorted(set(counts.tolist())) == [3, 7, 8, 12]
    guides = g.render_guides(W, H)
    for variance in (1, 0):
        params = (pta.DenoiseParams.default_var if variance else pta.DenoiseParams.default)(iterations=2)
        want_col, want_ferr = fdm.film_denoise_with(params, W, H, counts, acc, mom, guides, bool(variance), 0.01)
        want_rgb = oracle.post_process(pta.Profile.make(W, H, 1, 1, int(params.tonemap)), want_col)
        got = film.denoise(g, params, variance=bool(variance), want_ferr=bool(variance))
        assert same_bits(got[0], want_col) and np.array_equal(got[1], want_rgb), variance
        if variance:
            assert same_bits(got[2], want_ferr)
    st = film.filtered_noise(g, pta.DenoiseParams.default_var(iterations=2), 0.03)
    assert st.samples == 12 and st.pixel_samples == int(counts.sum())
    film.close()
    g.close()
