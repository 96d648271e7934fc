"""Sharded films on the GPU, every comparison bit for bit: the packed kernels against tests/film_shard_model.py and
against the unsharded film holding the same planes; tile passes and tile windows of shard films against the unsharded film driven
with the same global lists; the adaptive loop across ranks - stepped by one thread, and run by one thread per rank through
pt_film_render_until_adaptive_sharded with a barrier for the exchange - against pt_film_render_until_adaptive; the windowed loop
against pt_render_moments(N) and pt_film_render_until_windowed; pt_film_assemble and what it refuses; what stayed as it was.

Several shard films of one film live on the one GPU here: the ranks are a matter of tile ownership, not of devices."""
import ctypes as C
import threading

import numpy as np
import pytest

import film_adaptive_model as am
import film_model as fm
import film_shard_model as sm
from conftest import SCENES

pytestmark = pytest.mark.gpu

f32 = np.float32
W, H, TILE, BOUNCES = 72, 40, 16, 2   # 5 x 3 tiles, a last column 8 wide, a last row 8 high
SHAPES = ((W, H, TILE, TILE), (70, 50, 32, 8))
TILING = am.Tiling(W, H, TILE, TILE)
EVERY = list(range(TILING.n_tiles))
ENUM = 12                             # the enumeration of the windowed films (test_film_window_gpu.py's N)
TARGET, LUM_FLOOR = 0.03, 0.01


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, f32), np.ascontiguousarray(b, f32)
    return a.shape == b.shape and bool((a.view(np.uint32) == b.view(np.uint32)).all())


def host(pta, name="cube"):
    return pta.HostScene.load_isf(SCENES / name / "scene.isf")


def whole_film(pta, shape=SHAPES[0], samples=1, windowed=False):
    w, h, tw, th = shape
    make = pta.Film.windowed if windowed else pta.Film
    return make(pta.Profile.make(w, h, samples, BOUNCES), pta.Opts.make(tile_w=tw, tile_h=th))


def shard_films(pta, n, shape=SHAPES[0], samples=1, windowed=False):
    w, h, tw, th = shape
    return [pta.Film.shard(pta.Profile.make(w, h, samples, BOUNCES),
                           pta.Opts.make(tile_w=tw, tile_h=th, shard_rank=r, shard_count=n), windowed) for r in range(n)]


def shards_of(n, shape=SHAPES[0]):
    t = am.Tiling(*shape)
    return [sm.Shard(t, r, n) for r in range(n)]


def image_of(films, shards):
    """The shard films' planes and counts in image order, through the pixel maps."""
    t = shards[0].tiling
    acc, mom, cnt = np.zeros((t.n_pixels, 3), f32), np.zeros((t.n_pixels, 2), f32), np.zeros(t.n_pixels, np.uint32)
    for f, s in zip(films, shards):
        a, m = f.read()
        acc[s.map], mom[s.map], cnt[s.map] = a, m, f.read_counts()
    return acc, mom, cnt


def assert_same_film(got, want, label=""):
    """Two films in the same layout: planes, counts and counters."""
    (a, m), (wa, wm_) = got.read(), want.read()
    assert same_bits(a, wa) and same_bits(m, wm_), label
    assert np.array_equal(got.read_counts(), want.read_counts()), label
    gi, wi = got.info, want.info
    assert (gi.passes, gi.last_pass_samples, gi.samples, gi.n_local) == (wi.passes, wi.last_pass_samples, wi.samples, wi.n_local), label
    ga, wa_ = got.adaptive_info, want.adaptive_info
    for field in ("uniform", "n_tiles", "tile_passes", "last_pass_tiles", "min_samples", "max_samples", "pixel_samples"):
        assert getattr(ga, field) == getattr(wa_, field), (label, field)
    gw, ww = got.window_info, want.window_info
    assert (gw.windowed, gw.enumeration, gw.windows, gw.tile_windows) == (ww.windowed, ww.enumeration, ww.windows, ww.tile_windows), label


def assert_shards_are(films, shards, want, label=""):
    """Every rank's planes, scattered through its pixel map, are the unsharded film's; the whole film's counters on every rank."""
    acc, mom, cnt = image_of(films, shards)
    (wa, wm_), wc = want.read(), want.read_counts()
    assert same_bits(acc, wa) and same_bits(mom, wm_) and np.array_equal(cnt, wc), label
    wi, wai, wwi = want.info, want.adaptive_info, want.window_info
    for f, s in zip(films, shards):
        i, ai, wn, si = f.info, f.adaptive_info, f.window_info, f.shard_info
        assert (i.passes, i.last_pass_samples, i.samples, i.n_local) == (wi.passes, wi.last_pass_samples, wi.samples, s.n_local), label
        assert (ai.uniform, ai.n_tiles, ai.tiles_x, ai.tiles_y, ai.tile_passes, ai.last_pass_tiles, ai.min_samples, ai.max_samples,
                ai.pixel_samples) == (wai.uniform, wai.n_tiles, wai.tiles_x, wai.tiles_y, wai.tile_passes, wai.last_pass_tiles,
                                      wai.min_samples, wai.max_samples, wai.pixel_samples), label
        assert (wn.windowed, wn.enumeration, wn.windows, wn.tile_windows) == (wwi.windowed, wwi.enumeration, wwi.windows, wwi.tile_windows)
        assert (si.shard, si.rank, si.count, si.n_tiles, si.own_tiles, si.n_pixels) == (1, s.rank, s.count, s.tiling.n_tiles, len(s.tiles),
                                                                                       s.tiling.n_pixels)


def assemble(pta, films, shape=SHAPES[0], samples=1, windowed=False):
    whole = whole_film(pta, shape, samples, windowed)
    whole.assemble(films)
    return whole


def close(*things):
    for t in things:
        for x in (t if isinstance(t, (list, tuple)) else [t]):
            x.close()


# ------------------------------------------------------------------------------------------------ 1. kernels against the model
@pytest.mark.parametrize("shape", SHAPES, ids=("72x40 in 16x16", "70x50 in 32x8"))
@pytest.mark.parametrize("n", (2, 3))
def test_packed_kernels_equal_the_model_and_the_unsharded_film(pta, shape, n):
    t = am.Tiling(*shape)
    npx = t.n_pixels
    shards = shards_of(n, shape)
    films, whole = shard_films(pta, n, shape), whole_film(pta, shape)
    acc, mom = fm.synthetic_planes(npx, 6, npx)
    whole.add_planes(acc, mom, 6)
    state = []
    for f, s in zip(films, shards):
        assert f.info.n_local == s.n_local and np.array_equal(
            s.map, pta.local_pixel_map(pta.Profile.make(shape[0], shape[1], 1, BOUNCES),
                                       pta.Opts.make(tile_w=shape[2], tile_h=shape[3], shard_rank=s.rank, shard_count=n)))
        f.add_planes(acc[s.map], mom[s.map], 6)
        state.append([acc[s.map], mom[s.map], np.full(s.n_local, 6, np.uint32)])

    def check(label):
        assert_shards_are(films, shards, whole, label)
        for lum_floor, target in ((0.01, 0.05), (0.5, 0.0)):
            w_st, w_err, w_sum, w_max = whole.tile_noise(target, lum_floor, want_planes=True)
            sums, maxes = [], []
            for f, s, (a, m, c) in zip(films, shards, state):
                got = f.read()
                assert same_bits(got[0], a) and same_bits(got[1], m) and np.array_equal(f.read_counts(), c), (label, s.rank)
                m_err, m_sum, m_max = sm.tile_noise(s, m, c, lum_floor)
                tsum, tmax, err = f.shard_tile_noise(lum_floor, want_err=True)
                assert same_bits(err, m_err) and same_bits(tsum, m_sum) and same_bits(tmax, m_max), (label, s.rank)
                assert same_bits(err, w_err[s.map])
                other = [k for k in range(t.n_tiles) if k not in s.tiles]
                assert other and not tsum[other].view(np.uint32).any() and not tmax[other].view(np.uint32).any()   # +0.f exactly
                assert same_bits(f.shard_tile_noise(lum_floor)[0], tsum)        # (without the err plane: the same figures)
                sums.append(tsum)
                maxes.append(tmax)
            # the ranks' arrays combined - by sum, by maximum - are the unsharded film's, array for array
            assert same_bits(sm.combine(sums), w_sum) and same_bits(sm.combine(maxes), w_max), label
            assert same_bits(np.maximum.reduce(sums), w_sum) and same_bits(np.maximum.reduce(maxes), w_max), label
            for f in films + [whole]:
                assert f.tile_stats_from_sums(w_sum, target).as_dict() == w_st.as_dict(), label
    check("uniform")
    assert all(f.adaptive_info.uniform == 1 for f in films)
    # tile passes as planes: global lists that mix the ranks' tiles, counts that differ between tiles
    lists = ([0, 1, t.n_tiles - 1], [0, t.n_tiles - 1], [2, 3])
    for samples, tiles in zip((12, 1 << 10, 1 << 20), lists):
        where = t.pixel_map(tiles)
        p_acc, p_mom = fm.synthetic_planes(npx, samples, samples + npx)     # a whole frame; a pass takes its listed pixels
        whole.add_tile_planes(p_acc[where], p_mom[where], samples, tiles)
        owned = []
        for f, s, st in zip(films, shards, state):
            lp = s.list_pixels(tiles)
            owned.append(len(s.own(tiles)))
            f.add_tile_planes(p_acc[lp], p_mom[lp], samples, tiles)
            st[:] = sm.merge_tiles(s, st[0], st[1], st[2], tiles, p_acc[lp], p_mom[lp], samples)
        assert sum(owned) == len(tiles) and (tiles != lists[0] or max(owned) < len(tiles))   # (the first list mixes ranks for sure)
        check(tiles)
    assert len(set(whole.read_counts().tolist())) >= 3
    # the measurement entries run the packed kernels over the rank's tiles and leave the film as it was
    for f in films:
        f.adaptive_kernel_times(reps=2)
        f.window_kernel_times(reps=2)
    check("after the kernel times")
    # a refusal changes nothing: the rules of a pass and of a list hold for global lists
    f = films[0]
    one = np.asarray([0], np.uint32)
    far = np.asarray([t.n_tiles], np.uint32)
    down = np.asarray([3, 1], np.uint32)
    a, m = state[0][0], state[0][1]
    for samples, lst in (((1 << 21) - 1, one), (1 << 24, one), (1 << 21, far), (1 << 21, down)):
        assert f.lib.pt_film_add_tile_planes(f.handle, samples, lst.ctypes.data, len(lst), a.ctypes.data, m.ctypes.data) == pta.PT_ERR_INVALID
    check("after the refusals")
    close(films, whole)


# ------------------------------------------------------------------------------------------------ 2. passes
A_TILES, B_TILES = [1, 2, 6, 7, 9, 14], [2, 6, 14]


def test_tile_passes_of_shard_films_are_the_unsharded_films(pta):
    n = 3
    shards = shards_of(n)
    assert shards[1].own(A_TILES) and not shards[1].own(B_TILES)       # one list has no tile of rank 1
    g = pta.GpuScene(host(pta))
    films, whole = shard_films(pta, n, samples=999), whole_film(pta, samples=999)
    for samples, tiles in ((2, None), (4, A_TILES), (8, B_TILES), (16, None), (32, [0, 1, 13])):
        before = films[1].read() + (films[1].read_counts(),)
        for f in films + [whole]:
            if tiles is None:
                f.add_pass(g, samples)
            else:
                f.add_tile_pass(g, samples, tiles)
        assert_shards_are(films, shards, whole, (samples, tiles))
        if tiles == B_TILES:    # rank 1 holds none of it: its planes stay, its counters move
            now, i = films[1].read(), films[1].info
            assert same_bits(now[0], before[0]) and same_bits(now[1], before[1]) and np.array_equal(films[1].read_counts(), before[2])
            assert (i.passes, i.last_pass_samples, i.samples) == (3, 8, 14) and films[1].adaptive_info.tile_passes == 2
        if samples == 2:
            assert all(f.adaptive_info.uniform == 1 for f in films)
    assert sorted(set(whole.read_counts().tolist())) == [18, 22, 30, 50, 54]
    for f, s in zip(films, shards):   # the resolve works on a rank's planes
        assert np.array_equal(f.resolve(), whole.resolve()[s.map])
    t = np.asarray(B_TILES, np.uint32)
    for f in films:   # refusals of a tile pass leave the film as it was
        assert f.lib.pt_film_add_tile_pass(f.handle, g.handle, 63, t.ctypes.data, 3) == pta.PT_ERR_INVALID
        assert f.lib.pt_film_add_tile_pass(f.handle, g.handle, 64, t.ctypes.data, 0) == pta.PT_ERR_INVALID
    assert_shards_are(films, shards, whole, "after the refusals")
    for f in films:
        f.reset()
        assert (f.info.samples, f.info.passes, f.adaptive_info.uniform, f.shard_info.shard) == (0, 0, 1, 1)
    close(films, whole, g)


def test_tile_windows_of_shard_films_are_the_unsharded_films(pta):
    n = 3
    shards = shards_of(n)
    quiet = [0, 2, 6]
    assert not shards[1].own(quiet)
    g = pta.GpuScene(host(pta))
    films, whole = shard_films(pta, n, samples=ENUM, windowed=True), whole_film(pta, samples=ENUM, windowed=True)
    # the last tile window spans the counts 7 (tiles 0, 2), 2 (3, 13) and 5 (7)
    for samples, tiles in ((2, None), (3, [0, 1, 2, 4, 7, 9]), (2, quiet), (4, [0, 2, 3, 7, 13]), (1, None)):
        before = films[1].read() + (films[1].read_counts(),)
        for f in films + [whole]:
            if tiles is None:
                f.add_window(g, samples)
            else:
                f.add_tile_window(g, samples, tiles)
        assert_shards_are(films, shards, whole, (samples, tiles))
        if tiles == quiet:
            now, i = films[1].read(), films[1].info
            assert same_bits(now[0], before[0]) and same_bits(now[1], before[1]) and np.array_equal(films[1].read_counts(), before[2])
            assert (i.passes, i.last_pass_samples, i.samples) == (3, 2, 7) and films[1].window_info.tile_windows == 2
    assert sorted(set(whole.read_counts().tolist())) == [3, 5, 6, 7, 10, 12]
    # a listed tile of ANOTHER rank that would pass the enumeration refuses the window on every rank (tile 0 is full)
    t = np.asarray([0, 5], np.uint32)
    for f in films:
        assert f.lib.pt_film_add_tile_window(f.handle, g.handle, 1, t.ctypes.data, 2) == pta.PT_ERR_INVALID
    assert_shards_are(films, shards, whole, "after the refusal")
    close(films, whole, g)


# ------------------------------------------------------------------------------------------------ 3. and 4. the adaptive loop
def adaptive_params(pta, dilate):
    return pta.FilmAdaptiveParams.default(target=TARGET, lum_floor=LUM_FLOOR, first_pass_samples=8, uniform_samples=8, dilate=dilate,
                                          max_samples=56)


@pytest.fixture(scope="module")
def unsharded(pta):
    """pt_film_render_until_adaptive on an unsharded film, once per dilate: the film, its result, what on_pass saw, the tiles of
    every pass and the tile sums after it."""
    cache = {}

    def get(dilate):
        if dilate not in cache:
            g = pta.GpuScene(host(pta))
            film = whole_film(pta)
            seen, rendered, sums = [], [], []

            def on_pass(info, noise):
                seen.append(((info.passes, info.last_pass_samples, info.samples), noise.as_dict()))
                rendered.append(film.adaptive_info.last_pass_tiles)
                sums.append(film.tile_noise(TARGET, LUM_FLOOR, want_planes=True)[2])
            out = film.render_until_adaptive(g, adaptive_params(pta, dilate), on_pass)
            g.close()
            # the condition that makes these tests of the adaptive path, on the inputs: the first measurement leaves some tiles
            # above the target and some below it, and the last pass renders fewer tiles than the first
            assert 0 < len(am.candidates(TILING, sums[0], TARGET)) < 15
            assert rendered[0] == 15 and rendered[-1] < rendered[0]
            cache[dilate] = {"film": film, "out": out, "seen": seen, "rendered": rendered, "sums": sums}
        return cache[dilate]
    yield get
    for c in cache.values():
        c["film"].close()


@pytest.mark.parametrize("dilate", (0, 1))
@pytest.mark.parametrize("n", (2, 3))
def test_the_loop_stepped_by_one_thread(pta, unsharded, n, dilate):
    ref = unsharded(dilate)
    shards = shards_of(n)
    g = pta.GpuScene(host(pta))
    films = shard_films(pta, n)
    cap, first, uniform = 56, 8, 8
    lists, active, stats, last, total = [], None, None, 0, 0
    while stats is None or not stats.converged:
        nxt = 2 * last if last else first
        if total + nxt > cap:
            break
        everything = stats is None or total < uniform or len(active) == 15
        for f in films:
            if everything:
                f.add_pass(g, nxt)
            else:
                f.add_tile_pass(g, nxt, active)
        lists.append(EVERY if everything else [int(k) for k in active])
        last, total = nxt, films[0].info.samples
        parts = [f.shard_tile_noise(LUM_FLOOR) for f in films]
        tsum = sm.combine([p[0] for p in parts])
        chosen = [f.select_tiles(tsum, TARGET, dilate) for f in films]
        assert all(np.array_equal(c, chosen[0]) for c in chosen)
        active = chosen[0]
        stats = films[0].tile_stats_from_sums(tsum, TARGET)
        assert all(f.tile_stats_from_sums(tsum, TARGET).as_dict() == stats.as_dict() for f in films)
        assert same_bits(tsum, ref["sums"][len(lists) - 1])
    assert [len(x) for x in lists] == ref["rendered"]
    assert dict(stats.as_dict(), active_tiles=len(lists[-1])) == ref["out"].as_dict()
    shares = [[len(s.own(tiles)) for s in shards] for tiles in lists]
    print("tiles per pass and per rank:", [len(t) for t in lists], shares)
    # In at least one tile pass the ranks' shares differ - with dilate 0: the passes of 4 and of 1 tiles are shared 3/1 and 1/0 by
    # two ranks, 2/1/1 and 1/0/0 by three.  With dilate 1 these inputs cannot say so: dilation makes the active sets the blocks of
    # 4 x 3 and 3 x 2 tiles, which a checkerboard and three diagonal stripes share equally (6/6 and 3/3; 4/4/4 and 2/2/2) - there
    # the uneven lists are test_tile_passes_of_shard_films_are_the_unsharded_films'.
    assert dilate == 1 or any(len(set(s)) > 1 for s, tiles in zip(shares, lists) if len(tiles) < 15)
    assert_shards_are(films, shards, ref["film"], (n, dilate))
    whole = assemble(pta, films)
    assert_same_film(whole, ref["film"], (n, dilate))
    assert whole.tile_noise(TARGET, LUM_FLOOR).as_dict() == ref["film"].tile_noise(TARGET, LUM_FLOOR).as_dict()
    close(films, whole, g)


class BarrierExchange:
    """An exchange for threads of one process: every rank adds its arrays to the round's sums, waits for the others, and takes
    the sums.  A broken barrier returns non-zero, so a rank that fails cannot hang the others."""

    def __init__(self, n, timeout=60.0):
        self.barrier = threading.Barrier(n, timeout=timeout)
        self.lock = threading.Lock()
        self.rounds = {}

    def rank(self, fail_on_first_call=False):
        calls = [0]

        def exchange(tile_sum, tile_max):
            k = calls[0]
            calls[0] += 1
            if fail_on_first_call and k == 0:
                self.barrier.abort()
                return 1
            with self.lock:
                acc = self.rounds.setdefault(k, [np.zeros_like(tile_sum), np.zeros_like(tile_max)])
                acc[0] += tile_sum
                acc[1] += tile_max
            try:
                self.barrier.wait()
            except threading.BrokenBarrierError:
                return 1
            tile_sum[:] = self.rounds[k][0]
            tile_max[:] = self.rounds[k][1]
            return 0
        return exchange


def run_ranks(pta, films, loop):
    """loop(film, scene, rank) on one thread per film, each with a scene of its own; returns the results (or exceptions)."""
    results = [None] * len(films)

    def work(r):
        g = None
        try:
            g = pta.GpuScene(host(pta))
            results[r] = loop(films[r], g, r)
        except BaseException as e:   # noqa: BLE001 (handed to the test's thread)
            results[r] = e
        finally:
            if g is not None:
                g.close()
    threads = [threading.Thread(target=work, args=(r,)) for r in range(len(films))]
    for th in threads:
        th.start()
    for th in threads:
        th.join(timeout=300)
    assert not any(th.is_alive() for th in threads)
    return results


@pytest.mark.parametrize("dilate", (0, 1))
@pytest.mark.parametrize("n", (2, 3))
def test_the_loop_with_the_callback(pta, unsharded, n, dilate):
    ref = unsharded(dilate)
    shards = shards_of(n)
    films = shard_films(pta, n)
    ex = BarrierExchange(n)
    seen = [[] for _ in range(n)]

    def loop(film, g, r):
        def on_pass(info, noise):
            seen[r].append(((info.passes, info.last_pass_samples, info.samples), noise.as_dict()))
        return film.render_until_adaptive_sharded(g, adaptive_params(pta, dilate), ex.rank(), on_pass)
    outs = run_ranks(pta, films, loop)
    for r in range(n):
        assert not isinstance(outs[r], BaseException), outs[r]
        assert outs[r].as_dict() == ref["out"].as_dict(), r
        assert seen[r] == ref["seen"], r
    assert_shards_are(films, shards, ref["film"], (n, dilate))
    whole = assemble(pta, films)
    assert_same_film(whole, ref["film"], (n, dilate))
    close(films, whole)


def test_a_failing_exchange_ends_every_rank(pta):
    n = 3
    films = shard_films(pta, n)
    ex = BarrierExchange(n)

    def loop(film, g, r):
        return film.render_until_adaptive_sharded(g, adaptive_params(pta, 1), ex.rank(fail_on_first_call=(r == 1)))
    outs = run_ranks(pta, films, loop)
    for r, f in enumerate(films):
        assert isinstance(outs[r], pta.PtError) and outs[r].code == pta.PT_ERR_DEVICE, outs[r]
        assert "returned 1" in str(outs[r])
        assert (f.info.passes, f.info.samples) == (1, 8)      # the first pass is kept
    # ... and the parts are still one film
    whole = assemble(pta, films)
    assert whole.info.samples == 8 and whole.adaptive_info.uniform == 1
    close(films, whole)


@pytest.mark.parametrize("dilate", (0, 1))
def test_one_rank_without_an_exchange(pta, unsharded, dilate):
    ref = unsharded(dilate)
    g = pta.GpuScene(host(pta))
    film = shard_films(pta, 1)[0]
    si = film.shard_info
    assert (si.shard, si.rank, si.count, si.own_tiles, si.n_tiles) == (1, 0, 1, 15, 15)
    seen = []
    out = film.render_until_adaptive_sharded(g, adaptive_params(pta, dilate), None,
                                             lambda info, noise: seen.append(((info.passes, info.last_pass_samples, info.samples), noise.as_dict())))
    assert out.as_dict() == ref["out"].as_dict() and seen == ref["seen"]
    assert_same_film(film, ref["film"])            # one rank holds the image in image order
    whole = assemble(pta, [film])
    assert_same_film(whole, ref["film"])
    # more ranks than one need an exchange
    two = shard_films(pta, 2)[0]
    none_ex, none_cb = C.cast(None, pta.FILM_EXCHANGE_FN), C.cast(None, pta.FILM_PASS_FN)
    p, ts = adaptive_params(pta, dilate), pta.FilmTileStats()
    assert two.lib.pt_film_render_until_adaptive_sharded(two.handle, g.handle, C.byref(p), none_ex, None, none_cb, None, C.byref(ts)) == pta.PT_ERR_INVALID
    assert two.info.samples == 0
    close(film, whole, two, g)


# ------------------------------------------------------------------------------------------------ 5. windowed
def test_a_windowed_shard_film_run_to_its_budget_is_the_render_of_the_enumeration(pta):
    n = 2
    ref = pta.GpuScene(host(pta))
    want = ref.render_moments(pta.Profile.make(W, H, ENUM, BOUNCES), pta.Opts.make(tile_w=TILE, tile_h=TILE))
    films = shard_films(pta, n, samples=ENUM, windowed=True)
    ex = BarrierExchange(n)
    windows = [[] for _ in range(n)]
    params = pta.FilmWindowParams.default(target=0.0, window_samples=5, adaptive=0)
    outs = run_ranks(pta, films, lambda film, g, r: film.render_until_windowed_sharded(
        g, params, ex.rank(), lambda info, noise: windows[r].append(info.last_pass_samples)))
    for r in range(n):
        assert not isinstance(outs[r], BaseException), outs[r]
        assert windows[r] == [5, 5, 2] and not outs[r].converged and outs[r].samples == ENUM
    whole = assemble(pta, films, samples=ENUM, windowed=True)
    acc, mom = whole.read()
    assert same_bits(acc, want[1]) and same_bits(mom, want[2]) and np.array_equal(whole.resolve(), want[0])
    assert whole.adaptive_info.uniform == 1 and (whole.window_info.windows, whole.info.passes) == (3, 3)
    close(films, whole, ref)


def test_the_adaptive_windowed_loop_across_ranks(pta):
    n = 2
    shards = shards_of(n)
    params = pta.FilmWindowParams.default(target=TARGET, lum_floor=LUM_FLOOR, window_samples=5, adaptive=1, uniform_samples=4, dilate=0)
    g = pta.GpuScene(host(pta))
    one = whole_film(pta, samples=ENUM, windowed=True)
    seen1 = []
    out1 = one.render_until_windowed(g, params, lambda info, noise: seen1.append(((info.passes, info.last_pass_samples, info.samples),
                                                                                 noise.as_dict(), one.adaptive_info.last_pass_tiles)))
    g.close()
    assert one.adaptive_info.uniform == 0 and seen1[-1][2] < seen1[0][2] == 15      # the selection bites
    films = shard_films(pta, n, samples=ENUM, windowed=True)
    ex = BarrierExchange(n)
    seen = [[] for _ in range(n)]

    def loop(film, gs, r):
        return film.render_until_windowed_sharded(gs, params, ex.rank(), lambda info, noise: seen[r].append(
            ((info.passes, info.last_pass_samples, info.samples), noise.as_dict(), film.adaptive_info.last_pass_tiles)))
    outs = run_ranks(pta, films, loop)
    for r in range(n):
        assert not isinstance(outs[r], BaseException), outs[r]
        assert outs[r].as_dict() == out1.as_dict() and seen[r] == seen1, r
    assert_shards_are(films, shards, one)
    whole = assemble(pta, films, samples=ENUM, windowed=True)
    assert_same_film(whole, one)
    close(films, whole, one)


# ------------------------------------------------------------------------------------------------ 6. assembly
def test_an_assembled_film_is_an_ordinary_film(pta, unsharded):
    ref = unsharded(1)
    want = ref["film"]
    n = 3
    g = pta.GpuScene(host(pta))
    films, replay = shard_films(pta, n), whole_film(pta)
    for k in range(len(ref["rendered"])):               # the unsharded loop's passes, replayed (its lists are its selections)
        tiles = EVERY if k == 0 else [int(x) for x in want.select_tiles(ref["sums"][k - 1], TARGET, 1)]
        assert len(tiles) == ref["rendered"][k]
        for f in films + [replay]:
            f.add_pass(g, 8 << k) if len(tiles) == 15 else f.add_tile_pass(g, 8 << k, tiles)
    assert_same_film(replay, want)
    whole = assemble(pta, list(reversed(films)))          # (any order)
    assert_same_film(whole, want)
    dn = pta.DenoiseParams.default_var()
    got_d, want_d = whole.denoise(g, dn, True, LUM_FLOOR, want_ferr=True), want.denoise(g, dn, True, LUM_FLOOR, want_ferr=True)
    assert same_bits(got_d[0], want_d[0]) and np.array_equal(got_d[1], want_d[1]) and same_bits(got_d[2], want_d[2])
    got_r, want_r = whole.resolve(want_color=True), want.resolve(want_color=True)
    assert np.array_equal(got_r[0], want_r[0]) and same_bits(got_r[1], want_r[1])
    # refusals: PT_ERR_INVALID, the whole film untouched
    lib = whole.lib
    fresh = whole_film(pta)

    def refused(target, shards):
        handles = (C.c_void_p * len(shards))(*[f.handle for f in shards])
        rc = lib.pt_film_assemble(target.handle, handles, len(shards))
        return rc == pta.PT_ERR_INVALID
    other_tile = shard_films(pta, n, shape=(W, H, 32, 8))
    windowed = shard_films(pta, n, samples=ENUM, windowed=True)
    ahead = shard_films(pta, n)
    for f in ahead:
        f.add_pass(g, 8)
        f.add_tile_pass(g, 16, [0, 1, 2])
    ahead[2].add_tile_pass(g, 32, [3])                                  # rank 2 has taken a pass the others have not
    cases = {"a missing rank": films[:2], "a rank twice": [films[0], films[1], films[1]], "other counters": [films[0], films[1], ahead[2]],
             "other counters on every shard than a sibling": [ahead[0], ahead[1], ahead[2]],
             "another tile size": other_tile, "a windowed / non-windowed mix": windowed,
             "a mix of kinds among the shards": [films[0], films[1], windowed[2]], "not a shard film": [films[0], films[1], want]}
    for label, shards in cases.items():
        assert refused(fresh, shards), label
        assert (fresh.info.samples, fresh.info.passes, fresh.adaptive_info.uniform) == (0, 0, 1), label
        assert not fresh.read()[0].any() and not fresh.read()[1].any(), label
    assert refused(whole, films)                                        # a whole film that is not empty
    assert_same_film(whole, want, "a refused assembly")
    assert refused(films[0], films)                                     # a shard film is no whole film
    assert lib.pt_film_assemble(fresh.handle, None, 3) == pta.PT_ERR_INVALID and lib.pt_film_assemble(None, None, 0) == pta.PT_ERR_INVALID
    # a reset film takes an assembly, and the assembled film takes further passes like any other
    whole.reset()
    whole.assemble(films)
    assert_same_film(whole, want, "assembled again after a reset")
    nxt = 2 * want.info.last_pass_samples
    for f in (whole, replay):
        f.add_tile_pass(g, nxt, [0, 7, 14])
    assert_same_film(whole, replay, "a further tile pass")
    close(films, whole, replay, fresh, other_tile, windowed, ahead, g)


# ------------------------------------------------------------------------------------------------ 7. nothing old moved
def test_what_each_kind_of_film_refuses(pta):
    g = pta.GpuScene(host(pta))
    INVALID = pta.PT_ERR_INVALID
    one = np.asarray([0], np.uint32)
    npx = W * H
    acc, mom = fm.synthetic_planes(npx, 8, 3)
    # a film of pt_film_create with shard_count = 2 takes whole passes only, as before
    prof = pta.Profile.make(W, H, ENUM, BOUNCES)
    o = pta.Opts.make(tile_w=TILE, tile_h=TILE, shard_rank=0, shard_count=2)
    old, old_w = pta.Film(prof, o), pta.Film.windowed(prof, o)
    lib = old.lib
    assert lib.pt_film_add_tile_planes(old.handle, 8, one.ctypes.data, 1, acc.ctypes.data, mom.ctypes.data) == INVALID
    assert lib.pt_film_add_tile_pass(old.handle, g.handle, 8, one.ctypes.data, 1) == INVALID
    assert lib.pt_film_add_tile_window(old_w.handle, g.handle, 2, one.ctypes.data, 1) == INVALID
    assert "whole passes only" in lib.pt_last_error().decode()
    assert old.shard_info.shard == 0 and old.info.samples == 0 and old_w.info.samples == 0
    # a shard film refuses the calls whose figures are defined over one device's planes
    shard = shard_films(pta, 2)[0]
    s = shards_of(2)[0]
    shard.add_planes(acc[s.map], mom[s.map], 8)
    before = shard.read()
    none_cb = C.cast(None, pta.FILM_PASS_FN)
    ts, ns = pta.FilmTileStats(), pta.FilmNoise()
    ap, wp, fp = pta.FilmAdaptiveParams.default(), pta.FilmWindowParams.default(), pta.FilmFilteredParams.default()
    dn = pta.DenoiseParams.default_var()
    rgb = np.zeros((npx, 3), np.uint8)
    err = np.zeros(npx, f32)
    h, gh = shard.handle, g.handle
    assert lib.pt_film_tile_noise(h, 0.01, 0.1, C.byref(ts), None, None, None) == INVALID
    assert lib.pt_film_render_until(h, gh, 2, 100, 0.01, 0.1, none_cb, None, C.byref(ns)) == INVALID
    assert lib.pt_film_render_until_adaptive(h, gh, C.byref(ap), none_cb, None, C.byref(ts)) == INVALID
    assert lib.pt_film_render_until_windowed(h, gh, C.byref(wp), none_cb, None, C.byref(ts)) == INVALID
    assert lib.pt_film_render_until_filtered(h, gh, C.byref(fp), none_cb, None, C.byref(ts)) == INVALID
    assert lib.pt_film_denoise(h, gh, 1, C.byref(dn), 0.01, rgb.ctypes.data, None, None) == INVALID
    assert lib.pt_film_denoise(h, gh, 0, C.byref(dn), 0.01, rgb.ctypes.data, None, None) == INVALID
    assert lib.pt_film_filtered_noise(h, gh, C.byref(dn), 0.01, 0.1, C.byref(ts), err.ctypes.data, None, None) == INVALID
    assert shard.denoise_scratch_bytes() == 0
    now = shard.read()
    assert same_bits(now[0], before[0]) and same_bits(now[1], before[1]) and (shard.info.passes, shard.info.samples) == (1, 8)
    # a film that is not a shard film refuses the shard calls
    plain = whole_film(pta)
    plain.add_planes(acc, mom, 8)
    tsum = np.zeros(15, f32)
    none_ex = C.cast(None, pta.FILM_EXCHANGE_FN)
    for f in (plain, old):
        assert lib.pt_film_shard_tile_noise(f.handle, 0.01, tsum.ctypes.data, tsum.ctypes.data, None) == INVALID
        assert lib.pt_film_render_until_adaptive_sharded(f.handle, gh, C.byref(ap), none_ex, None, none_cb, None, C.byref(ts)) == INVALID
        assert lib.pt_film_render_until_windowed_sharded(f.handle, gh, C.byref(wp), none_ex, None, none_cb, None, C.byref(ts)) == INVALID
    assert plain.info.passes == 1 and plain.shard_info.shard == 0
    # a shard film's own refusals: every pixel of the image needs two samples; the kinds do not mix
    fresh = shard_films(pta, 2)[0]
    assert lib.pt_film_shard_tile_noise(fresh.handle, 0.01, tsum.ctypes.data, tsum.ctypes.data, None) == INVALID
    assert lib.pt_film_shard_tile_noise(h, 0.0, tsum.ctypes.data, tsum.ctypes.data, None) == INVALID
    assert lib.pt_film_shard_tile_noise(h, 0.01, None, tsum.ctypes.data, None) == INVALID
    assert lib.pt_film_render_until_windowed_sharded(h, gh, C.byref(wp), none_ex, None, none_cb, None, C.byref(ts)) == INVALID
    win = shard_films(pta, 1, samples=ENUM, windowed=True)[0]
    assert lib.pt_film_render_until_adaptive_sharded(win.handle, gh, C.byref(ap), none_ex, None, none_cb, None, C.byref(ts)) == INVALID
    hnd = C.c_void_p()
    assert lib.pt_film_create_shard(0, C.byref(prof), C.byref(o), 2, C.byref(hnd)) == INVALID and not hnd.value
    assert lib.pt_film_create_shard(0, None, C.byref(o), 0, C.byref(hnd)) == INVALID
    bad = pta.Profile.make(W, H, 1, BOUNCES)     # an enumeration of one sample
    assert lib.pt_film_create_shard(0, C.byref(bad), C.byref(o), 1, C.byref(hnd)) == INVALID and not hnd.value
    close(old, old_w, shard, plain, fresh, win, g)


# ------------------------------------------------------------------------------------------------ 8. the ready-made exchange
def test_exchange_comm_with_one_rank(pta):
    """pt_film_exchange_comm through librccl.so with a one-rank communicator (all this box has): the arrays come back as they
    went in, and the one-rank loop run with it is the unsharded loop."""
    comm = pta.Comm(pta.Comm.unique_id(), 0, 1, 0)
    lib = pta.gpu_lib()
    rng = np.random.default_rng(11)
    tsum, tmax = rng.uniform(0, 9, 15).astype(f32), rng.uniform(0, 1, 15).astype(f32)
    tsum[3] = tmax[3] = 0
    a, b = tsum.copy(), tmax.copy()
    assert lib.pt_film_exchange_comm(a.ctypes.data, b.ctypes.data, 15, comm.handle) == pta.PT_OK
    assert same_bits(a, tsum) and same_bits(b, tmax)
    assert lib.pt_film_exchange_comm(a.ctypes.data, b.ctypes.data, 15, None) == pta.PT_ERR_INVALID
    g = pta.GpuScene(host(pta))
    film, plain = shard_films(pta, 1)[0], whole_film(pta)
    out = film.render_until_adaptive_sharded(g, adaptive_params(pta, 1), (lib.pt_film_exchange_comm, comm.handle))
    want = plain.render_until_adaptive(g, adaptive_params(pta, 1))
    assert out.as_dict() == want.as_dict()
    assert_same_film(film, plain)
    close(film, plain, g)
    comm.close()
