"""The numpy model of windowed films (tests/film_window_model.py) on synthetic sample planes: every pixel holds a prefix of
its own samples whatever the schedule, a tile window is one frame per distinct count, windows are clipped at N, refusals change
nothing, and the loop's selection is a pure function of the planes."""
import numpy as np
import pytest

import denoise_var_model as dvm
import film_adaptive_model as am
import film_window_model as wm

f32 = np.float32
W, H, TILE, N = 40, 24, 16, 13   # 3 x 2 tiles: a last column 8 wide, a last row 8 high


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


@pytest.fixture(scope="module")
def tiling():
    return am.Tiling(W, H, TILE, TILE)


@pytest.fixture(scope="module")
def planes(tiling):
    """Radiance that is noisy in the left tiles and nearly constant in the right ones, so a target separates them."""
    rng = np.random.default_rng(7)
    base = rng.uniform(0.2, 1.0, (1, tiling.n_pixels, 3))
    x = (np.arange(tiling.n_pixels) % W)[None, :, None]
    noise = rng.uniform(-1.0, 1.0, (N, tiling.n_pixels, 3)) * np.where(x < 16, 0.6, 0.002)
    p = np.maximum(base + noise * base, 0.0).astype(f32)
    p.setflags(write=False)
    return p


def assert_prefixes(film):
    """Every pixel's sums are the in-order sums of its first count[p] samples."""
    for c in sorted(set(int(v) for v in film.counts)):
        where = np.nonzero(film.counts == c)[0]
        if c == 0:
            assert not film.accum[where].any() and not film.moments[where].any()
            continue
        acc, mom = dvm.moments_of(film.planes[:c, where])
        assert np.array_equal(bits(film.accum[where]), bits(acc)), c
        assert np.array_equal(bits(film.moments[where]), bits(mom)), c


def test_a_chain_of_windows_is_the_whole_sum(planes):
    acc, mom = None, None
    for s0, s1 in ((0, 1), (1, 4), (4, 5), (5, N)):
        acc, mom = wm.carry(acc, mom, planes, s0, s1)
        want = dvm.moments_of(planes[:s1])
        assert np.array_equal(bits(acc), bits(want[0])) and np.array_equal(bits(mom), bits(want[1])), s1
    # a window that starts at 0 ignores what the buffers hold
    again = wm.carry(acc, mom, planes, 0, 3)
    assert np.array_equal(bits(again[0]), bits(dvm.moments_of(planes[:3])[0]))


def test_every_schedule_leaves_prefixes(tiling, planes):
    film = wm.WindowFilm(tiling, planes)
    assert film.add_window(3)
    assert film.add_tile_window(2, [0, 3])
    assert film.add_tile_window(4, [0, 1, 5])         # tiles at 5 and at 3: two frames
    assert film.add_tile_window(1, [2])
    assert film.tile_count == [9, 7, 4, 5, 3, 7]
    assert_prefixes(film)
    for t in range(tiling.n_tiles):
        assert (film.counts[tiling.pixels(t)] == film.tile_count[t]).all()


def test_a_tile_window_is_one_frame_per_count_ascending(tiling, planes):
    film = wm.WindowFilm(tiling, planes)
    film.add_window(2)
    film.add_tile_window(3, [1, 4])
    film.add_tile_window(1, [4])
    film.frames.clear()
    assert film.add_tile_window(2, [0, 1, 2, 4, 5])   # counts 2, 5, 2, 6, 2
    assert film.frames == [(2, 4, [0, 2, 5]), (5, 7, [1]), (6, 8, [4])]
    assert wm.groups_by_count([2, 5, 2, 9, 6, 2], [5, 4, 0]) == [(2, [0, 5]), (6, [4])]
    assert_prefixes(film)


def test_refusals_change_nothing_and_windows_clip_at_the_enumeration(tiling, planes):
    film = wm.WindowFilm(tiling, planes)
    film.add_window(N - 3)
    film.add_tile_window(2, [1])
    before = (film.accum.copy(), film.moments.copy(), film.counts.copy(), list(film.tile_count))
    assert not film.add_window(2)                      # tile 1 would pass N
    assert not film.add_tile_window(4, [0])
    assert not film.add_tile_window(1, [2, 1]) and not film.add_tile_window(1, []) and not film.add_tile_window(0, [0])
    assert not film.add_tile_window(1, [tiling.n_tiles])
    assert np.array_equal(bits(film.accum), bits(before[0])) and np.array_equal(bits(film.moments), bits(before[1]))
    assert np.array_equal(film.counts, before[2]) and film.tile_count == before[3]
    assert wm.next_window(film.tile_count, range(6), 8, N) == (list(range(6)), 1)     # clipped by tile 1 at N - 1
    assert film.add_window(1)
    assert wm.next_window(film.tile_count, range(6), 8, N) == ([0, 2, 3, 4, 5], 2)    # tile 1 is full and takes no more
    assert wm.next_window(film.tile_count, [1], 8, N) == ([], 0)


@pytest.mark.parametrize("window", (2, 5, 8))
def test_a_target_of_zero_renders_the_whole_enumeration(tiling, planes, window):
    film = wm.WindowFilm(tiling, planes)
    made, reason = wm.render_until_windowed(film, window, 0, 4, 1, 0.0)
    assert reason == "budget" and [m[0] for m in made] == [window] * (N // window) + ([N % window] if N % window else [])
    assert all(m[1] == list(range(tiling.n_tiles)) for m in made)
    acc, mom = dvm.moments_of(planes)
    assert np.array_equal(bits(film.accum), bits(acc)) and np.array_equal(bits(film.moments), bits(mom))
    assert (film.counts == N).all()


def test_the_adaptive_loop_drops_quiet_tiles_and_is_deterministic(tiling, planes):
    runs = []
    for _ in range(2):
        film = wm.WindowFilm(tiling, planes)
        runs.append((wm.render_until_windowed(film, 3, 1, 4, 0, 0.05), film))
    (made, reason), film = runs[0]
    assert [(m[0], m[1]) for m in made] == [(m[0], m[1]) for m in runs[1][0][0]] and reason == runs[1][0][1]
    assert np.array_equal(bits(film.accum), bits(runs[1][1].accum)) and np.array_equal(film.counts, runs[1][1].counts)
    every = list(range(tiling.n_tiles))
    assert made[0][1] == every and made[1][1] == every           # below uniform_samples = 4 every tile is rendered
    assert made[2][1] == [0, 3]                                  # then the noisy column only (dilate 0)
    assert reason == "budget" and film.tile_count == [N, 6, 6, N, 6, 6]
    assert made[-1][0] == 1                                      # 6 + 3 + 3 + 1: the last window is clipped
    assert [m[2]["active_tiles"] for m in made] == [len(m[1]) for m in made]
    assert made[-1][2]["pixel_samples"] == int(film.counts.sum()) and made[-1][2]["samples"] == N
    assert_prefixes(film)
    # with dilation the neighbours come along
    film = wm.WindowFilm(tiling, planes)
    made, _ = wm.render_until_windowed(film, 3, 1, 4, 1, 0.05)
    assert made[2][1] == [0, 1, 3, 4]
    # the same planes without adaptivity: every window covers every tile
    film = wm.WindowFilm(tiling, planes)
    made, reason = wm.render_until_windowed(film, 3, 0, 4, 1, 0.05)
    assert reason == "budget" and all(m[1] == every for m in made) and (film.counts == N).all()
