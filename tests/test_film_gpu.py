"""The progressive film on the GPU: k_film_noise and k_film_merge against tests/film_model.py bit for bit, passes against the
frames of pt_render_moments on a second scene, what a film session leaves behind in its scene, pt_film_render_until against the
model's schedule, the film's device planes through the variance-guided filter, and every refusal."""
import ctypes as C

import numpy as np
import pytest

import film_model as fm
from conftest import SCENES

pytestmark = pytest.mark.gpu

f32 = np.float32
W, H, BOUNCES = 70, 50, 2   # 9 x 2 tiles of 8 x 32; neither side a multiple of a tile
PT_FLAG_NO_GRIDS, PT_FLAG_MEGAKERNEL = 4, 8


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def same_bits(a, b):
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    return a.shape == b.shape and bool((bits(a) == bits(b)).all())


def host(pta, name):
    return pta.HostScene.load_isf(SCENES / name / "scene.isf")


# ------------------------------------------------------------------------------------------------ kernels against the model
@pytest.mark.parametrize("n_local", (1, 2, 255, 256, 257, 8710))
def test_noise_equals_the_model_bit_for_bit(pta, n_local):
    for n in (2, 3, 14, 1 << 24):
        accum, mom = fm.synthetic_planes(n_local, n, 100 * n_local + (n % 97))
        film = pta.Film.from_planes(accum, mom, n, last_pass_samples=max(1, n // 2))
        info = film.info
        assert (info.n_local, info.samples, info.passes, info.last_pass_samples) == (n_local, n, 1, max(1, n // 2))
        assert (info.width, info.height) == (0, 0) and info.device_bytes >= accum.nbytes + mom.nbytes
        got_acc, got_mom = film.read()
        assert same_bits(got_acc, accum) and same_bits(got_mom, mom)
        for lum_floor, target in ((0.01, 0.05), (0.5, 0.0), (1e-3, 10.0)):
            want, w_err, w_sum, w_max = fm.noise(mom, n, target, lum_floor)
            st, err, bsum, bmax = film.noise(target, lum_floor, want_planes=True)
            assert same_bits(err, w_err), (n_local, n, lum_floor)
            assert same_bits(bsum, w_sum), (n_local, n, lum_floor)
            assert same_bits(bmax, w_max), (n_local, n, lum_floor)
            assert st.as_dict() == want, (n_local, n, lum_floor, target)
            assert film.noise(target, lum_floor).as_dict() == want   # (without the err plane: the same figures)
        assert same_bits(film.resolve(want_color=True)[1], fm.resolve_color(accum, n))
        film.close()


@pytest.mark.parametrize("n_local", (1, 2, 255, 256, 257, 8710))
def test_merge_equals_the_model_bit_for_bit(pta, n_local):
    """k_film_merge on planes of every length: a film made from planes takes two more passes as planes (pt_film_add_planes
    runs the kernel pt_film_add_pass runs).  The magnitudes differ by orders, so every addition rounds."""
    a_acc, a_mom = fm.synthetic_planes(n_local, 3, n_local + 1)
    b_acc, b_mom = fm.synthetic_planes(n_local, 14, n_local + 2)
    c_acc, c_mom = fm.synthetic_planes(n_local, 1 << 20, n_local + 3)
    film = pta.Film.from_planes(a_acc, a_mom, 3)
    film.add_planes(b_acc, b_mom, 14)
    got = film.read()
    assert same_bits(got[0], fm.merge(a_acc, b_acc)) and same_bits(got[1], fm.merge(a_mom, b_mom))
    film.add_planes(c_acc, c_mom, 1 << 20)
    got = film.read()
    want_acc, want_mom = fm.merge(fm.merge(a_acc, b_acc), c_acc), fm.merge(fm.merge(a_mom, b_mom), c_mom)
    assert same_bits(got[0], want_acc) and same_bits(got[1], want_mom)
    info = film.info
    assert (info.samples, info.passes, info.last_pass_samples) == (3 + 14 + (1 << 20), 3, 1 << 20)
    n = int(info.samples)
    want, w_err, w_sum, w_max = fm.noise(want_mom, n, 0.05)
    st, err, bsum, bmax = film.noise(0.05, want_planes=True)
    assert same_bits(err, w_err) and same_bits(bsum, w_sum) and same_bits(bmax, w_max) and st.as_dict() == want
    # the rules of a pass hold for planes too, and a refusal changes nothing
    assert film.lib.pt_film_add_planes(film.handle, (1 << 21) - 1, c_acc.ctypes.data, c_mom.ctypes.data) == pta.PT_ERR_INVALID
    assert film.lib.pt_film_add_planes(film.handle, 1 << 24, c_acc.ctypes.data, c_mom.ctypes.data) == pta.PT_ERR_INVALID
    assert film.lib.pt_film_add_planes(film.handle, 1 << 21, None, c_mom.ctypes.data) == pta.PT_ERR_INVALID
    got = film.read()
    assert same_bits(got[0], want_acc) and same_bits(got[1], want_mom) and film.info.samples == n
    # the measurement entry runs both kernels and leaves the film as it was
    film.kernel_times(reps=2)
    got = film.read()
    assert same_bits(got[0], want_acc) and same_bits(got[1], want_mom)
    film.reset()
    assert not film.read()[0].any() and not film.read()[1].any() and film.info.passes == 0
    film.close()


# ------------------------------------------------------------------------------------------------ passes
def conditions(pta):
    yield "unsharded", pta.Opts.make()
    yield "rank 1 of 3 shards of 8x32 tiles", pta.Opts.make(shard_rank=1, shard_count=3, tile_w=8, tile_h=32)
    yield "PT_FLAG_NO_GRIDS", pta.Opts.make(flags=PT_FLAG_NO_GRIDS)


@pytest.mark.parametrize("name", ("cube", "spheres"))
def test_passes_are_the_frames_of_render_moments_added_in_order(pta, name):
    h = host(pta, name)
    for label, opts in conditions(pta):
        g, ref = pta.GpuScene(h), pta.GpuScene(h)   # the film's scene and a second, fresh one for the frames
        frames = {n: ref.render_moments(pta.Profile.make(W, H, n, BOUNCES), opts) for n in (2, 4, 8)}
        film = pta.Film(pta.Profile.make(W, H, 999, BOUNCES), opts)     # (the profile's samples are ignored)
        n_local = int(pta.gpu_lib().pt_local_pixel_count(C.byref(pta.Profile.make(W, H, 1, BOUNCES)), C.byref(opts)))
        info = film.info
        assert (info.width, info.height, info.n_local, info.samples, info.passes, info.last_pass_samples) == (W, H, n_local, 0, 0, 0)
        for n in (2, 4, 8):
            film.add_pass(g, n)
        info = film.info
        assert (info.samples, info.passes, info.last_pass_samples) == (14, 3, 8), label
        acc, mom = film.read()
        want_acc = fm.merge(fm.merge(fm.merge(np.zeros_like(acc), frames[2][1]), frames[4][1]), frames[8][1])
        want_mom = fm.merge(fm.merge(fm.merge(np.zeros_like(mom), frames[2][2]), frames[4][2]), frames[8][2])
        assert same_bits(want_acc, (frames[2][1] + frames[4][1]) + frames[8][1])
        assert same_bits(acc, want_acc), (name, label)
        assert same_bits(mom, want_mom), (name, label)
        assert np.abs(acc).max() > 0 and (mom[:, 1] > 0).any()
        # the noise of rendered planes, held to the model as well
        want, w_err, w_sum, w_max = fm.noise(want_mom, 14, 0.05)
        st, err, bsum, bmax = film.noise(0.05, want_planes=True)
        assert same_bits(err, w_err) and same_bits(bsum, w_sum) and same_bits(bmax, w_max) and st.as_dict() == want, (name, label)
        # reset: zero passes, zero planes, the film takes the same passes again
        film.reset()
        info = film.info
        assert (info.samples, info.passes, info.last_pass_samples) == (0, 0, 0)
        assert not film.read()[0].any() and not film.read()[1].any()
        film.add_pass(g, 2)
        assert same_bits(film.read()[0], frames[2][1]) and same_bits(film.read()[1], frames[2][2])
        film.close()
        g.close()
        ref.close()


@pytest.mark.parametrize("name", ("cube", "spheres"))
def test_one_pass_is_a_render(pta, name):
    h = host(pta, name)
    g, ref = pta.GpuScene(h), pta.GpuScene(h)
    prof = pta.Profile.make(W, H, 4, BOUNCES)
    for tm in ("FILMIC", "ACES"):
        prof.tonemap = pta.TONEMAPS[tm]
        want_rgb, want_acc = ref.render(prof)
        film = pta.Film(prof)
        film.add_pass(g, 4)
        rgb, col = film.resolve(want_color=True)
        assert np.array_equal(rgb, want_rgb), (name, tm)
        assert same_bits(film.read()[0], want_acc), (name, tm)
        assert same_bits(col, fm.resolve_color(want_acc, 4))
        assert np.array_equal(film.resolve(), want_rgb) and np.array_equal(film.resolve(tm), want_rgb)
        only = np.empty_like(col)
        pta.check_gpu(film.lib.pt_film_resolve(film.handle, prof.tonemap, None, only.ctypes.data))
        assert same_bits(only, col)
        film.close()


def test_resolve_device_writes_nothing_past_the_image(pta):
    import torch
    accum, mom = fm.synthetic_planes(257, 14, 5)
    film = pta.Film.from_planes(accum, mom, 14)
    want_rgb, want_col = film.resolve(1, want_color=True)
    n, guard = 257 * 3, 32
    d_rgb = torch.full((n + guard,), 0xA5, dtype=torch.uint8, device="cuda")
    d_col = torch.full((n + guard,), -7.0, dtype=torch.float32, device="cuda")
    film.resolve_device(1, d_rgb.data_ptr(), d_col.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    rgb, col = d_rgb.cpu().numpy(), d_col.cpu().numpy()
    assert (rgb[n:] == 0xA5).all() and (col[n:] == f32(-7.0)).all()
    assert np.array_equal(rgb[:n].reshape(-1, 3), want_rgb) and same_bits(col[:n].reshape(-1, 3), want_col)
    film.close()


def test_a_film_session_leaves_the_scene_undisturbed(pta):
    import torch
    h = host(pta, "spheres")
    prof = pta.Profile.make(W, H, 4, BOUNCES)
    g = pta.GpuScene(h)
    for warm in (0, 4):   # a fresh scene, then one that has rendered four frames (planned, caches keyed)
        for _ in range(warm):
            g.render(prof)
        before = g.render(prof)
        film = pta.Film(prof)
        film.render_until(g, 2, 14, 0.0)
        assert film.info.samples == 14
        film.resolve()
        film.close()
        after = g.render(prof)
        assert np.array_equal(before[0], after[0]) and same_bits(before[1], after[1]), warm
    fresh = pta.GpuScene(h)
    want = fresh.render(prof)
    assert np.array_equal(before[0], want[0]) and same_bits(before[1], want[1])
    torch.cuda.synchronize()   # no HIP error is pending on the device the scene renders on
    assert float(torch.ones(4, device="cuda").sum().item()) == 4.0


# ------------------------------------------------------------------------------------------------ render_until
@pytest.mark.parametrize("name", ("cube", "spheres"))
def test_render_until_makes_the_models_passes(pta, name):
    h = host(pta, name)
    g = pta.GpuScene(h)
    prof = pta.Profile.make(64, 48, 1, BOUNCES)
    film = pta.Film(prof)

    def run(first, max_samples, target, lum_floor=0.01):
        film.reset()
        seen = []

        def on_pass(info, noise):
            seen.append((info.passes, info.last_pass_samples, info.samples, noise.as_dict(), film.read()[1]))
        out = film.render_until(g, first, max_samples, target, lum_floor, on_pass)
        # every reported noise is the model's over the planes read back after that pass
        for passes, last, total, st, mom in seen:
            assert st == fm.noise(mom, total, target, lum_floor)[0], (name, first, max_samples, target, passes)
        made, conv = fm.render_until(lambda k, total: seen[k][3]["mean_error"], first, max_samples, target)
        assert [s[1] for s in seen] == made and [s[0] for s in seen] == list(range(1, len(made) + 1))
        assert [s[2] for s in seen] == list(np.cumsum(made))
        assert out.as_dict() == seen[-1][3] and bool(out.converged) == conv
        assert film.info.samples == sum(made) <= max_samples
        return made, out, [x[3]["mean_error"] for x in seen]

    made, out, _ = run(4, 60, 0.0)        # target 0: to the last pass that fits
    assert made == fm.schedule(4, 60) == [4, 8, 16, 32] and not out.converged
    made, out, _ = run(4, 60, 1e9)        # a huge target: one pass
    assert made == [4] and out.converged == 1
    made, out, _ = run(2, 2, 0.0)
    assert made == [2] and not out.converged
    made, out, _ = run(8, 64, 0.0)
    assert made == [8, 16, 32]
    made, out, errors = run(2, 62, 0.0)   # a target between two passes' errors stops in the middle
    assert made == [2, 4, 8, 16, 32] and out.mean_error == errors[-1]
    assert errors[-1] < errors[0]         # (31 times the samples: the standard error of a mean falls as 1 / sqrt(n))
    k = int(np.argmin(errors))            # the first pass at or below errors[k] is pass k
    made, out, _ = run(2, 62, errors[k])
    assert made == [2, 4, 8, 16, 32][:k + 1] and out.converged == 1
    # a film that already has passes goes on doubling
    film.reset()
    film.add_pass(g, 3)
    out = film.render_until(g, 2, 21, 0.0)
    assert (film.info.passes, film.info.samples, film.info.last_pass_samples) == (3, 21, 12) and not out.converged
    film.close()


# ------------------------------------------------------------------------------------------------ composition
def test_the_films_device_planes_feed_the_variance_guided_filter(pta):
    import torch
    h = host(pta, "spheres")
    g = pta.GpuScene(h)
    prof = pta.Profile.make(W, H, 1, BOUNCES)
    film = pta.Film(prof)
    for n in (2, 4, 8):
        film.add_pass(g, n)
    n = int(film.info.samples)
    acc, mom = film.read()
    guides = g.render_guides(W, H)
    params = pta.DenoiseParams.default_var(tonemap=prof.tonemap)
    want_col, want_rgb = pta.denoise_var(W, H, n, params, acc, mom, guides)
    d_acc, d_mom = film.planes_device()
    assert d_acc and d_mom and d_acc % 256 == 0 and d_mom % 256 == 0
    d_guides = torch.from_numpy(guides).cuda()
    d_col = torch.empty(W * H * 3, dtype=torch.float32, device="cuda")
    d_rgb = torch.empty(W * H * 3, dtype=torch.uint8, device="cuda")
    d_scratch = torch.empty(pta.denoise_var_scratch_bytes(W, H) + 256, dtype=torch.uint8, device="cuda")
    scratch = (d_scratch.data_ptr() + 255) & ~255
    pta.check_gpu(pta.gpu_lib().pt_denoise_var_device(0, W, H, n, C.byref(params), d_acc, d_mom, d_guides.data_ptr(),
                                                      d_col.data_ptr(), d_rgb.data_ptr(), scratch,
                                                      torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert same_bits(d_col.cpu().numpy().reshape(-1, 3), want_col)
    assert np.array_equal(d_rgb.cpu().numpy().reshape(-1, 3), want_rgb)
    after = film.read()
    assert same_bits(after[0], acc) and same_bits(after[1], mom)   # the filter only read the planes
    film.close()


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_leave_the_film_unchanged(pta):
    """Every refusal is PT_ERR_INVALID or PT_ERR_UNSUPPORTED before any device work.  (The foreign-device case needs a second
    GPU to make a film on; on a machine with one it is the only case not exercised.)"""
    import torch
    INVALID = pta.PT_ERR_INVALID
    h = host(pta, "cube")
    g = pta.GpuScene(h)
    prof = pta.Profile.make(W, H, 1, BOUNCES)
    film = pta.Film(prof)
    lib = film.lib
    film.add_pass(g, 2)
    film.add_pass(g, 4)
    before = film.read()

    def unchanged():
        now, i = film.read(), film.info
        return same_bits(now[0], before[0]) and same_bits(now[1], before[1]) and (i.samples, i.passes, i.last_pass_samples) == (6, 2, 4)
    out = pta.FilmNoise()
    rgb, col = np.empty((W * H, 3), np.uint8), np.empty((W * H, 3), f32)
    for samples in (0, 1, 4, 7):     # smaller than twice the last pass
        assert lib.pt_film_add_pass(film.handle, g.handle, samples) == INVALID, samples
    assert lib.pt_film_add_pass(film.handle, g.handle, (1 << 24) - 5) == INVALID   # a total above 2^24
    assert lib.pt_film_add_pass(film.handle, None, 8) == INVALID and lib.pt_film_add_pass(None, g.handle, 8) == INVALID
    assert lib.pt_film_resolve(film.handle, prof.tonemap, None, None) == INVALID
    assert lib.pt_film_resolve_device(film.handle, prof.tonemap, None, None, None) == INVALID
    assert lib.pt_film_resolve(film.handle, 3, rgb.ctypes.data, None) == INVALID and lib.pt_film_resolve(None, 1, rgb.ctypes.data, None) == INVALID
    for lum_floor, target in ((0.0, 0.1), (-1.0, 0.1), (np.inf, 0.1), (np.nan, 0.1), (0.01, -1e-9), (0.01, np.inf), (0.01, np.nan)):
        assert lib.pt_film_noise(film.handle, lum_floor, target, C.byref(out), None, None, None) == INVALID, (lum_floor, target)
        assert lib.pt_film_render_until(film.handle, g.handle, 2, 100, lum_floor, target, C.cast(None, pta.FILM_PASS_FN), None, C.byref(out)) == INVALID
    assert lib.pt_film_noise(film.handle, 0.01, 0.1, None, None, None, None) == INVALID
    assert lib.pt_film_noise(None, 0.01, 0.1, C.byref(out), None, None, None) == INVALID
    for first in (0, 1):
        assert lib.pt_film_render_until(film.handle, g.handle, first, 100, 0.01, 0.1, C.cast(None, pta.FILM_PASS_FN), None, C.byref(out)) == INVALID
    assert lib.pt_film_render_until(film.handle, None, 2, 100, 0.01, 0.1, C.cast(None, pta.FILM_PASS_FN), None, C.byref(out)) == INVALID
    assert lib.pt_film_render_until(film.handle, g.handle, 2, 100, 0.01, 0.1, C.cast(None, pta.FILM_PASS_FN), None, None) == INVALID
    info = pta.FilmInfo()
    assert lib.pt_film_get_info(None, C.byref(info)) == INVALID and lib.pt_film_get_info(film.handle, None) == INVALID
    assert lib.pt_film_read(None, col.ctypes.data, None) == INVALID and lib.pt_film_reset(None) == INVALID
    if torch.cuda.device_count() > 1:   # a scene on another device than the film's
        other = pta.Film(prof, device=1)
        assert lib.pt_film_add_pass(other.handle, g.handle, 2) == INVALID
        assert lib.pt_film_render_until(other.handle, g.handle, 2, 100, 0.01, 0.1, C.cast(None, pta.FILM_PASS_FN), None, C.byref(out)) == INVALID
        assert other.info.samples == 0 and not other.read()[0].any()
        other.close()
        torch.cuda.set_device(0)
    assert unchanged()
    # an empty film: nothing to resolve, no noise; first > max
    empty = pta.Film(prof)
    assert lib.pt_film_resolve(empty.handle, prof.tonemap, rgb.ctypes.data, None) == INVALID
    assert lib.pt_film_noise(empty.handle, 0.01, 0.1, C.byref(out), None, None, None) == INVALID
    assert lib.pt_film_render_until(empty.handle, g.handle, 8, 7, 0.01, 0.1, C.cast(None, pta.FILM_PASS_FN), None, C.byref(out)) == INVALID
    assert empty.info.samples == 0 and not empty.read()[0].any()
    empty.add_pass(g, 1)   # a total of one sample has no variance
    assert lib.pt_film_noise(empty.handle, 0.01, 0.1, C.byref(out), None, None, None) == INVALID
    assert empty.info.samples == 1
    empty.close()
    # the megakernel stages no samples; options pt_render refuses; a rank without pixels
    handle = C.c_void_p()
    mega = pta.Opts.make(flags=PT_FLAG_MEGAKERNEL)
    assert lib.pt_film_create(0, C.byref(prof), C.byref(mega), C.byref(handle)) == pta.PT_ERR_UNSUPPORTED and not handle.value
    assert lib.pt_film_create(0, None, None, C.byref(handle)) == INVALID and lib.pt_film_create(0, C.byref(prof), None, None) == INVALID
    bad = pta.Opts.make(shard_rank=3, shard_count=3)
    assert lib.pt_film_create(0, C.byref(prof), C.byref(bad), C.byref(handle)) == INVALID
    tiny = pta.Opts.make(shard_rank=1, shard_count=2)   # one 32x32 tile: rank 1 has none
    assert lib.pt_film_create(0, C.byref(pta.Profile.make(16, 16, 1, BOUNCES)), C.byref(tiny), C.byref(handle)) == INVALID
    assert not handle.value
    # a film from planes has no profile
    accum, mom = fm.synthetic_planes(W * H, 6, 1)
    planes = pta.Film.from_planes(accum, mom, 6, 4)
    assert lib.pt_film_add_pass(planes.handle, g.handle, 8) == INVALID
    assert lib.pt_film_render_until(planes.handle, g.handle, 2, 100, 0.01, 0.1, C.cast(None, pta.FILM_PASS_FN), None, C.byref(out)) == INVALID
    got = planes.read()
    assert same_bits(got[0], accum) and same_bits(got[1], mom) and planes.info.samples == 6
    planes.close()
    create = lib.pt_film_create_from_planes
    for n_local, samples, last in ((0, 6, 4), (W * H, 0, 1), (W * H, (1 << 24) + 1, 1), (W * H, 6, 0), (W * H, 6, 7)):
        assert create(0, n_local, samples, last, accum.ctypes.data, mom.ctypes.data, C.byref(handle)) == INVALID
    assert create(0, W * H, 6, 4, None, mom.ctypes.data, C.byref(handle)) == INVALID
    assert create(0, W * H, 6, 4, accum.ctypes.data, None, C.byref(handle)) == INVALID
    assert create(0, W * H, 6, 4, accum.ctypes.data, mom.ctypes.data, None) == INVALID
    assert not handle.value
    lib.pt_film_destroy(None)
    assert unchanged()
    film.add_pass(g, 8)   # and the film still takes the pass it is due
    assert film.info.samples == 14
    film.close()
    torch.cuda.synchronize()
