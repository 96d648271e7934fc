"""The film filter on the GPU: pt_film_denoise on a uniform film against pt_denoise_device / pt_denoise_var_device
bit for bit, on a non-uniform film of synthetic planes against tests/film_denoise_model.py bit for bit (colour, rgb8, ferr,
tile sums and maxima), what the family refuses, pt_film_render_until_filtered against the model's run over the planes read
back after every pass, and the film's lazily made scratch: when it appears, that a reset keeps it, that destroy frees it."""
import ctypes as C

import numpy as np
import pytest

import denoise_model as dm
import denoise_var_model as dvm
import film_adaptive_model as am
import film_denoise_model as fdm
import film_model as fm
from conftest import SCENES

pytestmark = pytest.mark.gpu

f32 = np.float32
BOUNCES = 2
SHAPES = ((72, 40, 16, 16), (70, 50, 32, 8))     # both with clipped edge tiles
SHAPE_IDS = ("72x40 in 16x16", "70x50 in 32x8")
W, H, TILE = 72, 40, 16
TILING = am.Tiling(W, H, TILE, TILE)
EVERY = list(range(15))


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def same_bits(a, b):
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    return a.shape == b.shape and bool((bits(a) == bits(b)).all())


def host(pta, name):
    return pta.HostScene.load_isf(SCENES / name / "scene.isf")


def make_film(pta, w=W, h=H, tw=TILE, th=TILE, **opts):
    return pta.Film(pta.Profile.make(w, h, 1, BOUNCES), pta.Opts.make(tile_w=tw, tile_h=th, **opts))


def parent_device_bytes(n_local):
    """What pt_film_create allocates."""
    up = lambda floats: (floats + 63) & ~63   # noqa: E731
    return 4 * (2 * (up(3 * n_local) + up(2 * n_local)) + up(n_local) + 2 * up((n_local + 255) // 256))


def on_device(film, params, variance, guides, want_ferr, lum_floor=0.01, tiles=False):
    """pt_film_denoise_device (and pt_film_tile_reduce_device over its ferr) on torch tensors and torch's current stream, with
    guard bytes behind every output."""
    import torch
    n, guard = int(film.info.n_local), 64
    stream = torch.cuda.current_stream().cuda_stream
    d_g = torch.from_numpy(np.ascontiguousarray(guides, f32)).cuda()
    d_col = torch.full((3 * n + guard,), -7.0, dtype=torch.float32, device="cuda")
    d_rgb = torch.full((3 * n + guard,), 0xA5, dtype=torch.uint8, device="cuda")
    d_ferr = torch.full((n + guard,), -7.0, dtype=torch.float32, device="cuda")
    d_scratch = torch.empty(film.denoise_scratch_bytes(), dtype=torch.uint8, device="cuda")
    assert d_scratch.data_ptr() % 256 == 0 and d_g.data_ptr() % 16 == 0
    film.denoise_device(params, variance, d_g.data_ptr(), d_col.data_ptr(), d_rgb.data_ptr(),
                        d_ferr.data_ptr() if want_ferr else None, d_scratch.data_ptr(), lum_floor, stream)
    out = []
    if tiles:
        nt = int(film.adaptive_info.n_tiles)
        d_ts = torch.full((2 * nt + guard,), -7.0, dtype=torch.float32, device="cuda")
        film.tile_reduce_device(d_ferr.data_ptr(), d_ts.data_ptr(), d_ts.data_ptr() + 4 * nt, stream)
        torch.cuda.synchronize()
        ts = d_ts.cpu().numpy()
        assert (ts[2 * nt:] == f32(-7.0)).all()
        out = [ts[:nt], ts[nt:2 * nt]]
    torch.cuda.synchronize()
    col, rgb, ferr = d_col.cpu().numpy(), d_rgb.cpu().numpy(), d_ferr.cpu().numpy()
    assert (col[3 * n:] == f32(-7.0)).all() and (rgb[3 * n:] == 0xA5).all() and (ferr[n:] == f32(-7.0)).all()
    if not want_ferr:
        assert (ferr == f32(-7.0)).all()
    return [col[:3 * n].reshape(n, 3), rgb[:3 * n].reshape(n, 3), ferr[:n] if want_ferr else None] + out


def reference_on_device(pta, w, h, samples, params, variance, d_acc, d_mom, guides):
    """pt_denoise_device / pt_denoise_var_device on the film's own device planes."""
    import torch
    n = w * h
    lib = pta.gpu_lib()
    d_g = torch.from_numpy(np.ascontiguousarray(guides, f32)).cuda()
    d_col = torch.empty((n, 3), dtype=torch.float32, device="cuda")
    d_rgb = torch.empty((n, 3), dtype=torch.uint8, device="cuda")
    d_scratch = torch.empty(max(1, pta.denoise_scratch_bytes(w, h)), dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    if variance:
        pta.check_gpu(lib.pt_denoise_var_device(0, w, h, samples, C.byref(params), d_acc, d_mom, d_g.data_ptr(), d_col.data_ptr(),
                                                d_rgb.data_ptr(), d_scratch.data_ptr(), stream))
    else:
        pta.check_gpu(lib.pt_denoise_device(0, w, h, samples, C.byref(params), d_acc, d_g.data_ptr(), d_col.data_ptr(),
                                            d_rgb.data_ptr(), d_scratch.data_ptr(), stream))
    torch.cuda.synchronize()
    return d_col.cpu().numpy(), d_rgb.cpu().numpy()


def filter_params(pta, variance, **changes):
    return (pta.DenoiseParams.default_var if variance else pta.DenoiseParams.default)(**changes)


# ------------------------------------------------------------------------------------------------ a uniform film
@pytest.mark.parametrize("name", ("cube", "spheres"))
def test_a_uniform_film_is_filtered_like_its_planes(pta, name):
    g = pta.GpuScene(host(pta, name))
    film = make_film(pta)
    film.add_pass(g, 4)
    film.add_pass(g, 8)
    guides = g.render_guides(W, H)
    d_acc, d_mom = film.planes_device()
    before = film.info.device_bytes
    for variance in (0, 1):
        for it in (0, 1, 3):
            for fl in (0, pta.PT_DENOISE_NO_DEMODULATE):
                params = filter_params(pta, variance, iterations=it, flags=fl, tonemap=("FILMIC", "ACES")[it % 2])
                want_col, want_rgb = reference_on_device(pta, W, H, 12, params, variance, d_acc, d_mom, guides)
                col, rgb, ferr = on_device(film, params, variance, guides, bool(variance))
                assert same_bits(col, want_col) and np.array_equal(rgb, want_rgb), (name, variance, it, fl)
                if variance:     # the error output changes neither image
                    col2, rgb2, _ = on_device(film, params, variance, guides, False)
                    assert same_bits(col2, col) and np.array_equal(rgb2, rgb)
                    assert np.isfinite(ferr).all() and (ferr >= 0).all()
                if it == 0:
                    r_rgb, r_col = film.resolve(int(params.tonemap), want_color=True)
                    assert same_bits(col, r_col) and np.array_equal(rgb, r_rgb), (name, variance, fl)
                    if variance:
                        assert same_bits(ferr, film.noise(0.05, want_planes=True)[1])
    assert film.info.device_bytes == before == parent_device_bytes(W * H)    # (the device form allocates nothing)
    # the host form renders the same guides itself
    params = pta.DenoiseParams.default_var(iterations=3)
    col, rgb, ferr = film.denoise(g, params, want_ferr=True)
    d_col, d_rgb, d_ferr = on_device(film, params, 1, guides, True)
    assert same_bits(col, d_col) and np.array_equal(rgb, d_rgb) and same_bits(ferr, d_ferr)
    assert (ferr[guides[:, 3] >= 0] > 0).any()
    pcol, prgb = film.denoise(g, pta.DenoiseParams.default(iterations=2), variance=False)
    d_col, d_rgb, _ = on_device(film, pta.DenoiseParams.default(iterations=2), 0, guides, False)
    assert same_bits(pcol, d_col) and np.array_equal(prgb, d_rgb)
    film.close()
    g.close()


# ------------------------------------------------------------------------------------------------ a non-uniform film
def synthetic_film(pta, w, h, tw, th, seed):
    """A film of counts 2 / 6 / 18 in adjacent tiles from synthetic planes, and synthetic guides with invalid pixels, a depth
    edge, zero normals and a non-finite normal.  Returns (film, tiling, accum, moments, counts, guides)."""
    t = am.Tiling(w, h, tw, th)
    n = t.n_pixels
    film = make_film(pta, w, h, tw, th)
    _, acc, guides = dm.synthetic_inputs(w, h, seed)
    acc = (acc / f32(2)).astype(f32)                     # (synthetic_inputs makes a sum of 4 samples)
    mom = dvm.synthetic_moments(2, acc, seed + 1)
    film.add_planes(acc, mom, 2)
    counts = np.full(n, 2, np.uint32)
    third = [k for k in range(t.n_tiles) if k % 3 != 0]
    ninth = [k for k in range(t.n_tiles) if k % 3 == 2]
    for samples, tiles in ((4, third), (12, ninth)):
        where = t.pixel_map(tiles)
        _, p_acc, _ = dm.synthetic_inputs(len(where), 1, seed + samples)
        p_acc = (p_acc * f32(samples / 4)).astype(f32)
        p_mom = dvm.synthetic_moments(samples, p_acc, seed + samples + 1)
        film.add_tile_planes(p_acc, p_mom, samples, tiles)
        acc, mom, counts = am.merge_tiles(t, acc, mom, counts, tiles, p_acc, p_mom, samples)
    got = film.read()
    assert same_bits(got[0], acc) and same_bits(got[1], mom) and np.array_equal(film.read_counts(), counts)
    assert sorted(set(counts.tolist())) == [2, 6, 18]
    guides = guides.copy()
    y, x = np.divmod(np.arange(n), w)
    guides[(x >= w // 2) & (guides[:, 3] >= 0), 3] += f32(15.0)      # a depth edge down the middle
    valid = np.flatnonzero(guides[:, 3] >= 0)
    guides[valid[5], 0:3] = (np.inf, 0.0, 1.0)                       # a non-finite normal
    guides[valid[9], 0:3] = 0.0                                      # a zero normal (synthetic_inputs has a cluster of them too)
    return film, t, acc, mom, counts, guides


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_a_non_uniform_film_equals_the_model_bit_for_bit(pta, oracle, shape):
    w, h, tw, th = shape
    film, t, acc, mom, counts, guides = synthetic_film(pta, w, h, tw, th, 500 + w)
    valid = guides[:, 3] >= 0
    assert (~valid).any() and valid.any()
    # counts differ under the taps of step 1, 2 and 4: some valid pixel has a valid neighbour of another count at that distance
    c2, v2 = counts.reshape(h, w), valid.reshape(h, w)
    for s in (1, 2, 4):
        differ = (c2[:, s:] != c2[:, :-s]) & v2[:, s:] & v2[:, :-s]
        assert differ.any(), s
    for variance in (1, 0):
        for k, (it, fl) in enumerate((it, fl) for it in (0, 1, 3) for fl in (0, pta.PT_DENOISE_NO_DEMODULATE)):
            params = filter_params(pta, variance, iterations=it, flags=fl, tonemap=k % 3, normal_power_log2=(0, 3, 10)[k % 3],
                                   sigma_depth=(0.5, 4.0)[k % 2])
            floor = (0.01, 0.5)[k % 2]
            want_col, want_ferr = fdm.film_denoise_with(params, w, h, counts, acc, mom, guides, bool(variance), floor)
            want_rgb = oracle.post_process(pta.Profile.make(w, h, 1, 1, int(params.tonemap)), want_col)
            got = on_device(film, params, variance, guides, bool(variance), floor, tiles=bool(variance))
            assert same_bits(got[0], want_col), (variance, it, fl, int((bits(got[0]) != bits(want_col)).any(axis=1).sum()))
            assert np.array_equal(got[1], want_rgb), (variance, it, fl)
            if it == 0:
                r_rgb, r_col = film.resolve(int(params.tonemap), want_color=True)
                assert same_bits(got[0], r_col) and np.array_equal(got[1], r_rgb)
            if not variance:
                continue
            assert same_bits(got[2], want_ferr), (it, fl, int((bits(got[2]) != bits(want_ferr)).sum()))
            assert np.isfinite(want_ferr).all()
            w_sum, w_max = fdm.tile_reduce(t, want_ferr)
            assert same_bits(got[3], w_sum) and same_bits(got[4], w_max), (it, fl)
            assert same_bits(want_ferr[~valid], am.pixel_error(mom, counts, floor)[~valid])
            if it:
                assert not same_bits(want_ferr[valid], am.pixel_error(mom, counts, floor)[valid])
    film.close()


# ------------------------------------------------------------------------------------------------ refusals
def test_what_the_film_filter_refuses(pta):
    import torch
    g = pta.GpuScene(host(pta, "cube"))
    film, t, acc, mom, counts, guides = synthetic_film(pta, W, H, TILE, TILE, 77)
    lib, INVALID = film.lib, pta.PT_ERR_INVALID
    n, nt = W * H, t.n_tiles
    d_g = torch.from_numpy(np.ascontiguousarray(guides, f32)).cuda()
    d_col = torch.full((3 * n,), -7.0, dtype=torch.float32, device="cuda")
    d_rgb = torch.full((3 * n,), 0xA5, dtype=torch.uint8, device="cuda")
    d_ferr = torch.full((n,), -7.0, dtype=torch.float32, device="cuda")
    d_scratch = torch.empty(film.denoise_scratch_bytes(), dtype=torch.uint8, device="cuda")
    col, rgb, ferr = np.full((n, 3), -7.0, f32), np.full((n, 3), 0xA5, np.uint8), np.full(n, -7.0, f32)
    tsum, tmax = np.full(nt, -7.0, f32), np.full(nt, -7.0, f32)
    stats = pta.FilmTileStats()
    before_info = film.info
    pv, pp = pta.DenoiseParams.default_var(iterations=2), pta.DenoiseParams.default(iterations=2)

    def device(f=film, variance=1, p=pv, floor=0.01, gd=d_g.data_ptr(), out=(d_col.data_ptr(), d_rgb.data_ptr(), d_ferr.data_ptr()),
               scratch=d_scratch.data_ptr()):
        return lib.pt_film_denoise_device(f.handle if f else None, variance, C.byref(p) if p else None, floor, gd, *out, scratch, 0)

    def hostf(f=film, scene=g, variance=1, p=pv, floor=0.01, out=(rgb.ctypes.data, col.ctypes.data, ferr.ctypes.data)):
        return lib.pt_film_denoise(f.handle if f else None, scene.handle if scene else None, variance, C.byref(p) if p else None,
                                   floor, *out)

    def noise(f=film, scene=g, p=pv, floor=0.01, target=0.05, out=stats):
        return lib.pt_film_filtered_noise(f.handle if f else None, scene.handle if scene else None, C.byref(p) if p else None, floor,
                                          target, C.byref(out) if out is not None else None, ferr.ctypes.data, tsum.ctypes.data,
                                          tmax.ctypes.data)

    def untouched(f=film):
        torch.cuda.synchronize()
        now, i = f.read(), f.info
        return ((d_col == -7.0).all().item() and (d_rgb == 0xA5).all().item() and (d_ferr == -7.0).all().item()
                and (col == f32(-7.0)).all() and (rgb == 0xA5).all() and (ferr == f32(-7.0)).all() and (tsum == f32(-7.0)).all()
                and (tmax == f32(-7.0)).all() and same_bits(now[0], acc) and same_bits(now[1], mom)
                and np.array_equal(f.read_counts(), counts)
                and (i.samples, i.passes, i.last_pass_samples, i.device_bytes)
                == (before_info.samples, before_info.passes, before_info.last_pass_samples, before_info.device_bytes))
    # null pointers
    assert device(f=None) == INVALID and device(p=None) == INVALID and device(gd=None) == INVALID
    assert device(out=(None, None, None)) == INVALID and device(scratch=None) == INVALID
    assert hostf(f=None) == INVALID and hostf(scene=None) == INVALID and hostf(p=None) == INVALID and hostf(out=(None, None, None)) == INVALID
    assert noise(f=None) == INVALID and noise(scene=None) == INVALID and noise(p=None) == INVALID and noise(out=None) == INVALID
    # the plain filter has no variance
    assert device(variance=0, p=pp) == INVALID and hostf(variance=0, p=pp) == INVALID and device(variance=2) == INVALID
    # lum_floor
    for floor in (0.0, -1.0, float("nan"), float("inf")):
        assert device(floor=floor) == INVALID and hostf(floor=floor) == INVALID and noise(floor=floor) == INVALID, floor
        assert device(variance=0, p=pp, floor=floor, out=(d_col.data_ptr(), d_rgb.data_ptr(), None)) == INVALID
    for target in (-1.0, float("nan"), float("inf")):
        assert noise(target=target) == INVALID
    # every parameter rule of pt_denoise / pt_denoise_var
    for change in ({"iterations": 9}, {"flags": 2}, {"normal_power_log2": 11}, {"tonemap": 7}, {"sigma_depth": 0.0},
                   {"sigma_depth": float("nan")}, {"sigma_color": -1.0}, {"sigma_color": float("inf")}):
        for variance in (0, 1):
            p = filter_params(pta, variance, **change)
            out = (d_col.data_ptr(), d_rgb.data_ptr(), d_ferr.data_ptr() if variance else None)
            assert device(variance=variance, p=p, out=out) == INVALID, (change, variance)
        assert hostf(p=pta.DenoiseParams.default_var(**change)) == INVALID and noise(p=pta.DenoiseParams.default_var(**change)) == INVALID
    assert device(p=pta.DenoiseParams.default_var(sigma_color=0.0)) == INVALID      # (the luminance sigma must be positive)
    fp = pta.FilmFilteredParams.default(filter=pta.DenoiseParams.default_var(sigma_color=0.0))
    none = C.cast(None, pta.FILM_PASS_FN)
    assert lib.pt_film_render_until_filtered(film.handle, g.handle, C.byref(fp), none, None, C.byref(stats)) == INVALID
    for change in ({"first_pass_samples": 1}, {"dilate": 2}, {"lum_floor": 0.0}, {"target": -1.0}):
        fp = pta.FilmFilteredParams.default(**change)
        assert lib.pt_film_render_until_filtered(film.handle, g.handle, C.byref(fp), none, None, C.byref(stats)) == INVALID, change
    fp = pta.FilmFilteredParams.default()
    assert lib.pt_film_render_until_filtered(None, g.handle, C.byref(fp), none, None, C.byref(stats)) == INVALID
    assert lib.pt_film_render_until_filtered(film.handle, None, C.byref(fp), none, None, C.byref(stats)) == INVALID
    assert lib.pt_film_render_until_filtered(film.handle, g.handle, None, none, None, C.byref(stats)) == INVALID
    assert lib.pt_film_render_until_filtered(film.handle, g.handle, C.byref(fp), none, None, None) == INVALID
    assert lib.pt_film_tile_reduce_device(film.handle, None, d_ferr.data_ptr(), d_ferr.data_ptr(), 0) == INVALID
    assert untouched()
    # a film without a profile, a sharded film: no scratch size either
    planes = pta.Film.from_planes(acc, mom, 4)
    sharded = make_film(pta, shard_rank=0, shard_count=2)
    for f in (planes, sharded):
        assert f.denoise_scratch_bytes() == 0
        assert device(f=f) == INVALID and hostf(f=f) == INVALID and noise(f=f) == INVALID
        assert lib.pt_film_render_until_filtered(f.handle, g.handle, C.byref(fp), none, None, C.byref(stats)) == INVALID
        assert lib.pt_film_tile_reduce_device(f.handle, d_ferr.data_ptr(), d_ferr.data_ptr(), d_ferr.data_ptr(), 0) == INVALID
    # a pixel with no samples; the variance filter with a pixel below two
    empty = make_film(pta)
    assert device(f=empty) == INVALID and hostf(f=empty) == INVALID and noise(f=empty) == INVALID
    assert device(f=empty, variance=0, p=pp, out=(d_col.data_ptr(), d_rgb.data_ptr(), None)) == INVALID
    one = make_film(pta)
    one.add_planes(acc, mom, 1)
    assert device(f=one) == INVALID and hostf(f=one) == INVALID and noise(f=one) == INVALID
    where = TILING.pixel_map([3])
    one.add_tile_planes(acc[where], mom[where], 2, [3])          # tile 3 has three samples, every other tile one
    assert device(f=one) == INVALID and hostf(f=one) == INVALID and noise(f=one) == INVALID
    # ... and the filtered loop on such a film, where it would measure before it renders: refused before the scratch is made
    bytes_one = one.info.device_bytes
    for change in ({"uniform_samples": 1}, {"uniform_samples": 1000, "max_samples": 4}):
        fp = pta.FilmFilteredParams.default(first_pass_samples=2, **change)
        assert lib.pt_film_render_until_filtered(one.handle, g.handle, C.byref(fp), none, None, C.byref(stats)) == INVALID, change
    assert one.info.device_bytes == bytes_one and (one.info.samples, one.info.passes) == (3, 2)
    assert untouched()
    assert device(f=one, variance=0, p=pp, out=(d_col.data_ptr(), d_rgb.data_ptr(), None)) == 0      # (the plain filter needs one)
    torch.cuda.synchronize()
    assert not (d_col == -7.0).any().item()
    # a scene on another device than the film's
    if torch.cuda.device_count() > 1:
        far = make_film_on(pta, 1)
        assert hostf(f=far) == INVALID and noise(f=far) == INVALID
        fp = pta.FilmFilteredParams.default()
        assert lib.pt_film_render_until_filtered(far.handle, g.handle, C.byref(fp), none, None, C.byref(stats)) == INVALID
        ms = np.zeros(4, f32)
        assert lib.pt_film_denoise_kernel_times(far.handle, g.handle, C.byref(pv), 0.01, 1, *(ms[i:].ctypes.data for i in range(4))) == INVALID
        far.close()
    for f in (film, planes, sharded, empty, one):
        f.close()
    g.close()


def make_film_on(pta, device):
    film = pta.Film(pta.Profile.make(W, H, 1, BOUNCES), pta.Opts.make(tile_w=TILE, tile_h=TILE), device=device)
    acc, mom = fm.synthetic_planes(W * H, 4, 5)
    film.add_planes(acc, mom, 4)
    return film


# ------------------------------------------------------------------------------------------------ render_until_filtered
FILTERED_TARGET = 0.02      # (the model's run over these frames makes 15, 4, 1, 1 tiles with dilate 0 and 15, 12, 11, 6 with 1)


@pytest.mark.parametrize("dilate", (0, 1))
def test_render_until_filtered_makes_the_models_passes(pta, dilate):
    g = pta.GpuScene(host(pta, "cube"))
    film = make_film(pta)
    guides = g.render_guides(W, H)
    target, lum_floor, budget = FILTERED_TARGET, 0.01, 120
    flt = pta.DenoiseParams.default_var(iterations=2)
    params = pta.FilmFilteredParams.default(filter=flt, target=target, lum_floor=lum_floor, first_pass_samples=8, uniform_samples=8,
                                            dilate=dilate, max_samples=budget)
    seen = []

    def on_pass(info, noise):
        seen.append({"info": (info.passes, info.last_pass_samples, info.samples), "noise": noise.as_dict(),
                     "planes": film.read(), "counts": film.read_counts()})
    out = film.render_until_filtered(g, params, on_pass)
    assert seen
    rendered, stats, sums = [], [], []
    counts = np.zeros(W * H, np.uint32)
    for s in seen:
        moved = s["counts"] != counts
        tiles = [k for k in EVERY if moved[TILING.pixels(k)].any()]
        assert (s["counts"][moved] - counts[moved] == s["info"][1]).all() and all(moved[TILING.pixels(k)].all() for k in tiles)
        counts = s["counts"]
        st, _, tsum, _ = fdm.filtered_noise(TILING, flt, counts, s["planes"][0], s["planes"][1], guides, target, lum_floor,
                                            active_tiles=len(tiles))
        rendered.append(tiles)
        stats.append(st)
        sums.append(tsum)
        assert s["noise"] == {"mean_error": st["mean_error"], "max_block_error": st["max_tile_error"],
                              "fraction_over": st["over_tiles"] / 15, "samples": st["samples"], "n_blocks": 15,
                              "converged": st["converged"]}
        assert s["info"][2] == st["samples"] == int(counts.max())
    made, why = fdm.render_until_filtered(TILING, lambda k, samples, tiles: sums[k], 8, 8, dilate, target, budget)
    assert [m[0] for m in made] == [s["info"][1] for s in seen]
    assert [m[1] for m in made] == rendered
    assert out.as_dict() == stats[-1] and bool(out.converged) == (why == "converged")
    # what makes this a test of the filtered selection (from the model, not hard-coded): at least two tile passes, a tile dropped
    tile_passes = [r for r in rendered if len(r) < 15]
    assert len(tile_passes) >= 2 and rendered[0] == EVERY, [len(r) for r in rendered]
    assert rendered[1] == am.dilate(TILING, am.candidates(TILING, sums[0], target), dilate)
    # ... and it is not the raw selection: the raw error of the same planes keeps other tiles
    raw_first = am.candidates(TILING, am.tile_noise(TILING, seen[0]["planes"][1], seen[0]["counts"], target, lum_floor)[2], target)
    assert raw_first != am.candidates(TILING, sums[0], target)
    # the library's own figures and planes after the run
    st, ferr, tsum, tmax = film.filtered_noise(g, flt, target, lum_floor, want_planes=True)
    w_st, w_ferr, w_sum, w_max = fdm.filtered_noise(TILING, flt, counts, seen[-1]["planes"][0], seen[-1]["planes"][1], guides, target,
                                                    lum_floor)
    assert same_bits(ferr, w_ferr) and same_bits(tsum, w_sum) and same_bits(tmax, w_max) and st.as_dict() == w_st
    # every pixel is still the sum of the whole frames' pixels it took part in (the same pt_render_tiles planes)
    o = pta.Opts.make(tile_w=TILE, tile_h=TILE)
    acc, mom = np.zeros((W * H, 3), f32), np.zeros((W * H, 2), f32)
    cnt = np.zeros(W * H, np.uint32)
    for (samples, tiles) in made:
        _, p_acc, p_mom = g.render_tiles(pta.Profile.make(W, H, samples, BOUNCES), tiles, o)
        acc, mom, cnt = am.merge_tiles(TILING, acc, mom, cnt, tiles, p_acc, p_mom, samples)
    assert same_bits(seen[-1]["planes"][0], acc) and same_bits(seen[-1]["planes"][1], mom) and np.array_equal(cnt, counts)
    # called again with the same budget: the film measures what it holds and renders nothing
    again = film.render_until_filtered(g, params)
    assert np.array_equal(film.read_counts(), counts) and again.as_dict() == dict(stats[-1], active_tiles=0)
    film.close()
    g.close()


def test_a_generous_filtered_target_keeps_the_film_uniform(pta):
    g = pta.GpuScene(host(pta, "cube"))
    film = make_film(pta)
    out = film.render_until_filtered(g, pta.FilmFilteredParams.default(target=1e9, first_pass_samples=4, max_samples=60))
    assert out.converged == 1 and out.active_tiles == 15 and film.info.samples == 4 and film.adaptive_info.uniform == 1
    other = make_film(pta)
    other.render_until(g, 4, 4, 0.0)
    assert same_bits(film.read()[0], other.read()[0]) and same_bits(film.read()[1], other.read()[1])
    # target 0 with every pass whole: pt_film_render_until's film
    film.reset()
    other.reset()
    out = film.render_until_filtered(g, pta.FilmFilteredParams.default(target=0.0, first_pass_samples=4, max_samples=60,
                                                                       uniform_samples=1000))
    other.render_until(g, 4, 60, 0.0)
    assert film.info.samples == other.info.samples == 60 and film.adaptive_info.uniform == 1 and not out.converged
    assert same_bits(film.read()[0], other.read()[0]) and same_bits(film.read()[1], other.read()[1])
    for f in (film, other):
        f.close()
    g.close()


# ------------------------------------------------------------------------------------------------ scratch
def test_the_scratch_appears_with_the_first_host_call_and_outlives_a_reset(pta):
    g = pta.GpuScene(host(pta, "cube"))
    film = make_film(pta)
    parent = parent_device_bytes(W * H)
    film.add_pass(g, 4)
    film.resolve()
    film.noise(0.05)
    assert film.info.device_bytes == parent
    scratch = film.denoise_scratch_bytes()
    assert scratch >= pta.denoise_var_scratch_bytes(W, H) + 4 * W * H + 2 * 4 * 15 and scratch % 256 == 0
    assert film.info.device_bytes == parent                      # (asking for the size allocates nothing)
    film.denoise(g, pta.DenoiseParams.default_var())
    held = film.info.device_bytes - parent
    assert held == scratch + 32 * W * H                          # the scratch and a plane of guides
    film.filtered_noise(g, pta.DenoiseParams.default_var(), 0.05)
    film.denoise(g, pta.DenoiseParams.default(), variance=False)
    assert film.info.device_bytes - parent == held               # made once
    first = film.denoise(g, pta.DenoiseParams.default_var(), want_ferr=True)
    film.reset()
    assert film.info.device_bytes - parent == held and film.info.samples == 0
    film.add_pass(g, 4)
    again = film.denoise(g, pta.DenoiseParams.default_var(), want_ferr=True)
    assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(first, again))
    assert film.adaptive_info.device_bytes == film.info.device_bytes
    film.close()
    g.close()


def test_destroy_frees_the_scratch(pta):
    """Films of 1920x1080 that each make their scratch (149 MB and 66 MB of guides) and are destroyed: the device's free memory
    comes back.  24 leaked scratches would be 5.2 GB; the margin of 1 GiB is for whatever else runs on the device meanwhile."""
    import torch
    w, h, rounds = 1920, 1080, 24
    g = pta.GpuScene(host(pta, "cube"))
    params = pta.DenoiseParams.default_var()

    def one_film():
        film = pta.Film(pta.Profile.make(w, h, 1, BOUNCES))
        film.add_pass(g, 2)
        film.denoise(g, params, want_ferr=True)
        film.filtered_noise(g, params, 0.05)
        held = film.info.device_bytes - parent_device_bytes(w * h)
        film.close()
        return held
    held = one_film()                                            # (the process's first such film: code objects, the scene's queues)
    assert held == film_scratch_and_guides(pta, w, h) > 200 << 20
    torch.cuda.synchronize()
    free_before, _ = torch.cuda.mem_get_info()
    for _ in range(rounds):
        assert one_film() == held
    torch.cuda.synchronize()
    free_after, _ = torch.cuda.mem_get_info()
    assert rounds * held > 4 << 30
    assert free_before - free_after < 1 << 30, (free_before, free_after, held)
    g.close()


def film_scratch_and_guides(pta, w, h):
    film = pta.Film(pta.Profile.make(w, h, 1, BOUNCES))
    scratch = film.denoise_scratch_bytes()
    film.close()
    return scratch + 32 * w * h
