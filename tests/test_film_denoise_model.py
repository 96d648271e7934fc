"""tests/film_denoise_model.py on the CPU: with one count for every pixel it is denoise_model / denoise_var_model bit for bit,
its error figure is finite at two samples and falls back to film_model's err where nothing is filtered, and its tile
reduction is film_adaptive_model's."""
import numpy as np
import pytest

import denoise_model as dm
import denoise_var_model as dvm
import film_adaptive_model as am
import film_denoise_model as fdm
import film_model as fm

f32 = np.float32
SHAPES = ((72, 40, 16, 16), (70, 50, 32, 8), (5, 4, 16, 16))


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def same_bits(a, b):
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    return a.shape == b.shape and bool(((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))).all())


def inputs(w, h, seed):
    samples, accum, guides = dm.synthetic_inputs(w, h, seed)
    return samples, accum, dvm.synthetic_moments(samples, accum, seed + 1), guides


@pytest.mark.parametrize("w,h,tw,th", SHAPES)
def test_a_constant_count_gives_the_uniform_models_bits(w, h, tw, th):
    samples, accum, moments, guides = inputs(w, h, 40 + w)
    counts = np.full(w * h, samples, np.uint32)
    for k, (it, fl) in enumerate((it, fl) for it in (0, 1, 3) for fl in (0, fdm.NO_DEMODULATE)):
        sc, sd, npow = (4.0, 0.75, 16.0)[k % 3], (0.5, 2.0)[k % 2], (0, 3, 10)[(k // 2) % 3]
        for c in (counts, samples):     # an array, and the uniform film's one number
            col, ferr = fdm.film_denoise(w, h, c, accum, moments, guides, it, sc, sd, npow, fl, True)
            assert same_bits(col, dvm.denoise_var(w, h, samples, accum, moments, guides, it, sc, sd, npow, fl)), (it, fl)
            assert ferr.shape == (w * h,)
            col, ferr = fdm.film_denoise(w, h, c, accum, moments, guides, it, sc, sd, npow, fl, False)
            assert same_bits(col, dm.denoise(w, h, samples, accum, guides, it, sc, sd, npow, fl)), (it, fl)
            assert ferr is None
        col, _ = fdm.film_denoise(w, h, counts, accum, moments, guides, it, 0.0, sd, npow, fl, False)
        assert same_bits(col, dm.denoise(w, h, samples, accum, guides, it, 0.0, sd, npow, fl)), (it, fl)


def test_counts_change_the_result_pixel_by_pixel():
    w, h = 72, 40
    samples, accum, moments, guides = inputs(w, h, 7)
    counts = np.full(w * h, samples, np.uint32)
    counts[: w * h // 2] = 2 * samples
    col, ferr = fdm.film_denoise(w, h, counts, accum, moments, guides, 0, 4.0, 4.0, 3)
    assert same_bits(col, accum / counts.astype(f32)[:, None])
    assert same_bits(col[w * h // 2:], fm.resolve_color(accum[w * h // 2:], samples))
    col1, _ = fdm.film_denoise(w, h, counts, accum, moments, guides, 1, 4.0, 4.0, 3)
    ref, _ = fdm.film_denoise(w, h, samples, accum, moments, guides, 1, 4.0, 4.0, 3)
    far = np.zeros((h, w), bool)
    far[h // 2 + 2:] = True      # rows the 5x5 taps of step 1 cannot reach from the other half
    assert same_bits(col1.reshape(h, w, 3)[far], ref.reshape(h, w, 3)[far]) and not same_bits(col1, ref)


@pytest.mark.parametrize("flags", (0, fdm.NO_DEMODULATE))
def test_two_samples_give_a_finite_error(flags):
    w, h = 33, 9
    _, accum, _, guides = inputs(w, h, 11)
    accum = (accum / f32(2)).astype(f32)
    moments = dvm.synthetic_moments(2, accum, 12)
    for it in (0, 1, 3):
        col, ferr = fdm.film_denoise(w, h, np.full(w * h, 2, np.uint32), accum, moments, guides, it, 4.0, 4.0, 3, flags)
        assert np.isfinite(ferr).all() and (ferr >= 0).all() and ferr.max() > 0, it
        assert np.isfinite(col).all()


def test_unfiltered_pixels_carry_the_films_raw_error():
    w, h = 70, 50
    samples, accum, moments, guides = inputs(w, h, 21)
    counts = np.full(w * h, samples, np.uint32)
    counts[::3] = 3 * samples
    invalid = ~(guides[:, 3] >= 0)
    assert invalid.any() and (~invalid).any()
    for floor in (0.01, 0.5):
        _, ferr = fdm.film_denoise(w, h, counts, accum, moments, guides, 2, 4.0, 4.0, 3, 0, True, floor)
        for c in (samples, 3 * samples):
            sel = invalid & (counts == c)
            assert sel.any() and same_bits(ferr[sel], fm.pixel_error(moments, c, floor)[sel])
        assert not same_bits(ferr[~invalid], am.pixel_error(moments, counts, floor)[~invalid])
        _, ferr0 = fdm.film_denoise(w, h, counts, accum, moments, guides, 0, 4.0, 4.0, 3, 0, True, floor)
        assert same_bits(ferr0, am.pixel_error(moments, counts, floor))
    uniform = fdm.film_denoise(w, h, samples, accum, moments, guides, 0, 4.0, 4.0, 3)[1]
    assert same_bits(uniform, fm.pixel_error(moments, samples))


@pytest.mark.parametrize("w,h,tw,th", SHAPES)
def test_the_tile_reduction_over_an_error_plane_is_the_adaptive_films(w, h, tw, th):
    t = am.Tiling(w, h, tw, th)
    _, mom = fm.synthetic_planes(w * h, 6, w)
    counts = np.full(w * h, 6, np.uint32)
    want, err, tsum, tmax = am.tile_noise(t, mom, counts, 0.05)
    got_sum, got_max = fdm.tile_reduce(t, err)
    assert same_bits(got_sum, tsum) and same_bits(got_max, tmax)
    # filtered_noise with no pass filters nothing: the adaptive film's figures
    samples, accum, moments, guides = inputs(w, h, 3)

    class P:
        iterations, sigma_color, sigma_depth, normal_power_log2, flags = 0, 4.0, 4.0, 3, 0
    cnt = np.full(w * h, samples, np.uint32)
    st, ferr, fs, fx = fdm.filtered_noise(t, P, cnt, accum, moments, guides, 0.05)
    w_st, w_err, w_sum, w_max = am.tile_noise(t, moments, cnt, 0.05)
    assert st == w_st and same_bits(ferr, w_err) and same_bits(fs, w_sum) and same_bits(fx, w_max)


def test_the_filtered_loop_selects_by_the_filtered_sums():
    t = am.Tiling(72, 40, 16, 16)
    pixels = np.array([t.rect(k)[2] * t.rect(k)[3] for k in range(15)], f32)
    means = np.full(15, 0.05, f32)
    means[[0, 7, 14]] = f32(0.01)        # three tiles are below the target after the first pass, every tile after the second
    sums = [means * pixels, f32(0.01) * pixels]
    asked = []

    def after(k, samples, tiles):
        asked.append((samples, list(tiles)))
        return sums[k]
    made, why = fdm.render_until_filtered(t, after, 8, 8, 0, 0.02, 512)
    assert why == "converged" and [m[0] for m in made] == [8, 16] and made[0][1] == list(range(15))
    assert made[1][1] == am.candidates(t, sums[0], 0.02) and 0 < len(made[1][1]) < 15 and asked == made
