"""tests/denoise_var_model.py on the CPU: the variance-guided filter's defining properties and the gain
tools/measure_denoise_var_gain.py recorded (tests/golden/denoise_var_gain.json) for the library's default parameters."""
import json
import re

import numpy as np
import pytest

import denoise_model as dm
import denoise_var_model as dvm
from conftest import GOLDEN, ROOT, SCENES

f32 = np.float32
GAIN = json.loads((GOLDEN / "denoise_var_gain.json").read_text())
PLAIN = json.loads((GOLDEN / "denoise_gain.json").read_text())
SCORED = ("cube", "head", "reflection", "spheres", "white_furnace_direct")


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def mse(a, b):
    return float(np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2))


# ------------------------------------------------------------------------------------------------ properties of the model
@pytest.mark.parametrize("flags", [0, dvm.NO_DEMODULATE])
def test_zero_iterations_is_the_identity_and_invalid_pixels_pass_through(flags):
    w, h = 37, 23
    samples, accum, g = dm.synthetic_inputs(w, h, 1)
    mom = dvm.synthetic_moments(samples, accum, 2)
    c = accum / f32(samples)
    assert np.array_equal(bits(dvm.denoise_var(w, h, samples, accum, mom, g, 0, 4.0, 1.0, 5, flags)), bits(c))
    out = dvm.denoise_var(w, h, samples, accum, mom, g, 4, 4.0, 1.0, 5, flags)
    invalid = g[:, 3] < 0
    assert invalid.any() and np.array_equal(bits(out[invalid]), bits(c[invalid]))
    assert (out[~invalid] != c[~invalid]).any()
    # an invalid pixel is never a tap: neither its colour nor its moments reach anybody
    accum2, mom2 = accum.copy(), mom.copy()
    accum2[invalid] = accum2[invalid] * f32(7.0) + f32(1.0)
    mom2[invalid] = mom2[invalid] * f32(5.0) + f32(3.0)
    out2 = dvm.denoise_var(w, h, samples, accum2, mom2, g, 4, 4.0, 1.0, 5, flags)
    assert np.array_equal(bits(out2[~invalid]), bits(out[~invalid]))


def flat_guides(w, h):
    g = np.zeros((w * h, 8), f32)
    g[:, 2], g[:, 3], g[:, 4:7] = 1.0, 5.0, 0.5
    return g


def test_a_zero_variance_region_of_distinct_colours_is_unchanged_to_the_bit():
    """m2 = m1^2/N on every pixel: vb = 0, lden = 1e-6, and a luminance difference of 8e-6 or more cuts the tap (wexp = 0).
    What is left is acc = x*k, wsum = k for the centre weight k = 9/64.  The colours are multiples of 1/8 below 64: x*9 is
    exact in f32, so (x*k)/k gives x back without a rounding - for arbitrary mantissas that round trip may move the last bit,
    which is the arithmetic of the specification, not a leak between pixels."""
    w, h, samples = 17, 13, 4
    rng = np.random.default_rng(4)
    n = w * h
    g = flat_guides(w, h)
    mean = (rng.permutation(n)[:, None] % 251 + np.arange(3)[None, :] * 7 + 1).astype(f32) / f32(8.0)
    accum = mean * f32(samples)
    lum_c = dvm.lum(mean)
    gaps = np.abs(lum_c[:, None] - lum_c[None, :])[~np.eye(n, dtype=bool)]
    assert gaps.min() >= 8e-6          # distinct colours: every tap is cut
    m1 = dvm.lum(accum)
    mom = np.stack([m1, (m1 * m1) / f32(samples)], axis=1).astype(f32)
    assert (dvm.variance_of_mean(samples, mom) == 0).all()
    for it in (1, 3):
        out = dvm.denoise_var(w, h, samples, accum, mom, g, it, 4.0, 1.0, 3, dvm.NO_DEMODULATE)
        assert np.array_equal(bits(out), bits(mean)), it
    # with a variance the same pixels do mix
    mom_noisy = mom.copy()
    mom_noisy[:, 1] *= f32(2.0)
    out = dvm.denoise_var(w, h, samples, accum, mom_noisy, g, 1, 4.0, 1.0, 3, dvm.NO_DEMODULATE)
    assert (out != mean).any()


def test_the_clamp_of_a_negative_variance_is_taken():
    """m2 below m1^2/N (what rounding of the two sums can produce): s2 is clamped to 0, the pixel behaves as one of zero
    variance - not as one of NaN or negative variance."""
    w, h = 29, 17
    samples, accum, g = dm.synthetic_inputs(w, h, 5)
    mom = dvm.synthetic_moments(samples, accum, 6)
    N = f32(samples)
    raw = mom[:, 1] / N - (mom[:, 0] / N) * (mom[:, 0] / N)
    low = raw < 0
    assert low.sum() > 20 and (dvm.variance_of_mean(samples, mom)[low] == 0).all()
    assert (dvm.variance_of_mean(samples, mom) >= 0).all()
    clamped = mom.copy()
    clamped[low, 1] = (mom[low, 0] * mom[low, 0]) / N     # exactly zero variance (N is a power of two)
    for flags in (0, dvm.NO_DEMODULATE):
        a = dvm.denoise_var(w, h, samples, accum, mom, g, 3, 4.0, 1.0, 3, flags)
        b = dvm.denoise_var(w, h, samples, accum, clamped, g, 3, 4.0, 1.0, 3, flags)
        assert np.isfinite(a).all() and np.array_equal(bits(a), bits(b))


def test_moments_of_restates_sum_and_sum_of_squares():
    rng = np.random.default_rng(8)
    planes = rng.random((5, 40, 3)).astype(f32) * f32(3.0)
    acc, mom = dvm.moments_of(planes)
    L = dvm.lum(planes).astype(np.float64)
    assert np.allclose(acc, planes.astype(np.float64).sum(axis=0), rtol=1e-6)
    assert np.allclose(mom[:, 0], L.sum(axis=0), rtol=1e-6) and np.allclose(mom[:, 1], (L * L).sum(axis=0), rtol=1e-6)
    v = dvm.variance_of_mean(5, mom)
    assert np.allclose(v, L.var(axis=0, ddof=0) / 4.0, rtol=1e-3, atol=1e-6)


# ------------------------------------------------------------------------------------------------ the recorded gain
def test_header_defaults_are_the_recorded_winner(pta):
    text = (ROOT / "include" / "ptgpu.h").read_text()
    got = dict(re.findall(r"#define PT_DENOISE_VAR_DEFAULT_(\w+)\s+(\S+)", text))
    win = GAIN["defaults"]
    assert set(got) == {"ITERATIONS", "FLAGS", "NORMAL_POWER_LOG2", "SIGMA_COLOR", "SIGMA_DEPTH"}
    assert int(got["ITERATIONS"]) == win["iterations"] and int(got["NORMAL_POWER_LOG2"]) == win["normal_power_log2"]
    assert float(got["SIGMA_COLOR"].rstrip("f")) == win["sigma_color"] and float(got["SIGMA_DEPTH"].rstrip("f")) == win["sigma_depth"]
    assert {"0": 0, "PT_DENOISE_NO_DEMODULATE": dvm.NO_DEMODULATE}[got["FLAGS"]] == win["flags"]
    for key in ("sigma_color", "sigma_depth", "normal_power_log2", "iterations", "flags"):
        assert win[key] in GAIN["grid"][key]
    p = pta.DenoiseParams.default_var()
    assert (p.iterations, p.flags, p.normal_power_log2, p.sigma_color, p.sigma_depth, p.tonemap) == \
        (win["iterations"], win["flags"], win["normal_power_log2"], win["sigma_color"], win["sigma_depth"], pta.TONEMAPS["FILMIC"])


@pytest.fixture(scope="module")
def measured(pta, oracle):
    """name -> (mse raw, mse pt_denoise defaults, mse variance-guided winner), recomputed here for every recorded scene."""
    assert (GAIN["width"], GAIN["height"], GAIN["spp"], GAIN["bounces"]) == (PLAIN["width"], PLAIN["height"], PLAIN["spp"], PLAIN["bounces"])
    w, h, spp = GAIN["width"], GAIN["height"], GAIN["spp"]
    win, pd = GAIN["defaults"], PLAIN["defaults"]
    out = {}
    for name in list(GAIN["scenes"]) + list(GAIN["reported"]):
        accum, mom, guides = dvm.inputs_from_oracle(pta, oracle, SCENES / name / "scene.isf", w, h, spp, GAIN["bounces"])
        ref_path = GOLDEN / "denoise_ref" / f"{name}.npy"
        if not ref_path.exists():
            continue    # (a reported scene the winner does not improve has no reference and no assertion)
        ref = np.load(ref_path)
        var = dvm.denoise_var(w, h, spp, accum, mom, guides, win["iterations"], win["sigma_color"], win["sigma_depth"],
                              win["normal_power_log2"], win["flags"])
        plain = dm.denoise(w, h, spp, accum, guides, pd["iterations"], pd["sigma_color"], pd["sigma_depth"], pd["normal_power_log2"])
        out[name] = (mse(accum / f32(spp), ref), mse(plain, ref), mse(var, ref))
        print(name, "mse raw %.6g plain %.6g variance-guided %.6g" % out[name])
    return out


def test_the_five_scenes_are_the_recorded_ones():
    assert tuple(sorted(GAIN["scenes"])) == SCORED


@pytest.mark.parametrize("name", SCORED)
def test_the_winner_lowers_the_error_of_a_4spp_frame(measured, name):
    raw, _, var = measured[name]
    assert var < raw
    assert var == pytest.approx(GAIN["scenes"][name]["mse_variance_guided"], rel=1e-6)
    assert raw == pytest.approx(GAIN["scenes"][name]["mse_raw"], rel=1e-6)


def test_the_winner_beats_the_plain_filters_defaults(measured):
    score = float(np.mean([np.log(measured[n][2] / measured[n][0]) for n in SCORED]))
    plain = float(np.mean([np.log(measured[n][1] / measured[n][0]) for n in SCORED]))
    print("mean log ratio: variance-guided", score, "plain", plain)
    assert score < plain
    assert score == pytest.approx(GAIN["score_mean_log_ratio"], abs=1e-6)
    assert plain == pytest.approx(GAIN["plain_score_mean_log_ratio"], abs=1e-6)


@pytest.mark.parametrize("name", sorted(n for n, row in GAIN["reported"].items() if row["improved"]))
def test_other_scenes_recorded_as_improved_improve(measured, name):
    raw, _, var = measured[name]
    assert var < raw
