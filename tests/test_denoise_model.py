"""tests/denoise_model.py on the CPU: its camera ray against the oracle's, the filter's defining properties, and the gain
tools/measure_denoise_gain.py recorded (tests/golden/denoise_gain.json) for the library's default parameters."""
import json
import re

import numpy as np
import pytest

import denoise_model as dm
from conftest import GOLDEN, ROOT

f32 = np.float32
GAIN = json.loads((GOLDEN / "denoise_gain.json").read_text())


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


# ------------------------------------------------------------------------------------------------ the camera ray
@pytest.mark.parametrize("name,width,height,samples", [("cube", 64, 48, 4), ("spheres", 33, 17, 7), ("head", 130, 67, 1)])
def test_ray_restatement_equals_the_oracles_primary_ray(pta, oracle, scene_cache, name, width, height, samples):
    hs = scene_cache(name)
    osc = oracle.OracleScene(hs.desc, oracle.PTO_BRUTE_FORCE)
    prof = pta.Profile.make(width, height, samples, 1)
    rng = np.random.default_rng(5)
    pix = np.concatenate([[0, width - 1, width * height - 1], rng.integers(0, width * height, 150)])
    smp = rng.integers(1, samples + 1, len(pix))
    words = oracle.rng_words(smp.astype(np.uint64) + pix.astype(np.uint64) * np.uint64(samples), 2)
    r = (words >> 8).astype(f32) * f32(1.0 / 16777216.0)
    got = dm.primary_rays(hs.camera, width, height, r[:, 0], r[:, 1], pixels=pix)
    want = np.stack([osc.primary_ray(prof, int(p), int(s)) for p, s in zip(pix, smp)])
    assert np.array_equal(bits(got), bits(want))


# ------------------------------------------------------------------------------------------------ properties of the model
@pytest.mark.parametrize("flags", [0, dm.NO_DEMODULATE])
def test_invalid_pixels_pass_through_and_zero_iterations_is_the_identity(flags):
    w, h = 37, 23
    samples, accum, g = dm.synthetic_inputs(w, h, 1)
    c = accum / f32(samples)
    out0 = dm.denoise(w, h, samples, accum, g, 0, 1.0, 1.0, 5, flags)
    assert np.array_equal(bits(out0), bits(c))
    out = dm.denoise(w, h, samples, accum, g, 4, 1.0, 1.0, 5, flags)
    invalid = g[:, 3] < 0
    assert invalid.any() and np.array_equal(bits(out[invalid]), bits(c[invalid]))
    assert (out[~invalid] != c[~invalid]).any()
    # an invalid pixel is never a tap: its colour does not reach anybody
    accum2 = accum.copy()
    accum2[invalid] = accum2[invalid] * f32(7.0) + f32(1.0)
    out2 = dm.denoise(w, h, samples, accum2, g, 4, 1.0, 1.0, 5, flags)
    assert np.array_equal(bits(out2[~invalid]), bits(out[~invalid]))


@pytest.mark.parametrize("sigma_color", [0.0, 1.0])
def test_perpendicular_regions_do_not_mix(sigma_color):
    w, h = 40, 24
    rng = np.random.default_rng(3)
    n = w * h
    left = (np.arange(n) % w) < 17
    g = np.zeros((n, 8), f32)
    g[:, 0:3] = np.where(left[:, None], f32([0, 0, 1]), f32([3, 0, 0]))   # perpendicular, one not unit length
    g[:, 3] = 10.0
    g[:, 4:7] = 0.5
    accum = rng.random((n, 3)).astype(f32) * f32(8.0)
    out = dm.denoise(w, h, 4, accum, g, 5, sigma_color, 1.0, 0)   # (power 0: the weight is max(0, cos) itself)
    accum2 = accum.copy()
    accum2[left] = rng.random((int(left.sum()), 3)).astype(f32) * f32(100.0)
    out2 = dm.denoise(w, h, 4, accum2, g, 5, sigma_color, 1.0, 0)
    assert np.array_equal(bits(out2[~left]), bits(out[~left]))
    assert (out2[left] != out[left]).any()


def test_one_pass_is_the_b3_spline_where_every_weight_is_one():
    """A flat, fronto-parallel, constant-normal image with the colour weight off: every tap weight is k, so one pass is the
    5x5 B3-spline blur renormalised at the border (float64 check of the model's f32 result)."""
    w, h = 19, 11
    rng = np.random.default_rng(9)
    g = np.zeros((w * h, 8), f32)
    g[:, 2], g[:, 3] = 1.0, 5.0
    accum = rng.random((w * h, 3)).astype(f32)
    out = dm.denoise(w, h, 1, accum, g, 1, 0.0, 1.0, 3, dm.NO_DEMODULATE).reshape(h, w, 3)
    k1 = np.array([0.0625, 0.25, 0.375, 0.25, 0.0625])
    img = accum.reshape(h, w, 3).astype(np.float64)
    num, den = np.zeros_like(img), np.zeros((h, w, 1))
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            ys, xs = slice(max(0, -dy), min(h, h - dy)), slice(max(0, -dx), min(w, w - dx))
            yq, xq = slice(max(0, dy), min(h, h + dy)), slice(max(0, dx), min(w, w + dx))
            num[ys, xs] += k1[dy + 2] * k1[dx + 2] * img[yq, xq]
            den[ys, xs] += k1[dy + 2] * k1[dx + 2]
    assert np.allclose(out, num / den, rtol=1e-5, atol=1e-6)


# ------------------------------------------------------------------------------------------------ the recorded gain
def test_header_defaults_are_the_recorded_winner():
    text = (ROOT / "include" / "ptgpu.h").read_text()
    got = {k.lower(): float(v.rstrip("f")) for k, v in re.findall(r"#define PT_DENOISE_DEFAULT_(\w+)\s+([0-9.]+f?)", text)}
    assert got == {k: float(v) for k, v in GAIN["defaults"].items()}


@pytest.mark.parametrize("name", sorted(GAIN["scenes"]))
def test_default_parameters_lower_the_error_of_a_4spp_frame(pta, oracle, scene_cache, name):
    w, h, spp = GAIN["width"], GAIN["height"], GAIN["spp"]
    hs = scene_cache(name)
    osc = oracle.OracleScene(hs.desc, oracle.PTO_BVH)
    _, accum, _ = osc.render(pta.Profile.make(w, h, spp, GAIN["bounces"]))
    ref = np.load(GOLDEN / "denoise_ref" / f"{name}.npy").astype(np.float64)
    guides = dm.guides_from_oracle(osc, hs.camera, w, h)
    d = GAIN["defaults"]
    out = dm.denoise(w, h, spp, accum, guides, d["iterations"], d["sigma_color"], d["sigma_depth"], d["normal_power_log2"])
    before = float(np.mean(((accum / f32(spp)).astype(np.float64) - ref) ** 2))
    after = float(np.mean((out.astype(np.float64) - ref) ** 2))
    print(name, "mse before", before, "after", after)
    assert after < before
