"""tests/film_model.py on hand-made planes (no GPU): the definition of pt_film_noise case by case, the block tree, the
statistics, and the schedule of pt_film_render_until."""
import re

import numpy as np

import film_model as fm
from conftest import ROOT

f32 = np.float32


def moments_of(samples):
    """(m1, m2) built in sample order as pt_render_moments builds them."""
    m1 = m2 = f32(0)
    for L in samples:
        L = f32(L)
        m1 = f32(m1 + L)
        m2 = f32(m2 + f32(L * L))
    return [m1, m2]


def test_zero_variance_gives_zero_error():
    for n in (2, 3, 14, 1 << 24):
        mom = np.array([[0.5 * n, 0.25 * n], [2.0 * n, 4.0 * n], [0.0, 0.0]], f32)
        err = fm.pixel_error(mom, n)
        assert err.dtype == f32 and (err == 0).all(), n
    assert fm.pixel_error([moments_of([0.75] * 8)], 8)[0] == 0


def test_error_is_the_relative_standard_error_of_the_mean():
    s = [0.5, 1.5, 1.0, 3.0]
    err = fm.pixel_error([moments_of(s)], 4)[0]
    pop = np.var(s)                                   # e2 - mu^2
    want = np.sqrt(pop / 3) / np.mean(s)              # s2 / (n - 1), relative to the mean
    assert abs(float(err) - want) <= 4 * np.finfo(f32).eps * want
    # every step is a float32 operation in the header's order
    m1, m2 = moments_of(s)
    N = f32(4)
    mu, e2 = f32(m1 / N), f32(m2 / N)
    s2 = max(f32(0), f32(e2 - f32(mu * mu)))
    step = f32(np.sqrt(f32(s2 / f32(3)))) / max(mu, f32(0.01))
    assert err.view(np.uint32) == f32(step).view(np.uint32)


def test_a_mean_below_the_floor_uses_the_floor():
    n = 4
    mom = np.array([moments_of([0.0, 0.0, 0.0, 0.004])], f32)     # mu = 0.001
    at_floor = fm.pixel_error(mom, n, lum_floor=0.01)[0]
    own_mean = fm.pixel_error(mom, n, lum_floor=1e-6)[0]
    mu = f32(mom[0, 0] / f32(n))
    assert mu < f32(0.01) and at_floor < own_mean
    se = f32(np.sqrt(f32(max(f32(0), f32(f32(mom[0, 1] / f32(n)) - f32(mu * mu))) / f32(n - 1))))
    assert at_floor.view(np.uint32) == f32(se / f32(0.01)).view(np.uint32)
    assert own_mean.view(np.uint32) == f32(se / mu).view(np.uint32)
    black = fm.pixel_error([[0.0, 0.0]], n)[0]
    assert black == 0 and np.isfinite(black)


def test_a_negative_variance_clamps_to_zero():
    mom = np.array([[2.0 * 8, 3.0 * 8]], f32)   # e2 = 3 < mu*mu = 4
    assert fm.pixel_error(mom, 8)[0] == 0
    assert np.signbit(fm.pixel_error(mom, 8)[0]) == False   # noqa: E712  (+0: max(0, negative))


def test_257_pixels_are_two_blocks_the_second_with_one_pixel():
    err = np.arange(1, 258, dtype=f32) / f32(64)
    bsum, bmax = fm.blocks(err)
    assert bsum.shape == bmax.shape == (2,)
    assert bsum[1] == err[256] and bmax[1] == err[256] and bmax[0] == err[255]
    assert bsum[0] == f32(np.arange(1, 257).sum() / 64)   # (exact: small multiples of 2^-6)
    st = fm.statistics(bsum, 257, target=float(err[256]) - 1e-3, samples=8)
    assert st["n_blocks"] == 2 and st["fraction_over"] == 0.5   # block 1's mean (4.016) is over, block 0's (2.008) is not
    assert st["max_block_error"] == float(err[256])
    assert st["mean_error"] == (float(bsum[0]) + float(bsum[1])) / 257
    assert st["converged"] == 1   # the MEAN error (2.016) decides, not the worst block
    low = fm.statistics(bsum, 257, 1.0, 8)
    assert low["converged"] == 0 and low["fraction_over"] == 1.0


def test_the_block_sum_is_the_fixed_tree_not_a_running_sum():
    rng = np.random.default_rng(7)
    err = rng.uniform(0, 1, 300).astype(f32)
    bsum, bmax = fm.blocks(err)
    v = np.zeros(512, f32)
    v[:300] = err
    for b in range(2):
        w = [f32(x) for x in v[256 * b:256 * b + 256]]
        for stride in (128, 64, 32, 16, 8, 4, 2, 1):
            for i in range(stride):
                w[i] = f32(w[i] + w[i + stride])
        assert w[0].view(np.uint32) == bsum[b].view(np.uint32)
        assert bmax[b] == err[256 * b:256 * b + 256].max()
    # over random data a running f32 sum differs from the tree somewhere: the order is part of the definition
    differs = False
    for seed in range(8):
        e = np.random.default_rng(seed).uniform(0, 1, 256).astype(f32)
        run = f32(0)
        for x in e:
            run = f32(run + x)
        differs |= run.view(np.uint32) != fm.blocks(e)[0][0].view(np.uint32)
    assert differs


def test_noise_puts_the_pieces_together():
    accum, mom = fm.synthetic_planes(8710, 14, 3)
    st, err, bsum, bmax = fm.noise(mom, 14, 0.1)
    assert len(err) == 8710 and st["n_blocks"] == 35 == len(bsum) == len(bmax) and st["samples"] == 14
    assert err[0] == 0 and err[2] == 0 and err[3] == 0 and err[1] > 0 and np.isfinite(err).all() and (err >= 0).all()
    assert abs(st["mean_error"] - float(err.astype(np.float64).mean())) <= 1e-5 * st["mean_error"]
    assert st["max_block_error"] >= st["mean_error"] and 0.0 <= st["fraction_over"] <= 1.0


def test_merge_and_resolve():
    a = np.array([[1.0, 2.0, 3.0], [1e8, 1.0, 0.0]], f32)
    b = np.array([[0.5, 0.25, 1e-9], [1.0, 1e-8, 0.0]], f32)
    m = fm.merge(fm.merge(np.zeros_like(a), a), b)
    assert m.dtype == f32 and (m == (a + b)).all() and m[1, 0] == f32(1e8)   # (1e8 + 1 rounds back in float32)
    assert (fm.merge(np.zeros_like(a), a).view(np.uint32) == a.view(np.uint32)).all()
    assert (fm.resolve_color(a, 3) == a / f32(3)).all() and fm.resolve_color(a, 3).dtype == f32


def test_schedule():
    assert fm.schedule(8, 64) == [8, 16, 32]
    assert fm.schedule(2, 2) == [2]
    assert fm.schedule(4, 60) == [4, 8, 16, 32]
    assert fm.schedule(8, 7) == []
    assert fm.schedule(8, 512) == [8, 16, 32, 64, 128, 256]       # 504 in all
    assert fm.schedule(2, 1 << 30)[-1] == 1 << 23 and sum(fm.schedule(2, 1 << 30)) == fm.MAX_SAMPLES - 2   # the 2^24 cap
    assert fm.schedule(8, 64, last=8, total=8) == [16, 32]        # a film that already has a pass goes on doubling
    for first, cap in ((2, 2), (3, 100), (8, 64), (5, 1000)):
        s = fm.schedule(first, cap)
        assert all(b >= 2 * a for a, b in zip(s, s[1:])) and sum(s) <= cap


def test_render_until_stops_at_the_target_or_at_the_budget():
    errors = [0.4, 0.2, 0.09, 0.05]
    made, conv = fm.render_until(lambda k, total: errors[k], 4, 60, 0.1)
    assert (made, conv) == ([4, 8, 16], True)
    made, conv = fm.render_until(lambda k, total: errors[k], 4, 60, 0.0)
    assert (made, conv) == ([4, 8, 16, 32], False)
    made, conv = fm.render_until(lambda k, total: errors[k], 4, 60, 1e9)
    assert (made, conv) == ([4], True)


def test_the_header_states_what_the_model_restates():
    text = (ROOT / "include" / "ptgpu.h").read_text()
    assert "progressive film (DESIGN 4h; no reference counterpart)" in text
    assert re.search(r"PT_FILM_MAX_SAMPLES\s*=\s*1u\s*<<\s*24", text) and fm.MAX_SAMPLES == 1 << 24
    assert re.search(r"#define\s+PT_FILM_DEFAULT_LUM_FLOOR\s+0\.01f", text) and fm.DEFAULT_LUM_FLOOR == 0.01
    for step in ("mu = m1 / N", "e2 = m2 / N", "s2 = max(0, e2 - mu*mu)", "vL = s2 / (float)(n - 1)", "se = sqrt(vL)",
                 "den = max(mu, lum_floor)", "err = se / den", "stride = 128, 64, 32, 16, 8, 4, 2, 1"):
        assert step in text, step


def test_cli_refuses_bad_film_arguments_before_any_gpu_work(tmp_path):
    """`render --noise-target`: every refused combination exits with 2 and writes nothing (no GPU is touched: this runs
    without one)."""
    import subprocess
    exe = ROOT / "path-tracer_amd" / "path-tracer"
    scene = ROOT / "tests" / "golden" / "scenes" / "cube" / "scene.isf"
    prof = tmp_path / "p.yml"
    prof.write_text("resolution:\n  width: 32\n  height: 24\nsamples: 16\nbounces: 2\n")
    frames = tmp_path / "frames.json"
    frames.write_text("[{}, {}]")
    cases = {"target 0": ["--noise-target", "0"], "target negative": ["--noise-target=-0.5"], "target nan": ["--noise-target", "nan"],
             "target inf": ["--noise-target", "inf"], "target text": ["--noise-target", "fine"],
             "n0 below 2": ["--noise-target", "0.1", "--min-samples", "1"],
             "n0 above the profile's samples": ["--noise-target", "0.1", "--min-samples", "32"],
             "n0 above N": ["--noise-target", "0.1", "--max-samples", "4"],
             "several devices": ["--noise-target", "0.1", "--devices", "0,0"],
             "light mixer": ["--noise-target", "0.1", "--keyframes", str(frames), "--light-mixer"],
             "min-samples alone": ["--min-samples", "4"], "max-samples alone": ["--max-samples", "64"],
             "noise-map alone": ["--noise-map", str(tmp_path / "n.png")],
             "noise map that is no png": ["--noise-target", "0.1", "--noise-map", str(tmp_path / "n.jpg")]}
    for label, args in cases.items():
        out = tmp_path / label.replace(" ", "_").replace("'", "")
        out.mkdir()
        r = subprocess.run([str(exe), "render", str(scene), "-q", "-p", str(prof), *args, "-o", str(out / "f_%d.png")],
                           capture_output=True, text=True, timeout=60)
        assert r.returncode == 2, (label, r.stderr)
        assert r.stderr.strip() and not list(out.iterdir()), label
    assert not (tmp_path / "n.png").exists() and not (tmp_path / "n.jpg").exists()
    r = subprocess.run([str(exe), "render", "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and all(o in r.stdout for o in ("--noise-target", "--min-samples", "--max-samples", "--noise-map"))
