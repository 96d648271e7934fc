"""`render --noise-target --window-samples`: the combinations the command line refuses (no GPU: they exit before any device
work), a run to the budget whose PNG is plain `render` with the enumeration's samples byte for byte, and the adaptive form with
its maps against the film pt_film_render_until_windowed makes through Python."""
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, SCENES

EXE = ROOT / "path-tracer_amd" / "path-tracer"
W, H, BOUNCES, N = 33, 17, 3, 12
SCENE = SCENES / "cube" / "scene.isf"
SUMMARY = re.compile(r"^film: (\d+) passes, (\d+) samples, noise (\S+), (converged|max samples), pixel-samples (\d+) of (\d+)$", re.M)


def run(*args):
    return subprocess.run([str(EXE), "render", str(SCENE), *[str(a) for a in args]], capture_output=True, text=True, timeout=300)


def write_profile(path, samples):
    path.write_text(f"resolution:\n  width: {W}\n  height: {H}\nsamples: {samples}\nbounces: {BOUNCES}\n")
    return path


@pytest.fixture(scope="module")
def profiles(tmp_path_factory):
    d = tmp_path_factory.mktemp("film_window_cli")
    return {n: write_profile(d / f"p{n}.yml", n) for n in (12, 40, 1)}


def test_cli_refuses_before_any_gpu_work(tmp_path, profiles):
    out = tmp_path / "never.png"
    base = ("-q", "-p", profiles[12], "-o", out)
    cases = [
        (("--window-samples", 5), "'--window-samples <W>' needs '--noise-target <T>'"),
        (("--noise-target", 0.05, "--window-samples", 5, "--adaptive", "--film-denoise", "variance", "--filtered-target"),
         "'--window-samples <W>' cannot be used with '--filtered-target'"),
        (("--noise-target", 0.05, "--window-samples", 5, "--min-samples", 4), "cannot be used with '--min-samples <N0>'"),
        (("--noise-target", 0.05, "--window-samples", 1), "invalid value '1' for '--window-samples <W>'"),
        (("--noise-target", 0.05, "--window-samples", 0), "invalid value '0' for '--window-samples <W>'"),
        (("--noise-target", 0.05, "--window-samples", "x"), "a whole number expected"),
        (("--noise-target", 0.05, "--window-samples"), "a value is required"),
        (("--noise-target", -1, "--window-samples", 5), "invalid value '-1' for '--noise-target <T>'"),
        (("--noise-target", 0.05, "--window-samples", 5, "--max-samples", 1), "an enumeration of at least 2 samples"),
        (("--noise-target", 0.05, "--window-samples", 5, "--max-samples", (1 << 24) + 1), "for '--max-samples <N>': at most"),
        (("--noise-target", 0.05, "--window-samples", 5, "--devices", "0,1"), "more than one device"),
        (("--noise-target", 0.05, "--window-samples", 5, "--adaptive", "--denoise"), "cannot be used with '--denoise'"),
        (("--noise-target", 0.05, "--window-samples", 5, "--sample-map", tmp_path / "s.png"), "need '--noise-target <T> --adaptive'"),
        # a target of zero is a windowed film's alone
        (("--noise-target", 0), "invalid value '0' for '--noise-target <T>': a positive, finite number expected"),
        (("--noise-target", 0, "--adaptive"), "invalid value '0' for '--noise-target <T>'"),
    ]
    for args, message in cases:
        r = run(*base, *args)
        assert r.returncode == 2 and message in r.stderr, (args, r.returncode, r.stderr)
        assert not out.exists() and not (tmp_path / "s.png").exists()
    r = run("-q", "-p", profiles[1], "-o", out, "--noise-target", 0.05, "--window-samples", 5)   # the profile's samples are N
    assert r.returncode == 2 and "an enumeration of at least 2 samples" in r.stderr and not out.exists()


@pytest.mark.gpu
def test_a_run_to_the_budget_is_plain_render_byte_for_byte(tmp_path, profiles):
    plain, film, film2 = tmp_path / "plain.png", tmp_path / "film.png", tmp_path / "film2.png"
    r = run("-q", "-p", profiles[12], "-o", plain)
    assert r.returncode == 0, r.stderr
    # --max-samples is the enumeration (the profile says 40) ...
    r = run("-q", "-p", profiles[40], "--noise-target", 0, "--window-samples", 5, "--max-samples", N, "-o", film)
    assert r.returncode == 0, r.stderr
    assert film.read_bytes() == plain.read_bytes()
    m = SUMMARY.search(r.stderr)
    assert m and (int(m.group(1)), int(m.group(2)), m.group(4)) == (3, N, "max samples"), r.stderr      # windows of 5, 5, 2
    assert int(m.group(5)) == int(m.group(6)) == W * H * N
    # ... and defaults to the profile's samples
    r = run("-q", "-p", profiles[12], "--noise-target", 0, "--window-samples", 7, "-o", film2)
    assert r.returncode == 0, r.stderr
    assert film2.read_bytes() == plain.read_bytes()


@pytest.mark.gpu
def test_the_adaptive_form_writes_the_film_and_its_maps(pta, tmp_path, profiles):
    from PIL import Image
    target = 0.03
    g = pta.GpuScene(pta.HostScene.load_isf(SCENE))
    film = pta.Film.windowed(pta.Profile.make(W, H, N, BOUNCES), pta.Opts.make(tile_w=16, tile_h=16))
    passes = []
    stats = film.render_until_windowed(g, pta.FilmWindowParams.default(target=target, window_samples=5, adaptive=1, uniform_samples=4,
                                                                       dilate=0),
                                       lambda info, noise: passes.append((info.passes, info.last_pass_samples,
                                                                          film.adaptive_info.last_pass_tiles, noise.mean_error)))
    want, info, counts = film.resolve(), film.info, film.read_counts()
    err = film.tile_noise(target, want_planes=True)[1]
    film.close()
    g.close()
    out, smap, nmap = tmp_path / "o.png", tmp_path / "s.png", tmp_path / "n.png"
    r = run("-v", "-q", "-p", profiles[12], "--noise-target", target, "--window-samples", 5, "--adaptive", "--adaptive-tile", 16,
            "--uniform-samples", 4, "--adaptive-dilate", 0, "--sample-map", smap, "--noise-map", nmap, "-o", out)
    assert r.returncode == 0, r.stderr
    assert np.array_equal(np.asarray(Image.open(out)).reshape(-1, 3), want)
    m = SUMMARY.search(r.stderr)
    assert m, r.stderr
    assert (int(m.group(1)), int(m.group(2))) == (info.passes, info.samples), r.stderr
    assert m.group(3) == f"{stats.mean_error:.6g}" and m.group(4) == ("converged" if stats.converged else "max samples")
    assert (int(m.group(5)), int(m.group(6))) == (int(counts.sum()), W * H * info.samples)
    lines = re.findall(r"^film: pass (\d+): (\d+) samples, (\d+) of 6 tiles, noise (\S+)$", r.stderr, re.M)
    assert lines == [(str(p), str(s), str(t), f"{e:.6g}") for p, s, t, e in passes], r.stderr
    grey = np.asarray(Image.open(smap)).reshape(H * W, -1)
    v = counts.astype(np.float32) / np.float32(info.samples) * np.float32(255)
    assert (grey == v.astype(np.uint8)[:, None]).all()
    grey = np.asarray(Image.open(nmap)).reshape(H * W, -1)
    v = np.minimum(np.float32(1), err / (np.float32(2) * np.float32(target))) * np.float32(255)
    assert (grey == v.astype(np.uint8)[:, None]).all()
