"""`render --noise-target` on the GPU: the PNG is the film pt_film_render_until makes through Python, the summary line, the
noise map, the film reset between the frames of a camera path, the filtered forms, and the refused combinations."""
import json
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, SCENES

pytestmark = pytest.mark.gpu

EXE = ROOT / "path-tracer_amd" / "path-tracer"
W, H, BOUNCES = 64, 48, 2
SCENE = SCENES / "cube" / "scene.isf"
SUMMARY = re.compile(r"^film: (\d+) passes, (\d+) samples, noise (\S+), (converged|max samples)$", re.M)


def run(*args):
    return subprocess.run([str(EXE), "render", str(SCENE), *[str(a) for a in args]], capture_output=True, text=True, timeout=300)


@pytest.fixture(scope="module")
def profile_file(tmp_path_factory):
    p = tmp_path_factory.mktemp("film_cli") / "p.yml"
    p.write_text(f"resolution:\n  width: {W}\n  height: {H}\nsamples: 16\nbounces: {BOUNCES}\n")
    return p


def python_film(pta, host, first, max_samples, target, camera=None):
    g = pta.GpuScene(host)
    if camera is not None:
        g.set_camera(camera)
    film = pta.Film(pta.Profile.make(W, H, 16, BOUNCES))
    noise = film.render_until(g, first, max_samples, target)
    out = film.resolve(), film.info, noise, film.noise(target, want_planes=True)[1]
    film.close()
    g.close()
    return out


def test_cli_writes_the_film_render_until_makes(pta, tmp_path, profile_file):
    from PIL import Image
    host = pta.HostScene.load_isf(SCENE)
    for target in (0.05, 1e-6, 100.0):     # somewhere in the schedule, the whole budget, the first pass
        want, info, noise, err = python_film(pta, host, 4, 60, target)
        out, nmap = tmp_path / f"o_{target}.png", tmp_path / f"n_{target}.png"
        r = run("-q", "-p", profile_file, "--noise-target", target, "--min-samples", 4, "--max-samples", 60, "--noise-map", nmap, "-o", out)
        assert r.returncode == 0, r.stderr
        assert np.array_equal(np.asarray(Image.open(out)).reshape(-1, 3), want), target
        m = SUMMARY.search(r.stderr)
        assert m, r.stderr
        assert (int(m.group(1)), int(m.group(2))) == (info.passes, info.samples), r.stderr
        assert m.group(3) == f"{noise.mean_error:.6g}" and m.group(4) == ("converged" if noise.converged else "max samples")
        assert "film: pass " not in r.stderr     # (per-pass lines: with -v only)
        grey = np.asarray(Image.open(nmap))
        assert grey.shape[:2] == (H, W)
        grey = grey.reshape(H * W, -1)
        v = np.minimum(np.float32(1), err / (np.float32(2) * np.float32(target))) * np.float32(255)
        assert (grey == v.astype(np.uint8)[:, None]).all(), target
    assert info.passes == 1 and info.samples == 4 and noise.converged   # (the last case)
    # defaults: n0 = 8, N = the profile's samples (16): one pass of 8, the next would make 24
    out = tmp_path / "defaults.png"
    r = run("-q", "-p", profile_file, "--noise-target", 1e-6, "-o", out)
    assert r.returncode == 0 and SUMMARY.search(r.stderr).groups()[:2] == ("1", "8") and SUMMARY.search(r.stderr).group(4) == "max samples", r.stderr
    assert np.array_equal(np.asarray(Image.open(out)).reshape(-1, 3), python_film(pta, host, 8, 16, 1e-6)[0])
    # -v: one line per pass
    r = run("-v", "-q", "-p", profile_file, "--noise-target", 1e-6, "--min-samples", 4, "--max-samples", 60, "-o", tmp_path / "v.png")
    assert r.returncode == 0, r.stderr
    lines = re.findall(r"^film: pass (\d+): (\d+) samples \((\d+) in all\), noise \S+, over target \S+ of the blocks$", r.stderr, re.M)
    assert lines == [("1", "4", "4"), ("2", "8", "12"), ("3", "16", "28"), ("4", "32", "60")], r.stderr


def test_cli_resets_the_film_between_the_frames_of_a_camera_path(pta, tmp_path, profile_file):
    from PIL import Image
    host = pta.HostScene.load_isf(SCENE)
    cam = json.loads(SCENE.read_text())["camera"]
    moved = json.loads(json.dumps(cam))
    moved["transform"][3][0] += 0.3
    cams = tmp_path / "cams.json"
    cams.write_text(json.dumps([cam, moved]))
    r = run("-q", "-p", profile_file, "--noise-target", 1e-6, "--min-samples", 2, "--max-samples", 14, "--camera-path", cams,
            "--noise-map", tmp_path / "n.png", "-o", tmp_path / "f_%d.png")
    assert r.returncode == 0, r.stderr
    assert [m[:2] for m in SUMMARY.findall(r.stderr)] == [("3", "14"), ("3", "14")], r.stderr
    for i, c in enumerate((cam, moved)):
        want = python_film(pta, host, 2, 14, 1e-6, camera=c)[0]
        assert np.array_equal(np.asarray(Image.open(tmp_path / f"f_{i}.png")).reshape(-1, 3), want), i
        assert Image.open(tmp_path / f"n_{i}.png").size == (W, H)


def test_cli_filters_the_films_planes(pta, tmp_path, profile_file):
    from PIL import Image
    host = pta.HostScene.load_isf(SCENE)
    g = pta.GpuScene(host)
    film = pta.Film(pta.Profile.make(W, H, 16, BOUNCES))
    film.render_until(g, 2, 14, 1e-6)
    acc, mom = film.read()
    guides = g.render_guides(W, H)
    tm = pta.TONEMAPS["FILMIC"]
    want = {"--denoise": pta.denoise(W, H, 14, pta.DenoiseParams.default(tonemap=tm), acc, guides)[1],
            "--denoise-variance": pta.denoise_var(W, H, 14, pta.DenoiseParams.default_var(tonemap=tm), acc, mom, guides)[1]}
    film.close()
    for flag, rgb in want.items():
        out = tmp_path / f"{flag.strip('-')}.png"
        extra = ["--denoise"] + ([flag] if flag != "--denoise" else [])
        r = run("-q", "-p", profile_file, "--noise-target", 1e-6, "--min-samples", 2, "--max-samples", 14, *extra, "-o", out)
        assert r.returncode == 0 and SUMMARY.search(r.stderr), r.stderr
        assert np.array_equal(np.asarray(Image.open(out)).reshape(-1, 3), rgb), flag


def test_cli_refused_combinations_exit_with_2(tmp_path, profile_file):
    frames = tmp_path / "frames.json"
    frames.write_text("[{}, {}]")
    cases = {"light mixer": ["--noise-target", 0.1, "--keyframes", frames, "--light-mixer"],
             "several devices": ["--noise-target", 0.1, "--devices", "0,0"],
             "target 0": ["--noise-target", 0], "target inf": ["--noise-target", "inf"], "target nan": ["--noise-target", "nan"],
             "n0 below 2": ["--noise-target", 0.1, "--min-samples", 1],
             "n0 above N": ["--noise-target", 0.1, "--min-samples", 8, "--max-samples", 7],
             "n0 above the profile's samples": ["--noise-target", 0.1, "--min-samples", 17]}
    for label, args in cases.items():
        out = tmp_path / label.replace(" ", "_").replace("'", "")
        out.mkdir()
        r = run("-q", "-p", profile_file, *args, "-o", out / "f_%d.png")
        assert r.returncode == 2, (label, r.stderr)
        assert not list(out.iterdir()), label
