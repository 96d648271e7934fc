"""`render --denoise-guides` and `render --aov-dir`: what they refuse (no GPU needed: every refusal comes before any GPU work)
and, on the GPU, their files against the bytes of the Python entry points."""
import json
import subprocess

import numpy as np
import pytest

from conftest import ROOT, SCENES

f32 = np.float32
EXE = ROOT / "path-tracer_amd" / "path-tracer"
SCENE = SCENES / "alpha_transparency" / "scene.isf"
W, H, SPP, BOUNCES = 33, 17, 4, 2


def run(*args):
    return subprocess.run([str(EXE), "render", str(SCENE), "-q", *[str(a) for a in args]], capture_output=True, text=True, timeout=300)


def as_u8(v):
    v = np.asarray(v, f32)
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(v) | (v <= 0), 0, np.where(v >= 255, 255, np.trunc(np.nan_to_num(v)))).astype(np.uint8)


def test_help_lists_the_flags_and_impossible_combinations_are_refused(tmp_path):
    r = subprocess.run([str(EXE), "render", "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--denoise-guides <centre|samples>" in r.stdout and "--aov-dir <DIR>" in r.stdout
    out, aov = tmp_path / "o.png", tmp_path / "aov"
    refused = [
        (("--denoise-guides", "samples"), "needs '--denoise'"),
        (("--denoise-guides", "centre"), "needs '--denoise'"),
        (("--denoise", "--denoise-guides", "pixels"), "centre or samples expected"),
        (("--denoise", "--denoise-guides"), "a value is required"),
        (("--denoise-guides", "samples", "--noise-target", "0.1", "--film-denoise", "plain"), "cannot be used with '--film-denoise"),
        (("--denoise", "--denoise-guides", "samples", "--noise-target", "0.1"), "cannot be used with '--noise-target"),
        (("--denoise", "--denoise-guides", "samples", "--devices", "0,1"), "--denoise"),
        (("--aov-dir", aov, "--camera-path", "cams.json"), "cannot be used with '--camera-path"),
        (("--aov-dir", aov, "--keyframes", "frames.json"), "cannot be used with '--keyframes"),
        (("--aov-dir", aov, "--noise-target", "0.1"), "cannot be used with '--noise-target"),
        (("--aov-dir", aov, "--devices", "0,1"), "cannot be used with '--devices"),
        (("--aov-dir", aov, "--debug-textures"), "cannot be used with '--debug-textures"),
        (("--aov-dir=",), "a directory name expected"),
    ]
    for args, message in refused:
        r = run("-o", out, *args)
        assert r.returncode == 2 and message in r.stderr, (args, r.stderr)
        assert not out.exists() and not aov.exists(), args


@pytest.fixture()
def profile_file(tmp_path):
    p = tmp_path / "p.yml"
    p.write_text(f"resolution: {{width: {W}, height: {H}}}\nsamples: {SPP}\nbounces: {BOUNCES}\n")
    return p


@pytest.mark.gpu
def test_denoise_guides_samples_writes_render_denoised_aov(tmp_path, pta, gpu_scene_cache, profile_file):
    from PIL import Image
    g = gpu_scene_cache("alpha_transparency")
    prof = pta.Profile.make(W, H, SPP, BOUNCES)
    image = lambda path: np.asarray(Image.open(path)).reshape(-1, 3)
    for variance in (False, True):
        params = (pta.DenoiseParams.default_var if variance else pta.DenoiseParams.default)(iterations=3)
        extra = ("--denoise-variance",) if variance else ()
        out, centre = tmp_path / f"s{int(variance)}.png", tmp_path / f"c{int(variance)}.png"
        r = run("-p", profile_file, "-o", out, "--denoise", "--denoise-iterations", 3, "--denoise-guides", "samples", *extra)
        assert r.returncode == 0, r.stderr
        assert np.array_equal(image(out), g.render_denoised_aov(prof, params, variance=variance)[0]), variance
        # the default and `centre` are today's bytes
        want = (g.render_denoised_var if variance else g.render_denoised)(prof, params)[0]
        for k, more in enumerate(((), ("--denoise-guides", "centre"))):
            r = run("-p", profile_file, "-o", centre, "--denoise", "--denoise-iterations", 3, *more, *extra)
            assert r.returncode == 0, r.stderr
            assert np.array_equal(image(centre), want), (variance, k)
        assert not np.array_equal(image(out), want)
    # a camera path: every frame through the sample guides
    cam = json.loads(SCENE.read_text())["camera"]
    moved = json.loads(json.dumps(cam))
    moved["transform"][3][0] += 0.2
    cams = tmp_path / "cams.json"
    cams.write_text(json.dumps([cam, moved]))
    r = run("-p", profile_file, "-o", tmp_path / "f_%d.png", "--denoise", "--denoise-guides", "samples", "--camera-path", cams)
    assert r.returncode == 0, r.stderr
    fresh = pta.GpuScene(pta.HostScene.load_isf(SCENE))
    for i, c in enumerate((cam, moved)):
        fresh.set_camera(c)
        assert np.array_equal(image(tmp_path / f"f_{i}.png"), fresh.render_denoised_aov(prof, pta.DenoiseParams.default())[0]), i
    fresh.close()


@pytest.mark.gpu
def test_aov_dir_writes_the_four_planes(tmp_path, pta, gpu_scene_cache, profile_file):
    from PIL import Image
    g = gpu_scene_cache("alpha_transparency")
    prof = pta.Profile.make(W, H, SPP, BOUNCES)
    out, d = tmp_path / "o.png", tmp_path / "planes" / "aov"
    r = run("-p", profile_file, "-o", out, "--aov-dir", d)
    assert r.returncode == 0, r.stderr
    image = lambda path: np.asarray(Image.open(path)).reshape(-1, 3)
    assert np.array_equal(image(out), g.render(prof)[0])
    a = g.render_aov(prof)
    cov, fn = a[:, 7], f32(SPP)
    covered = cov > 0
    with np.errstate(all="ignore"):
        nn = ((a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]).astype(f32) + a[:, 2] * a[:, 2]).astype(f32)
        inv = np.where((nn > 0) & (nn < np.inf), f32(1.0) / np.sqrt(nn), f32(0)).astype(f32)
        z = (a[:, 3] / cov).astype(f32)
        zmax = z[covered & np.isfinite(z)].max()
        want = {"albedo": (a[:, 4:7] / fn).astype(f32) * f32(255.0),
                "normal": ((a[:, 0:3] * inv[:, None]).astype(f32) * f32(0.5) + f32(0.5)).astype(f32) * f32(255.0),
                "depth": np.repeat(((z / zmax).astype(f32) * f32(255.0))[:, None], 3, axis=1),
                "alpha": np.repeat(((cov / fn).astype(f32) * f32(255.0))[:, None], 3, axis=1)}
    assert covered.any() and not covered.all() and ((cov > 0) & (cov < fn)).any(), "misses and partly covered pixels"
    for name, v in want.items():
        assert np.array_equal(image(d / f"{name}.png"), np.where(covered[:, None], as_u8(v), 0)), name
    assert sorted(p.name for p in d.iterdir()) == ["albedo.png", "alpha.png", "depth.png", "normal.png"]
