"""`render --temporal`: what it refuses (no GPU needed: every refusal comes before any GPU work) and, on the GPU, its frames
against the bytes of the Python API (History.add_frame, resolve, denoise)."""
import json
import subprocess

import numpy as np
import pytest

from conftest import ROOT, SCENES

EXE = ROOT / "path-tracer_amd" / "path-tracer"
SCENE = SCENES / "cube" / "scene.isf"
W, H, SPP, BOUNCES = 33, 17, 4, 2


def run(*args):
    return subprocess.run([str(EXE), "render", str(SCENE), "-q", *[str(a) for a in args]], capture_output=True, text=True, timeout=300)


def test_help_lists_the_flags_and_impossible_combinations_are_refused(tmp_path):
    r = subprocess.run([str(EXE), "render", "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0
    for flag in ("--temporal ", "--temporal-frames <H>", "--temporal-rotate <K>", "--temporal-normal-cos <C>", "--temporal-plane-tol <T>",
                 "--temporal-map <FILE_%04d.png>"):
        assert flag in r.stdout, flag
    out = tmp_path / "o_%d.png"
    path = ("--camera-path", "cams.json")
    refused = [
        (("--temporal",), "needs '--camera-path <CAMERAS>' or '--keyframes <FRAMES>'"),
        (("--temporal-frames", 4, *path), "need '--temporal'"),
        (("--temporal-rotate", 2, *path), "need '--temporal'"),
        (("--temporal-normal-cos", 0.5, *path), "need '--temporal'"),
        (("--temporal-plane-tol", 0.5, *path), "need '--temporal'"),
        (("--temporal-map", tmp_path / "m_%d.png", *path), "need '--temporal'"),
        (("--temporal", *path, "--noise-target", 0.1), "cannot be used with '--noise-target"),
        (("--temporal", *path, "--film-denoise", "plain"), "cannot be used with '--film-denoise"),
        (("--temporal", "--keyframes", "frames.json", "--light-mixer"), "cannot be used with '--light-mixer"),
        (("--temporal", *path, "--aov-dir", tmp_path / "aov"), "cannot be used with '--aov-dir"),
        (("--temporal", *path, "--denoise", "--denoise-guides", "samples"), "cannot be used with '--denoise-guides"),
        (("--temporal", *path, "--devices", "0,1"), "cannot be used with '--devices"),
        (("--temporal", *path, "--debug-textures"), "cannot be used with '--debug-textures"),
        (("--temporal", *path, "--temporal-frames", 0), "at least 1"),
        (("--temporal", *path, "--temporal-rotate", 0), "1 .. 4096 expected"),
        (("--temporal", *path, "--temporal-normal-cos", 2), "for '--temporal-normal-cos <C>'"),
        (("--temporal", *path, "--temporal-plane-tol", "x"), "for '--temporal-plane-tol <T>'"),
        (("--temporal", *path, "--temporal-map", tmp_path / "m.jpg"), "only .png output is supported"),
        (("--temporal", *path, "--temporal-frames", 1 << 23), "must stay below"),
    ]
    for args, message in refused:
        r = run("-o", out, *args)
        assert r.returncode == 2 and message in r.stderr, (args, r.stderr)
        assert not list(tmp_path.glob("*.png")), args


@pytest.fixture()
def profile_file(tmp_path):
    p = tmp_path / "p.yml"
    p.write_text(f"resolution: {{width: {W}, height: {H}}}\nsamples: {SPP}\nbounces: {BOUNCES}\n")
    return p


def cameras(n):
    cam = json.loads(SCENE.read_text())["camera"]
    out = []
    for k in range(n):
        c = json.loads(json.dumps(cam))
        c["transform"][3][0] += 0.05 * k
        out.append(c)
    return out


@pytest.mark.gpu
def test_temporal_frames_equal_the_python_api(tmp_path, pta, profile_file):
    from PIL import Image
    image = lambda path: np.asarray(Image.open(path)).reshape(-1, 3)
    prof = pta.Profile.make(W, H, SPP, BOUNCES)
    cams = cameras(4)
    (tmp_path / "cams.json").write_text(json.dumps(cams))
    for k, (extra, kw, denoise) in enumerate(((("--temporal-frames", 2, "--temporal-rotate", 3, "--temporal-normal-cos", 0.8, "--temporal-plane-tol", 0.05),
                                               dict(max_samples=2 * SPP, rotate=3, normal_cos=0.8, plane_tol=0.05), None),
                                              (("--denoise", "--denoise-iterations", 2), dict(max_samples=4 * SPP), False),
                                              (("--denoise", "--denoise-variance"), dict(max_samples=4 * SPP), True))):
        r = run("-p", profile_file, "-o", tmp_path / f"t{k}_%02d.png", "--temporal", "--camera-path", tmp_path / "cams.json",
                "--temporal-map", tmp_path / f"m{k}_%d.png", *extra)
        assert r.returncode == 0, r.stderr
        g = pta.GpuScene(pta.HostScene.load_isf(SCENE))
        hist = pta.History(W, H, pta.HistoryParams.default(**kw))
        reached = 0
        for f, c in enumerate(cams):
            g.set_camera(c)
            hist.add_frame(g, prof, f)
            if denoise is None:
                want = hist.resolve("FILMIC")[0]
            else:
                params = pta.DenoiseParams.default_var() if denoise else pta.DenoiseParams.default(iterations=2)
                want = hist.denoise(params, denoise)[1]
            assert np.array_equal(image(tmp_path / f"t{k}_{f:02d}.png"), want), (k, f)
            hmap = hist.read_map()
            grey = np.where(hmap >= 0, 255, 32 * (-hmap - 1)).astype(np.uint8)
            assert np.array_equal(image(tmp_path / f"m{k}_{f}.png"), np.repeat(grey[:, None], 3, axis=1)), (k, f)
            reached += int((hmap >= 0).sum())
        assert reached > 0 and hist.info.max_count > SPP
        hist.close()
        g.close()


@pytest.mark.gpu
def test_one_frame_without_rotation_is_the_plain_render(tmp_path, profile_file):
    (tmp_path / "one.json").write_text(json.dumps(cameras(1)))
    plain, temporal = tmp_path / "plain.png", tmp_path / "temporal.png"
    r = run("-p", profile_file, "-o", plain, "--camera-path", tmp_path / "one.json")
    assert r.returncode == 0, r.stderr
    r = run("-p", profile_file, "-o", temporal, "--camera-path", tmp_path / "one.json", "--temporal", "--temporal-rotate", 1,
            "--temporal-frames", 1)
    assert r.returncode == 0, r.stderr
    assert plain.read_bytes() == temporal.read_bytes()


@pytest.mark.gpu
def test_a_keyframe_that_edits_the_lights_resets_the_history(tmp_path, pta, profile_file):
    from PIL import Image
    image = lambda path: np.asarray(Image.open(path)).reshape(-1, 3)
    cams = cameras(3)
    light = {"type": "Point", "position": [0.5, 3.0, 1.0], "color": [6.0, 5.0, 4.0], "size": 0.1}
    frames = [{"camera": cams[0]}, {"camera": cams[1]}, {"camera": cams[2], "lights": [light]}]
    (tmp_path / "frames.json").write_text(json.dumps(frames))
    r = run("-p", profile_file, "-o", tmp_path / "k_%d.png", "--temporal", "--keyframes", tmp_path / "frames.json")
    assert r.returncode == 0, r.stderr
    prof = pta.Profile.make(W, H, SPP, BOUNCES)
    host = pta.HostScene.load_isf(SCENE)
    keys = pta.load_keyframes(tmp_path / "frames.json")
    host.apply_keyframe(keys[0])
    g = pta.GpuScene(host)
    hist = pta.History(W, H, pta.HistoryParams.default(max_samples=4 * SPP))
    for f in range(3):
        if f:
            g.apply_keyframe(keys[f], host)
        if f and (keys[f].has_lights or keys[f].n_materials):
            hist.reset()
        hist.add_frame(g, prof, f)
        assert np.array_equal(image(tmp_path / f"k_{f}.png"), hist.resolve("FILMIC")[0]), f
        assert hist.info.max_count == (2 * SPP if f == 1 else SPP), f       # the third frame started afresh
    hist.close()
    g.close()
    keys.close()
