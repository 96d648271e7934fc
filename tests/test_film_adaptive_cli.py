"""`render --noise-target --adaptive`: the combinations the command line refuses (no GPU: they exit before any device work),
and one small run on the GPU - the PNG is the film pt_film_render_until_adaptive makes through Python, the summary line, the
per-pass lines of -v, the sample map and the noise map."""
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, SCENES

EXE = ROOT / "path-tracer_amd" / "path-tracer"
W, H, BOUNCES = 72, 40, 2
SCENE = SCENES / "cube" / "scene.isf"
SUMMARY = re.compile(r"^film: (\d+) passes, (\d+) samples, noise (\S+), (converged|max samples), pixel-samples (\d+) of (\d+)$", re.M)


def run(*args):
    return subprocess.run([str(EXE), "render", str(SCENE), *[str(a) for a in args]], capture_output=True, text=True, timeout=300)


@pytest.fixture(scope="module")
def profile_file(tmp_path_factory):
    p = tmp_path_factory.mktemp("film_adaptive_cli") / "p.yml"
    p.write_text(f"resolution:\n  width: {W}\n  height: {H}\nsamples: 56\nbounces: {BOUNCES}\n")
    return p


def test_cli_refuses_before_any_gpu_work(tmp_path, profile_file):
    out = tmp_path / "never.png"
    base = ("-q", "-p", profile_file, "-o", out)
    cases = [
        (("--adaptive",), "'--adaptive' needs '--noise-target <T>'"),
        (("--adaptive-tile", 16), "need '--noise-target <T> --adaptive'"),
        (("--uniform-samples", 16), "need '--noise-target <T> --adaptive'"),
        (("--adaptive-dilate", 0), "need '--noise-target <T> --adaptive'"),
        (("--sample-map", tmp_path / "s.png"), "need '--noise-target <T> --adaptive'"),
        (("--noise-target", 0.05, "--adaptive-tile", 16), "need '--noise-target <T> --adaptive'"),
        (("--noise-target", 0.05, "--sample-map", tmp_path / "s.png"), "need '--noise-target <T> --adaptive'"),
        (("--noise-target", 0.05, "--adaptive", "--denoise"), "cannot be used with '--denoise'"),
        (("--noise-target", 0.05, "--adaptive", "--denoise", "--denoise-variance"), "cannot be used with '--denoise'"),
        (("--noise-target", 0.05, "--adaptive", "--devices", "0,1"), "more than one device"),
        (("--noise-target", 0.05, "--adaptive", "--adaptive-tile", 12), "invalid value '12' for '--adaptive-tile <N>'"),
        (("--noise-target", 0.05, "--adaptive", "--adaptive-tile", 8), "invalid value '8' for '--adaptive-tile <N>'"),
        (("--noise-target", 0.05, "--adaptive", "--adaptive-tile", 0), "invalid value '0' for '--adaptive-tile <N>'"),
        (("--noise-target", 0.05, "--adaptive", "--adaptive-tile", "x"), "a whole number expected"),
        (("--noise-target", 0.05, "--adaptive", "--adaptive-dilate", 2), "0 or 1 expected"),
        (("--noise-target", 0.05, "--adaptive", "--uniform-samples", "-3"), "a whole number expected"),
        (("--noise-target", 0.05, "--adaptive", "--sample-map", tmp_path / "s.jpg"), "only .png output is supported"),
        (("--noise-target", 0.05, "--adaptive", "--sample-map"), "a value is required"),
    ]
    for args, message in cases:
        r = run(*base, *args)
        assert r.returncode == 2 and message in r.stderr, (args, r.returncode, r.stderr)
        assert not out.exists() and not (tmp_path / "s.png").exists()


@pytest.mark.gpu
def test_cli_writes_the_film_render_until_adaptive_makes(pta, tmp_path, profile_file):
    from PIL import Image
    host = pta.HostScene.load_isf(SCENE)
    target = 0.03
    g = pta.GpuScene(host)
    film = pta.Film(pta.Profile.make(W, H, 56, BOUNCES), pta.Opts.make(tile_w=16, tile_h=16))
    passes = []
    stats = film.render_until_adaptive(g, pta.FilmAdaptiveParams.default(target=target, first_pass_samples=8, uniform_samples=8,
                                                                         dilate=0, max_samples=56),
                                       lambda info, noise: passes.append((info.passes, info.last_pass_samples, film.adaptive_info.last_pass_tiles,
                                                                          noise.mean_error)))
    want, info, counts = film.resolve(), film.info, film.read_counts()
    err = film.tile_noise(target, want_planes=True)[1]
    assert film.adaptive_info.uniform == 0 and len(set(counts.tolist())) > 1    # (the run did go adaptive)
    film.close()
    g.close()
    out, smap, nmap = tmp_path / "o.png", tmp_path / "s.png", tmp_path / "n.png"
    r = run("-v", "-q", "-p", profile_file, "--noise-target", target, "--adaptive", "--adaptive-tile", 16, "--uniform-samples", 8,
            "--adaptive-dilate", 0, "--sample-map", smap, "--noise-map", nmap, "-o", out)
    assert r.returncode == 0, r.stderr
    assert np.array_equal(np.asarray(Image.open(out)).reshape(-1, 3), want)
    m = SUMMARY.search(r.stderr)
    assert m, r.stderr
    assert (int(m.group(1)), int(m.group(2))) == (info.passes, info.samples), r.stderr
    assert m.group(3) == f"{stats.mean_error:.6g}" and m.group(4) == ("converged" if stats.converged else "max samples")
    assert (int(m.group(5)), int(m.group(6))) == (int(counts.sum()), W * H * info.samples) and int(m.group(5)) < int(m.group(6))
    lines = re.findall(r"^film: pass (\d+): (\d+) samples, (\d+) of 15 tiles, noise (\S+)$", r.stderr, re.M)
    assert lines == [(str(p), str(s), str(t), f"{e:.6g}") for p, s, t, e in passes], r.stderr
    assert lines[0][2] == "15" and int(lines[-1][2]) < 15
    grey = np.asarray(Image.open(smap))
    assert grey.shape[:2] == (H, W)
    v = counts.astype(np.float32) / np.float32(info.samples) * np.float32(255)
    assert (grey.reshape(H * W, -1) == v.astype(np.uint8)[:, None]).all()
    grey = np.asarray(Image.open(nmap)).reshape(H * W, -1)
    v = np.minimum(np.float32(1), err / (np.float32(2) * np.float32(target))) * np.float32(255)
    assert (grey == v.astype(np.uint8)[:, None]).all()
