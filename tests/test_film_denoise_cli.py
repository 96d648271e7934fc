"""`render --noise-target --film-denoise` and `--filtered-target`: the combinations the command line refuses (no GPU: they exit
before any device work), and on the GPU the PNGs against the films Film.denoise and Film.render_until_filtered make through
Python, the summary line and the noise map of the filtered error."""
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, SCENES

EXE = ROOT / "path-tracer_amd" / "path-tracer"
W, H, BOUNCES = 72, 40, 2
SCENE = SCENES / "cube" / "scene.isf"
SUMMARY = re.compile(r"^film: (\d+) passes, (\d+) samples, (filtered noise|noise) (\S+), (converged|max samples), "
                     r"pixel-samples (\d+) of (\d+)$", re.M)


def run(*args):
    return subprocess.run([str(EXE), "render", str(SCENE), *[str(a) for a in args]], capture_output=True, text=True, timeout=300)


@pytest.fixture(scope="module")
def profile_file(tmp_path_factory):
    p = tmp_path_factory.mktemp("film_denoise_cli") / "p.yml"
    p.write_text(f"resolution:\n  width: {W}\n  height: {H}\nsamples: 56\nbounces: {BOUNCES}\n")
    return p


def test_cli_refuses_before_any_gpu_work(tmp_path, profile_file):
    out = tmp_path / "never.png"
    base = ("-q", "-p", profile_file, "-o", out)
    cases = [
        (("--film-denoise", "variance"), "'--film-denoise <plain|variance>' needs '--noise-target <T>'"),
        (("--film-denoise", "plain", "--adaptive"), "needs '--noise-target <T>'"),
        (("--noise-target", 0.05, "--film-denoise", "both"), "invalid value 'both' for '--film-denoise <plain|variance>'"),
        (("--noise-target", 0.05, "--film-denoise"), "a value is required"),
        (("--noise-target", 0.05, "--film-denoise", "variance", "--denoise"), "cannot be used with '--denoise'"),
        (("--noise-target", 0.05, "--film-denoise", "plain", "--denoise", "--denoise-variance"), "cannot be used with '--denoise'"),
        (("--noise-target", 0.05, "--film-denoise", "variance", "--devices", "0,1"), "more than one device"),
        (("--filtered-target",), "'--filtered-target' needs '--adaptive --film-denoise variance'"),
        (("--noise-target", 0.05, "--filtered-target"), "'--filtered-target' needs '--adaptive --film-denoise variance'"),
        (("--noise-target", 0.05, "--adaptive", "--filtered-target"), "'--filtered-target' needs '--adaptive --film-denoise variance'"),
        (("--noise-target", 0.05, "--film-denoise", "variance", "--filtered-target"), "'--filtered-target' needs '--adaptive --film-denoise variance'"),
        (("--noise-target", 0.05, "--adaptive", "--film-denoise", "plain", "--filtered-target"), "cannot be used with '--film-denoise plain'"),
        (("--noise-target", 0.05, "--film-denoise", "variance", "--denoise-iterations", 9), "0..8 expected"),
        # what was refused before stays refused, in the same words
        (("--noise-target", 0.05, "--adaptive", "--denoise"), "the filters take one sample count for the whole frame"),
        (("--denoise-iterations", 2), "'--denoise-iterations <N>' needs '--denoise'"),
    ]
    for args, message in cases:
        r = run(*base, *args)
        assert r.returncode == 2 and message in r.stderr, (args, r.returncode, r.stderr)
        assert not out.exists()
    r = subprocess.run([str(EXE), "render", "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--film-denoise <plain|variance>" in r.stdout and "--filtered-target" in r.stdout


ADAPTIVE = dict(first_pass_samples=8, uniform_samples=8, dilate=0, max_samples=56)
ADAPTIVE_ARGS = ("--adaptive", "--adaptive-tile", 16, "--uniform-samples", 8, "--adaptive-dilate", 0)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,iterations", (("variance", None), ("plain", 2)))
def test_cli_film_denoise_writes_what_film_denoise_makes(pta, tmp_path, profile_file, kind, iterations):
    from PIL import Image
    target = 0.03
    prof = pta.Profile.make(W, H, 56, BOUNCES)
    g = pta.GpuScene(pta.HostScene.load_isf(SCENE))
    film = pta.Film(prof, pta.Opts.make(tile_w=16, tile_h=16))
    film.render_until_adaptive(g, pta.FilmAdaptiveParams.default(target=target, **ADAPTIVE))
    assert film.adaptive_info.uniform == 0      # (the run did go adaptive)
    make = pta.DenoiseParams.default_var if kind == "variance" else pta.DenoiseParams.default
    params = make(tonemap=prof.tonemap) if iterations is None else make(tonemap=prof.tonemap, iterations=iterations)
    _, want = film.denoise(g, params, variance=kind == "variance")
    raw = film.resolve()
    # a uniform film goes the same way
    flat = pta.Film(prof)
    flat.render_until(g, 8, 56, target)
    _, want_flat = flat.denoise(g, params, variance=kind == "variance")
    for f in (film, flat):
        f.close()
    g.close()
    extra = () if iterations is None else ("--denoise-iterations", iterations)
    out = tmp_path / "o.png"
    r = run("-q", "-p", profile_file, "--noise-target", target, *ADAPTIVE_ARGS, "--film-denoise", kind, *extra, "-o", out)
    assert r.returncode == 0, r.stderr
    got = np.asarray(Image.open(out)).reshape(-1, 3)
    assert np.array_equal(got, want) and not np.array_equal(got, raw)
    m = SUMMARY.search(r.stderr)
    assert m and m.group(3) == "noise", r.stderr
    r = run("-q", "-p", profile_file, "--noise-target", target, "--film-denoise", kind, *extra, "-o", out)
    assert r.returncode == 0, r.stderr
    assert np.array_equal(np.asarray(Image.open(out)).reshape(-1, 3), want_flat)


@pytest.mark.gpu
def test_cli_filtered_target_writes_what_render_until_filtered_makes(pta, tmp_path, profile_file):
    from PIL import Image
    target = 0.012
    prof = pta.Profile.make(W, H, 56, BOUNCES)
    g = pta.GpuScene(pta.HostScene.load_isf(SCENE))
    film = pta.Film(prof, pta.Opts.make(tile_w=16, tile_h=16))
    flt = pta.DenoiseParams.default_var(tonemap=prof.tonemap, iterations=2)
    stats = film.render_until_filtered(g, pta.FilmFilteredParams.default(filter=flt, target=target, **ADAPTIVE))
    _, want = film.denoise(g, flt)
    info, counts = film.info, film.read_counts()
    ferr = film.filtered_noise(g, flt, target, want_planes=True)[1]
    raw_err = film.tile_noise(target, want_planes=True)[1]
    film.close()
    g.close()
    out, nmap = tmp_path / "o.png", tmp_path / "n.png"
    r = run("-q", "-p", profile_file, "--noise-target", target, *ADAPTIVE_ARGS, "--film-denoise", "variance", "--denoise-iterations", 2,
            "--filtered-target", "--noise-map", nmap, "-o", out)
    assert r.returncode == 0, r.stderr
    assert np.array_equal(np.asarray(Image.open(out)).reshape(-1, 3), want)
    m = SUMMARY.search(r.stderr)
    assert m and m.group(3) == "filtered noise", r.stderr
    assert (int(m.group(1)), int(m.group(2))) == (info.passes, info.samples), r.stderr
    assert m.group(4) == f"{stats.mean_error:.6g}" and m.group(5) == ("converged" if stats.converged else "max samples")
    assert (int(m.group(6)), int(m.group(7))) == (int(counts.sum()), W * H * info.samples)
    grey = np.asarray(Image.open(nmap)).reshape(H * W, -1)
    v = np.minimum(np.float32(1), ferr / (np.float32(2) * np.float32(target))) * np.float32(255)
    assert (grey == v.astype(np.uint8)[:, None]).all()
    raw = np.minimum(np.float32(1), raw_err / (np.float32(2) * np.float32(target))) * np.float32(255)
    assert not (grey == raw.astype(np.uint8)[:, None]).all()      # (the map is the filtered error, not the raw one)
