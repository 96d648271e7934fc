"""`render --noise-target .. --film-devices A,B,..`: the film held by several shard films (here: several on the one GPU, the
rehearsal mode) writes the PNG and the maps of the same command without --film-devices, byte for byte - the adaptive film, the
windowed film, and with a final --film-denoise.  The refusals are in test_film_shard_model.py (they need no GPU)."""
import json
import subprocess

import pytest

from conftest import ROOT, SCENES

pytestmark = pytest.mark.gpu

EXE = ROOT / "path-tracer_amd" / "path-tracer"
W, H, BOUNCES = 72, 40, 2
SCENE = SCENES / "cube" / "scene.isf"


def run(*args):
    return subprocess.run([str(EXE), "render", str(SCENE), *[str(a) for a in args]], capture_output=True, text=True, timeout=300)


@pytest.fixture(scope="module")
def profile(tmp_path_factory):
    path = tmp_path_factory.mktemp("film_shard_cli") / "p.yml"
    path.write_text(f"resolution:\n  width: {W}\n  height: {H}\nsamples: 56\nbounces: {BOUNCES}\n")
    return path


def film_lines(stderr):
    return [line for line in stderr.splitlines() if line.startswith("film:")]


@pytest.mark.parametrize("extra", ((), ("--window-samples", 5), ("--film-denoise", "variance")),
                         ids=("adaptive", "windowed", "film-denoise"))
def test_film_devices_write_the_one_device_runs_bytes(tmp_path, profile, extra):
    args = ("-v", "-q", "-p", profile, "--noise-target", 0.03, "--adaptive", "--adaptive-tile", 16, "--uniform-samples", 8, *extra)
    if "--window-samples" not in extra:
        args += ("--min-samples", 8)
    want = {}
    for label, more in (("one", ()), ("two", ("--film-devices", "0,0")), ("three", ("--film-devices", "0,0,0", "--stats"))):
        d = tmp_path / label
        d.mkdir()
        r = run(*args, *more, "-o", d / "o.png", "--sample-map", d / "s.png", "--noise-map", d / "n.png")
        assert r.returncode == 0, (label, r.stderr)
        got = {"png": (d / "o.png").read_bytes(), "samples": (d / "s.png").read_bytes(), "noise": (d / "n.png").read_bytes(),
               "film": film_lines(r.stderr)}
        if label == "one":
            want = got
            # the runs below mean something only if the selection bites: some pass renders fewer tiles than all 15
            assert any(" of 15 tiles" in line and " 15 of 15 tiles" not in line for line in got["film"]), r.stderr
        else:
            for key in want:
                assert got[key] == want[key], (label, key)
        if "--stats" in more:
            stats = json.loads([line for line in r.stderr.splitlines() if line.startswith("{")][-1])
            assert stats["film_devices"] == 3
