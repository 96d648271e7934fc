"""Camera paths on the host: pth_camera_path_load (a JSON array of ISF cameras), pth_scene_set_camera, the CLI's checks of
`render --camera-path` (all made before any GPU work: exit code 2) and tools/make_orbit.py.  No GPU."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
SCENES = ROOT / "tests" / "golden" / "scenes"
EXE = ROOT / "path-tracer_amd" / "path-tracer"
GOLDEN = ["alpha_transparency", "cube", "head", "reflection", "spheres", "white_furnace_direct", "white_furnace_indirect"]


def cam_bits(cam):
    return np.array(list(cam.transform) + [cam.fov, cam.zfar, cam.znear], np.float32).view(np.uint32)


def isf_camera(name):
    return json.loads((SCENES / name / "scene.isf").read_text())["camera"]


def test_camera_path_round_trips_the_golden_cameras(pta, tmp_path):
    path = tmp_path / "cams.json"
    path.write_text(json.dumps([isf_camera(n) for n in GOLDEN]))
    cams = pta.load_camera_path(path)
    assert len(cams) == len(GOLDEN)
    for name, cam in zip(GOLDEN, cams):
        scene = pta.HostScene.load_isf(SCENES / name / "scene.isf")
        assert np.array_equal(cam_bits(cam), cam_bits(scene.desc.contents.camera)), name
        # and back through the dict form the Python layer writes (tools/make_orbit.py)
        again = tmp_path / f"{name}.json"
        again.write_text(json.dumps([pta.camera_to_dict(cam)]))
        assert np.array_equal(cam_bits(pta.load_camera_path(again)[0]), cam_bits(cam))


@pytest.mark.parametrize("field", ["transform", "fov", "zfar", "znear"])
def test_missing_field_gives_the_isf_message(pta, tmp_path, field):
    cam = isf_camera("cube")
    del cam[field]
    path = tmp_path / "cams.json"
    path.write_text(json.dumps([isf_camera("cube"), cam]))
    with pytest.raises(pta.PtError) as e:
        pta.load_camera_path(path)
    assert e.value.code == -3 and f"missing field `{field}`" in str(e.value)
    # the ISF loader says the same about a scene's camera
    scene = json.loads((SCENES / "cube" / "scene.isf").read_text())
    scene["camera"] = cam
    (tmp_path / "scene.isf").write_text(json.dumps(scene))
    with pytest.raises(pta.PtError) as e2:
        pta.HostScene.load_isf(tmp_path / "scene.isf")
    assert f"missing field `{field}`" in str(e2.value)


@pytest.mark.parametrize("text", ["[]", " [ ] ", "{}", json.dumps(isf_camera("cube")), "3", "", "[", "[{}"])
def test_empty_or_non_array_is_a_parse_error(pta, tmp_path, text):
    path = tmp_path / "cams.json"
    path.write_text(text)
    with pytest.raises(pta.PtError) as e:
        pta.load_camera_path(path)
    assert e.value.code == -3


def test_missing_file_is_an_io_error(pta, tmp_path):
    with pytest.raises(pta.PtError) as e:
        pta.load_camera_path(tmp_path / "nope.json")
    assert e.value.code == -2


def test_host_scene_set_camera(pta):
    scene = pta.HostScene.load_isf(SCENES / "head" / "scene.isf")
    other = isf_camera("cube")
    scene.set_camera(other)
    ref = pta.make_camera(other)
    assert np.array_equal(cam_bits(scene.camera), cam_bits(ref))
    assert np.array_equal(cam_bits(scene.desc.contents.camera), cam_bits(ref))
    with pytest.raises(pta.PtError) as e:
        scene.set_camera(None)
    assert e.value.code == -1


def run_cli(*args, cwd=None):
    return subprocess.run([str(EXE), *map(str, args)], capture_output=True, text=True, cwd=cwd,
                          env=dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES=""))


def test_cli_help_lists_camera_path():
    r = run_cli("render", "--help")
    assert r.returncode == 0 and "--camera-path" in r.stdout


@pytest.mark.parametrize("case", ["no_field", "unreadable", "invalid", "empty", "debug_textures", "two_fields", "bad_field"])
def test_cli_camera_path_errors_exit_2_before_gpu_work(tmp_path, case):
    cams = tmp_path / "cams.json"
    cams.write_text(json.dumps([isf_camera("cube")] * 3))
    out = tmp_path / "frame_%03d.png"
    extra = []
    if case == "no_field":
        out = tmp_path / "frame.png"
    elif case == "unreadable":
        cams = tmp_path / "missing.json"
    elif case == "invalid":
        cams.write_text('[{"fov": 1.0}]')
    elif case == "empty":
        cams.write_text("[]")
    elif case == "debug_textures":
        extra = ["--debug-textures"]
    elif case == "two_fields":
        out = tmp_path / "f_%d_%d.png"
    elif case == "bad_field":
        out = tmp_path / "f_%x.png"
    # (the GPU is hidden: had the CLI got as far as the device, it would fail there with another message)
    r = run_cli("render", SCENES / "cube" / "scene.isf", "--camera-path", cams, "-o", out, *extra, cwd=tmp_path)
    assert r.returncode == 2 and r.stderr.strip(), (case, r.stderr)
    assert "device" not in r.stderr.lower(), r.stderr
    assert not list(tmp_path.glob("*.png"))


def test_make_orbit(pta, tmp_path):
    out = tmp_path / "orbit.json"
    r = subprocess.run([sys.executable, str(ROOT / "tools" / "make_orbit.py"), str(SCENES / "head" / "scene.isf"), "12",
                        "--axis", "y", "-o", str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    cams = pta.load_camera_path(out)
    assert len(cams) == 12
    scene = pta.HostScene.load_isf(SCENES / "head" / "scene.isf")
    assert np.array_equal(cam_bits(cams[0]), cam_bits(scene.camera))
    sys.path.insert(0, str(ROOT / "tools"))
    try:
        import make_orbit
    finally:
        sys.path.pop(0)
    pivot = make_orbit.scene_box_centre(scene)
    pos = np.array([list(c.transform)[12:15] for c in cams], np.float64)
    dist = np.linalg.norm(pos - pivot, axis=1)
    assert np.allclose(dist, dist[0], rtol=1e-6, atol=0)
    assert np.allclose(pos[:, 1], pos[0, 1], rtol=1e-6, atol=1e-6)   # (about y: the height stays)
    assert len({tuple(p) for p in pos.round(4)}) == 12
    for c in cams:   # fov / zfar / znear kept
        assert (c.fov, c.zfar, c.znear) == (cams[0].fov, cams[0].zfar, cams[0].znear)
