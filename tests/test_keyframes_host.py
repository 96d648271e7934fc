"""Light and material edits on the host: pth_keyframes_load (a JSON array of frames of camera / lights / material edits),
pth_scene_set_lights / pth_scene_set_materials and their checks, pth_keyframe_apply, save_isf of an edited scene, the CLI's
checks of `render --keyframes` (all made before any GPU work: exit code 2), and the host half of the device's orthographic
grid extent (params_ortho factored into axes, extent and parameters).  No GPU."""
import ctypes as C
import hashlib
import json
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
SCENES = ROOT / "tests" / "golden" / "scenes"
EXE = ROOT / "path-tracer_amd" / "path-tracer"
GOLDEN = ["alpha_transparency", "cube", "head", "reflection", "spheres", "white_furnace_direct", "white_furnace_indirect"]


def load(pta, name):
    return pta.HostScene.load_isf(SCENES / name / "scene.isf")


def raw(struct):
    return bytes(C.string_at(C.addressof(struct), C.sizeof(struct)))


def point(pta, pos, color=(1.0, 1.0, 1.0)):
    return pta.Light(pta.PT_LIGHT_POINT, (C.c_float * 3)(*pos), (C.c_float * 3)(*color), 0.1)


def directional(pta, d, color=(1.0, 1.0, 1.0)):
    return pta.Light(pta.PT_LIGHT_DIRECTIONAL, (C.c_float * 3)(*d), (C.c_float * 3)(*color), 0.0)


def write(tmp_path, obj, name="frames.json"):
    p = tmp_path / name
    p.write_text(obj if isinstance(obj, str) else json.dumps(obj))
    return p


def test_keyframes_parse(pta, tmp_path):
    cam = json.loads((SCENES / "head" / "scene.isf").read_text())["camera"]
    frames = [
        {},
        {"camera": cam},
        {"lights": [{"type": "Point", "position": [1, 2, 3], "color": [4, 5, 6], "size": 0.5},
                    {"type": "Directional", "direction": [0, -1, 0], "color": [0.5, 0.5, 0.5]}]},
        {"lights": []},
        {"materials": {"0": {"albedo": {"factor": [0.1, 0.2, 0.3]}, "ior": 1.5},
                       "2": {"opacity": {"factor": 0.25}, "emissive": {"factor": [1, 2, 3]},
                             "metalness": {"factor": 0.75}, "roughness": {"factor": 0.125}}}},
    ]
    kf = pta.load_keyframes(write(tmp_path, frames))
    assert len(kf) == 5
    f0, f1, f2, f3, f4 = list(kf)
    assert (f0.has_camera, f0.has_lights, f0.n_materials) == (0, 0, 0)
    assert f1.has_camera == 1 and f1.camera.fov == np.float32(cam["fov"])
    assert list(f1.camera.transform) == [float(np.float32(v)) for col in cam["transform"] for v in col]
    lights = pta.Keyframes.lights(f2)
    assert [(l.kind, list(l.vec), list(l.color), l.size) for l in lights] == [
        (pta.PT_LIGHT_POINT, [1, 2, 3], [4, 5, 6], 0.5), (pta.PT_LIGHT_DIRECTIONAL, [0, -1, 0], [0.5, 0.5, 0.5], 0.0)]
    assert f3.has_lights == 1 and pta.Keyframes.lights(f3) == []
    assert pta.Keyframes.lights(f4) is None
    edits = pta.Keyframes.material_edits(f4)
    assert [(e.index, e.fields) for e in edits] == [(0, pta.PTH_MAT_ALBEDO | pta.PTH_MAT_IOR),
                                                     (2, pta.PTH_MAT_OPACITY | pta.PTH_MAT_EMISSIVE | pta.PTH_MAT_METALNESS | pta.PTH_MAT_ROUGHNESS)]
    assert list(edits[0].albedo) == [float(np.float32(v)) for v in (0.1, 0.2, 0.3)] and edits[0].ior == 1.5
    assert (edits[1].opacity, list(edits[1].emissive), edits[1].metalness, edits[1].roughness) == (0.25, [1, 2, 3], 0.75, 0.125)
    kf.close()


@pytest.mark.parametrize("text, message", [
    ('{"camera": {}}', "expected an array of keyframes at line 1 column 1"),
    ("[]", "the keyframe file holds no frame at line 1 column 2"),
    ("", "EOF while parsing a value"),
    ('[{"camera_": {}}]', "unknown field `camera_`"),
    ('[{},\n {"materials": {"0": {"albedo": {"texture": "a.png"}}}}]', "a material edit cannot change a texture (`texture`) at line 2"),
    ('[{"materials": {"0": {"albedo": {"factor": [1, 1, 1], "texture": null}}}}]', "cannot change a texture"),
    ('[{"materials": {"0": {"normal_texture": "n.png"}}}]', "cannot change a texture (`normal_texture`)"),
    ('[{"materials": {"0": {"albedo": {}}}}]', "missing field `factor`"),
    ('[{"materials": {"0": {"shininess": 3}}}]', "unknown field `shininess`"),
    ('[{"materials": {"zero": {"ior": 1}}}]', "material index `zero` is not a decimal number"),
    ('[{"materials": {"-1": {"ior": 1}}}]', "is not a decimal number"),
    ('[{"lights": [{"type": "Point", "color": [1, 1, 1], "size": 1}]}]', "missing field `position`"),
    ('[{"lights": [{"type": "Point", "position": [1, 1, 1], "size": 1}]}]', "missing field `color`"),
    ('[{"lights": [{"type": "Point", "position": [1, 1, 1], "color": [1, 1, 1]}]}]', "missing field `size`"),
    ('[{"lights": [{"type": "Directional", "color": [1, 1, 1]}]}]', "missing field `direction`"),
    ('[{"lights": [{"position": [1, 1, 1]}]}]', "missing field `type`"),
    ('[{"lights": [{"type": "Spot"}]}]', "unknown variant `Spot`, expected `Point` or `Directional`"),
    ('[{"camera": {"fov": 1, "zfar": 1, "znear": 1}}]', "missing field `transform`"),
    ('[{}] x', "trailing characters"),
])
def test_keyframe_errors(pta, tmp_path, text, message):
    with pytest.raises(pta.PtError) as e:
        pta.load_keyframes(write(tmp_path, text))
    assert e.value.code == pta.PT_ERR_PARSE
    assert message in str(e.value)
    if "line" not in message and "unknown variant" not in message:   # (parse_light's message for a bad type has no position)
        assert " at line " in str(e.value)


def test_missing_keyframe_file(pta, tmp_path):
    with pytest.raises(pta.PtError) as e:
        pta.load_keyframes(tmp_path / "nope.json")
    assert e.value.code == pta.PT_ERR_IO


def test_set_lights_validation(pta):
    h = load(pta, "head")
    before = [raw(l) for l in h.lights]
    bad = point(pta, (0, 1, 0))
    bad.kind = 7
    with pytest.raises(pta.PtError) as e:
        h.set_lights([point(pta, (0, 1, 0)), bad])
    assert e.value.code == pta.PT_ERR_INVALID and "light 1: bad kind" in str(e.value)
    with pytest.raises(pta.PtError) as e:
        h.set_lights(None, n=1)
    assert e.value.code == pta.PT_ERR_INVALID
    assert [raw(l) for l in h.lights] == before
    h.set_lights(None)   # (null with 0: no lights)
    assert h.n_lights == 0
    new = [point(pta, (1, 2, 3)), directional(pta, (0, -1, 0)), point(pta, (-1, 2, 0))]
    h.set_lights(new)
    assert [raw(l) for l in h.lights] == [raw(l) for l in new] and h.n_lights == 3


def test_set_materials_validation(pta):
    h = load(pta, "head")   # (one material: an albedo texture, 3 channels, and an opacity texture, 1)
    mats = h.materials
    before = [raw(m) for m in mats]
    n_tex = h.desc.contents.n_textures
    cases = {
        "count": (mats + mats, "2 materials, the scene has 1"),
    }
    wrong = [pta.Material.from_buffer_copy(raw(m)) for m in mats]
    wrong[0].tex_albedo = n_tex
    cases["range"] = (wrong, "material 0: texture index out of range")
    chan = [pta.Material.from_buffer_copy(raw(m)) for m in mats]
    k = next(i for i, m in enumerate(chan) if m.tex_opacity >= 0)
    chan[0].tex_albedo = chan[k].tex_opacity   # a 1-channel texture where 3 are demanded
    cases["channels"] = (chan, "material 0: texture %d has 1 channels, expected 3" % chan[k].tex_opacity)
    for label, (table, msg) in cases.items():
        with pytest.raises(pta.PtError) as e:
            h.set_materials(table)
        assert e.value.code == pta.PT_ERR_INVALID and msg in str(e.value), label
    with pytest.raises(pta.PtError):
        h.set_materials(None, n=len(mats))
    assert [raw(m) for m in h.materials] == before
    ok = [pta.Material.from_buffer_copy(raw(m)) for m in mats]
    ok[0].opacity, ok[0].tex_opacity, ok[0].roughness = 1.0, -1, 0.25
    h.set_materials(ok)
    assert [raw(m) for m in h.materials] == [raw(m) for m in ok]


def test_keyframe_apply(pta, tmp_path):
    h = load(pta, "alpha_transparency")
    mats0 = h.materials
    n = len(mats0)
    frames = [{"materials": {"1": {"albedo": {"factor": [0.5, 0.25, 0.125]}}}},
              {"materials": {"1": {"roughness": {"factor": 0.5}}, str(n - 1): {"ior": 2.0}}},
              {"lights": [{"type": "Point", "position": [0, 3, 0], "color": [2, 2, 2], "size": 1}]},
              {"materials": {str(n): {"ior": 1.0}}}]
    kf = pta.load_keyframes(write(tmp_path, frames))
    h.apply_keyframe(kf[0])
    h.apply_keyframe(kf[1])
    m = h.materials
    assert list(m[1].albedo) == [0.5, 0.25, 0.125] and m[1].roughness == 0.5 and m[n - 1].ior == 2.0
    assert [raw(x) for i, x in enumerate(m) if i not in (1, n - 1)] == [raw(x) for i, x in enumerate(mats0) if i not in (1, n - 1)]
    h.apply_keyframe(kf[2])
    assert h.n_lights == 1 and list(h.lights[0].vec) == [0, 3, 0]
    state = ([raw(x) for x in h.materials], [raw(x) for x in h.lights])
    with pytest.raises(pta.PtError) as e:
        h.apply_keyframe(kf[3])
    assert e.value.code == pta.PT_ERR_INVALID and "out of range" in str(e.value)
    assert ([raw(x) for x in h.materials], [raw(x) for x in h.lights]) == state


def test_save_isf_round_trip_of_an_edited_scene(pta, tmp_path):
    h = load(pta, "alpha_transparency")
    lights = [point(pta, (0.5, 2.0, -1.0), (3, 2, 1)), directional(pta, (0.2, -1.0, 0.1), (0.5, 0.5, 0.5))]
    h.set_lights(lights)
    mats = [pta.Material.from_buffer_copy(raw(m)) for m in h.materials]
    mats[0].emissive[0], mats[0].metalness, mats[-1].opacity = 2.0, 0.5, 0.75
    h.set_materials(mats)
    h.save_isf(tmp_path)
    back = pta.HostScene.load_isf(tmp_path / "scene.isf")
    assert [raw(l) for l in back.lights] == [raw(l) for l in lights]
    got = [raw(m) for m in back.materials]
    assert got == [raw(m) for m in mats]


def test_ortho_grids_unchanged(pta):
    """The host half of k_og_ortho_extent: params_ortho, now axes + extent + parameters, gives the grids recorded from the
    builder before it was factored, for every golden scene's directional lights and a few more directions."""
    rec = json.loads((ROOT / "tests" / "golden" / "ortho_grids.json").read_text())
    assert sorted(rec) == GOLDEN
    for name in GOLDEN:
        h = load(pta, name)
        L = h.desc.contents.lights
        dirs = [[float(np.float32(-1.0) * np.float32(L[i].vec[k])) for k in range(3)] for i in range(h.n_lights)
                if L[i].kind == pta.PT_LIGHT_DIRECTIONAL]
        assert len(dirs) == rec[name]["n_directional"]
        for want in rec[name]["grids"]:
            g = pta.OriginGrid(h, direction=want["direction"], res=128)
            c = g.c
            assert int(c.enabled) == want["enabled"], name
            if c.enabled:
                assert (float(c.u0), float(c.v0), float(c.cells_per_unit)) == (want["u0"], want["v0"], want["cells_per_unit"]), name
                assert [float(x) for x in list(c.axis_u) + list(c.axis_v) + list(c.axis_w)] == want["axes"]
                assert (int(c.n_refs), int(c.n_global), int(c.max_cell_refs)) == (want["n_refs"], want["n_global"], want["max_cell_refs"])
                assert hashlib.sha256(g.cell_off.tobytes()).hexdigest() == want["cell_off_sha256"], name
                refs = np.stack([g.ref_prim, g.ref_mindist.view(np.uint32)], 1)
                assert hashlib.sha256(refs.tobytes()).hexdigest() == want["refs_sha256"], name
            g.close()
        assert dirs == [w["direction"] for w in rec[name]["grids"][:len(dirs)]]


def run_cli(*args):
    return subprocess.run([str(EXE), "render", *map(str, args)], capture_output=True, text=True, timeout=60)


@pytest.mark.parametrize("content, message", [
    ('{"camera": 1}', "expected an array of keyframes"),
    ("[]", "holds no frame"),
    ('[{"sun": 1}]', "unknown field `sun`"),
    ('[{"materials": {"99": {"ior": 1.5}}}]', "material 99 out of range"),
    ('[{}, {"materials": {"0": {"albedo": {"texture": "x.png"}}}}]', "cannot change a texture"),
])
def test_cli_keyframe_errors_before_gpu_work(tmp_path, content, message):
    frames = write(tmp_path, content)
    out = tmp_path / "f_%02d.png"
    r = run_cli(SCENES / "head" / "scene.isf", "--keyframes", frames, "-o", out, "-q")
    assert r.returncode == 2, r.stderr
    assert message in r.stderr
    assert not list(tmp_path.glob("*.png"))


def test_cli_keyframes_with_camera_path_is_an_error(tmp_path):
    frames = write(tmp_path, [{}])
    cams = write(tmp_path, [json.loads((SCENES / "head" / "scene.isf").read_text())["camera"]], "cams.json")
    r = run_cli(SCENES / "head" / "scene.isf", "--keyframes", frames, "--camera-path", cams, "-o", tmp_path / "f_%d.png", "-q")
    assert r.returncode == 2 and "cannot be used with" in r.stderr
    assert not list(tmp_path.glob("*.png"))


def test_cli_keyframes_need_a_frame_field(tmp_path):
    frames = write(tmp_path, [{}, {}])
    r = run_cli(SCENES / "head" / "scene.isf", "--keyframes", frames, "-o", tmp_path / "one.png", "-q")
    assert r.returncode == 2 and "has 2 frames" in r.stderr


def test_cli_help_names_keyframes():
    r = subprocess.run([str(EXE), "render", "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--keyframes <FRAMES>" in r.stdout


def test_make_light_orbit(pta, tmp_path):
    import sys
    out = tmp_path / "frames.json"
    r = subprocess.run([sys.executable, str(ROOT / "tools" / "make_light_orbit.py"), str(SCENES / "head" / "scene.isf"), "4",
                        "-o", str(out)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    kf = pta.load_keyframes(out)
    h = load(pta, "head")
    base = [raw(l) for l in h.lights]
    positions = []
    for i, f in enumerate(kf):
        h.apply_keyframe(f)
        assert h.n_lights == 2 and raw(h.lights[1]) == base[1]   # (the directional light stays)
        positions.append(np.array(list(h.lights[0].vec), np.float64))
    assert [raw(l) for l in pta.HostScene.load_isf(SCENES / "head" / "scene.isf").lights] == base
    assert np.allclose([p[1] for p in positions], positions[0][1])   # about the y axis: the height stays
    assert len({tuple(p) for p in positions}) == 4
