"""The bookkeeping of a scene's origin grids through edits: what pt_scene_get_info reports - device_bytes,
grid_refs, light_grids, cam_grid_res - and the grids themselves are, after any sequence of pt_scene_set_camera /
pt_scene_set_lights, those of a scene created from the edited description.  Pins the branches the other edit tests do not
reach: a byte budget under which the light count decides the camera grid's resolution (PT_OG_BUDGET_GIB), edits of a scene
whose grids the host built (PT_OG_HOST=1), device_bytes after a light edit.

The variables are process-static: one child process per setting, as in test_gpu_options.py."""
import json
import os
import subprocess
import sys
from pathlib import Path

import pytest

from test_camera_update import cameras, grid_bytes
from test_scene_edits import assert_grids_equal, fresh, light_edits, load

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
FACTS = ("device_bytes", "grid_refs", "light_grids", "cam_grid_res")


def facts(scene, names=FACTS):
    i = scene.info()
    return {k: int(getattr(i, k)) for k in names}


@pytest.mark.parametrize("name", ["cube", "ps5"])
def test_round_trip_restores_every_grid_fact(pta, name):
    # (no render anywhere: the escape masks never enter the byte count)
    host = load(pta, name)
    g = pta.GpuScene(host)
    lights0, cam0 = host.lights, host.camera
    edits = light_edits(pta, host)
    orbit = cameras(pta, host)["orbit"]
    facts0 = facts(g)
    grids0 = [pta.OriginGrid.from_device(g, k) for k in range(len(lights0) + 2)]
    assert grids0[0].enabled and not grids0[-1].enabled

    def set_lights(label, lights, cam):
        g.set_lights(lights)
        h = load(pta, name)
        h.set_lights(lights)
        if cam is not None:
            h.set_camera(cam)
        ref = pta.GpuScene(h)
        # (a fresh scene's entry lists depend on the camera position: device_bytes only while the camera is the first one)
        names = FACTS if cam is None else FACTS[1:]
        assert facts(g, names) == facts(ref, names), (name, label)
        for k in range(len(lights) + 2):
            assert_grids_equal(pta.OriginGrid.from_device(g, k), pta.OriginGrid.from_device(ref, k), (name, label, k))
        ref.close()

    def set_camera(label, cam):
        before, old = g.info().device_bytes, pta.OriginGrid.from_device(g, 0)
        g.set_camera(cam)
        got = pta.OriginGrid.from_device(g, 0)
        assert g.info().device_bytes - before == grid_bytes(got) - grid_bytes(old), (name, label)

    set_lights("added", edits["added"], None)
    set_camera("orbit", orbit)
    set_lights("none", edits["none"], orbit)
    set_lights("rejected", edits["rejected"], orbit)
    assert g.info().light_grids == 0
    set_lights("original lights", lights0, orbit)
    set_camera("original camera", cam0)
    assert facts(g) == facts0, name
    for k, want in enumerate(grids0):
        assert_grids_equal(pta.OriginGrid.from_device(g, k), want, (name, "round trip", k))


CHILD_HEAD = r"""
import json, os, sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
import numpy as np
import __graft_entry__ as e
pta = e.load_package()
from test_camera_update import cameras
from test_scene_edits import assert_grids_equal, light_edits, load, same
FACTS = ("device_bytes", "grid_refs", "light_grids", "cam_grid_res")

def facts(scene, names=FACTS):
    i = scene.info()
    return {k: int(getattr(i, k)) for k in names}

def fresh(name, lights=None, cam=None):
    h = load(pta, name)
    if lights is not None:
        h.set_lights(lights)
    if cam is not None:
        h.set_camera(cam)
    return h, pta.GpuScene(h)

prof = pta.Profile.make(160, 120, 4, 3)
"""

# PT_OG_BUDGET_GIB=0.15 (161.06 MB) on the 30 000-triangle scene (auto resolution 1024, estimate 60 res^2 bytes a grid):
# one light: 2 x 62.9 MB fits - camera grid 1024, 1 light grid; two lights: 3 x 62.9 MB does not, 3 x 15.7 MB at 512 does -
# camera grid 512, 2 light grids: pt_scene_set_lights rebuilds the camera grid.
CHILD_BUDGET = CHILD_HEAD + r"""
host = load(pta, "ps5")
g = pta.GpuScene(host)
edits = light_edits(pta, host)
out = []
for step, (label, lights) in enumerate((("base", host.lights), ("added", edits["added"]), ("none", edits["none"]), ("base", host.lights))):
    if step:
        g.set_lights(lights)
    _, ref = fresh("ps5", lights=lights)
    for k in range(len(lights) + 2):
        assert_grids_equal(pta.OriginGrid.from_device(g, k), pta.OriginGrid.from_device(ref, k), (step, label, k))
    assert pta.OriginGrid.from_device(g, 0).enabled
    assert same(g.render(prof), ref.render(prof)), (step, label)
    # (after the frames: both scenes have built their escape masks)
    print("FACTS", step, label, facts(g), facts(ref), flush=True)
    assert facts(g) == facts(ref), (step, label)
    out.append([facts(g)["cam_grid_res"], facts(g)["light_grids"]])
    ref.close()
print("SEQ", json.dumps(out))
"""

# PT_OG_HOST=1: the host builds the grids of a fresh scene; a moved camera and edited lights go without.
# %(og0)s: device_bytes of a fresh scene of every name under PT_OG=0 - the scene without any grid.
CHILD_HOST = CHILD_HEAD + r"""
og0 = json.loads(%(og0)r)
up = lambda n: max(16, n)   # (bytes of one uploaded array)
for name in ("cube", "ps5"):
    host = load(pta, name)
    lights0, orbit = host.lights, cameras(pta, host)["orbit"]
    added = light_edits(pta, host)["added"]
    # ---- the bookkeeping, without a frame (no escape masks in the byte count)
    g = pta.GpuScene(host)
    f0 = facts(g)
    assert f0["cam_grid_res"] > 0 and f0["light_grids"] == len(lights0), (name, f0)
    for k in (0, 1):
        assert not pta.OriginGrid.from_device(g, k).enabled, (name, k)
    t = list(host.camera.transform)
    fro = float(np.sqrt(sum(float(t[4 * k + r]) ** 2 for k in range(3) for r in range(3))))
    hg = pta.OriginGrid(host, origin=t[12:15], res=f0["cam_grid_res"], ray_offset=0.0, max_dir_len=np.float32(fro * 1.001))
    cam_rise = up(4 * (int(hg.c.n_cells) + 1)) + up(8 * max(1, hg.n_refs))   # (what uploading the camera grid added)
    g.set_camera(orbit)
    f1 = facts(g)
    print("HOST", name, "fresh", f0, "camera", f1, "cam_rise", cam_rise, "og0", og0[name], flush=True)
    assert f1["cam_grid_res"] == 0 and f1["light_grids"] == f0["light_grids"], (name, f1)
    assert f0["device_bytes"] - f1["device_bytes"] == cam_rise and f1["device_bytes"] < f0["device_bytes"], (name, f0, f1)
    assert f0["grid_refs"] - f1["grid_refs"] == hg.n_refs, (name, f0, f1)
    g.set_lights(added)
    f2 = facts(g)
    assert f2["light_grids"] == 0 and f2["grid_refs"] == 0 and f2["cam_grid_res"] == 0, (name, f2)
    g.set_lights(lights0)
    f3 = facts(g)
    print("HOST", name, "lights", f2, "original lights", f3, flush=True)
    # every grid gone, the tables those of the first lights: the bytes of the scene without grids - device_bytes has dropped
    # by exactly what it rose by when the grids were uploaded
    assert f3 == dict(device_bytes=og0[name], grid_refs=0, light_grids=0, cam_grid_res=0), (name, f3, og0[name])
    for k in (0, 1):
        assert not pta.OriginGrid.from_device(g, k).enabled, (name, k)
    g.close()
    # ---- the frames: before and after each edit those of a fresh scene of the edited description
    g = pta.GpuScene(host)
    for label, lights, cam in (("fresh", None, None), ("camera", None, orbit), ("lights", added, orbit)):
        if label == "camera":
            g.set_camera(cam)
        if label == "lights":
            g.set_lights(lights)
        _, ref = fresh(name, lights=lights, cam=cam)
        assert same(g.render(prof), ref.render(prof)), (name, label)
        ref.close()
    assert facts(g)["cam_grid_res"] == 0 and facts(g)["light_grids"] == 0
print("HOST done")
"""

CHILD_OG0 = CHILD_HEAD + r"""
print("OG0", json.dumps({name: facts(fresh(name)[1])["device_bytes"] for name in ("cube", "ps5")}))
"""


def run_child(code, extra, **fmt):
    env = dict(os.environ)
    for k in list(env):
        if k.startswith(("PT_WF_", "PT_OG", "PT_SHADE_", "PT_TILE_", "PT_KD_", "PT_CAM_", "PT_ESCAPE")):
            del env[k]
    env["PT_ESCAPE_AFTER"] = "0"   # (as the suite: the masked pipeline from frame one, in the edited and the fresh scene alike)
    env.update(extra)
    code = code % dict(root=str(ROOT), tests=str(ROOT / "tests"), **fmt)
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (extra, out.stdout[-3000:], out.stderr[-3000:])
    return out.stdout


def tagged(stdout, tag):
    lines = [ln for ln in stdout.splitlines() if ln.startswith(tag + " ")]
    assert len(lines) == 1, stdout[-2000:]
    return json.loads(lines[0][len(tag) + 1:])


def test_budget_makes_a_light_edit_rebuild_the_camera_grid():
    out = run_child(CHILD_BUDGET, {"PT_OG_BUDGET_GIB": "0.15"})
    # [cam_grid_res, light_grids] of base, added, none, base
    assert tagged(out, "SEQ") == [[1024, 1], [512, 2], [1024, 0], [1024, 1]], out[-3000:]


def test_edits_of_a_scene_with_host_built_grids():
    og0 = tagged(run_child(CHILD_OG0, {"PT_OG": "0"}), "OG0")
    out = run_child(CHILD_HOST, {"PT_OG_HOST": "1"}, og0=json.dumps(og0))
    assert "HOST done" in out, out[-3000:]
