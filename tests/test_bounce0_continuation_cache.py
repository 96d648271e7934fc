"""The scene's cache of bounce-0 continuations (csrc/pt_gpu.hip pt_scene::cont_cache, csrc/pt_wavefront.h: the overloads of
k_wf_shade_hits with GRIDX | 1024 and | 2048).  In an opaque scene the direction the BRDF samples at the camera hit and the
throughput behind it are made from that hit, the material record there and words 2-3 of the item's ChaCha block - no light
enters - so they have the key of the bounce-1 hits.  Two planes of uint4 by work item keep their raw bits and a state word;
the frame that stores a view's bounce-1 hits stores them from the bounce-0 kernel it runs anyway (| 1024), and every later
launch that reads the bounce-1 hits itself loads them (| 2048) - a kernel without ct_sample and ct_eval_indirect.

What could go wrong: a record of one item read for another or of one plane for the other, a stale record after a material
edit or a camera move, a record read above the mark, beyond the budget or by another shard, a hit lane without a record (the
kernel counts those: `missing`, held to 0 here), a record lost across the rare shadow cast of a loading launch (the lanes
reload it), escape masks that arrive after the records were stored.  Every frame is compared bit for bit - f32 accumulator
and rgb8 - with the CPU oracle, and every test reads the cache's own numbers (GpuScene.cont_cache_stats): without them it
would prove nothing."""
import hashlib
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import scene_builder as sb
import test_bounce1_hit_cache as h1
from test_bounce0_four_waves import kernel_table
from test_bounce1_hit_cache import BOUNCES, H, SPP, W, open_case, open_want, shared
from test_prestaged_misses import CAMERA, assert_same, oracle_frame
from test_tail_bounce_caches import spheres_case

gpu = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent

NAMES = ("bytes", "items", "cached", "resets", "stores", "loads", "missing")
NONE = dict.fromkeys(NAMES, 0)
LOAD, LOAD_ORTHO = 11 | 32 | 64 | 128 | 2048, 15 | 32 | 64 | 128 | 2048
STORES = (11 | 16 | 1024, 15 | 16 | 1024, 11 | 32 | 64 | 1024, 15 | 32 | 64 | 1024)


@pytest.fixture(autouse=True)
def escape_answers_on(monkeypatch):
    """The tests here run both steps - the records, and the escape test's answer in them - whatever ships on."""
    monkeypatch.setenv("PT_CONT_ESCAPE", "1")


def stats(g):
    return dict(zip(NAMES, g.cont_cache_stats()))


def counts(st):
    return st["resets"], st["stores"], st["loads"]


def fused_launches(g):
    return g.hit1_fused_stats()[0]


def steady(g, prof, want, what, frames=6):
    """The frames of a fresh scene: plain, then the one that keys and zeroes the planes and stores them - the frame that stores
    the bounce-1 hits -, then the loading ones: one load per frame (the frame is one chunk), every launch that reads the
    bounce-1 hits itself."""
    for frame in range(frames):
        assert_same(g.render(prof), want, (what, frame))
        st = stats(g)
        print(what, frame, st)
        if frame == 0:
            assert st == NONE, (what, frame, st)
            continue
        assert st["bytes"] == 32 * st["items"] > 0 and st["cached"] == st["items"] == h1.stats(g)["items"], (what, frame, st)
        assert counts(st) == (1, 1, frame - 1) and st["missing"] == 0, (what, frame, st)
        assert h1.stats(g)["stores"] == 1 and fused_launches(g) == st["loads"], (what, frame, st)


def test_the_library_has_the_getter(pta):
    """No GPU: the symbol is there, a scene and seven uint64."""
    lib = pta.gpu_lib()
    assert "pt_get_cont_cache_stats" in pta.GPU_SYMBOLS
    args = lib.pt_get_cont_cache_stats.argtypes
    assert len(args) == 8 and args[0].__name__ == "c_void_p", args
    assert all(a._type_.__name__ == "c_ulong" for a in args[1:]), args


def test_the_variants_keep_the_budget_of_the_kernels_they_replace(tmp_path):
    """From the built library.  The loading variant: at most 128 vector registers, no scratch, LDS for four workgroups per CU
    (the variant with the orthographic branch: its base's 8 B of scratch).  The storing variants run once per view and
    material table: 128 registers and four workgroups, a few bytes of scratch allowed."""
    t = kernel_table(tmp_path)

    def one(gridx):
        k = [v for name, v in t.items() if f"k_wf_shade_hitsILi{gridx}EE" in name]
        assert len(k) == 1, (gridx, [name for name in t if "k_wf_shade_hits" in name])
        print(gridx, k[0])
        return k[0]

    k = one(LOAD)
    assert k["vgpr_count"] <= 128 and k["private_segment_fixed_size"] == 0 and k["group_segment_fixed_size"] <= 40960, k
    k = one(LOAD_ORTHO)
    assert k["vgpr_count"] <= 128 and k["private_segment_fixed_size"] <= 8 and k["group_segment_fixed_size"] <= 40960, k
    for gridx in STORES:
        k = one(gridx)
        assert k["vgpr_count"] <= 128 and k["private_segment_fixed_size"] <= 32 and k["group_segment_fixed_size"] <= 40960, (gridx, k)


@gpu
def test_the_runtime_places_four_workgroups_of_the_loading_variant_per_cu(pta):
    n = pta.kernel_occupancy(6)
    print("workgroups per CU:", n)
    assert n >= 4, n


@gpu
@pytest.mark.parametrize("name", ["open", "spheres"])
def test_six_steady_frames_and_the_switch(pta, oracle, scene_cache, monkeypatch, name):
    """Zeroed once, stored in the frame that stores the bounce-1 hits, loaded from the next frame on, no hit lane without a
    record.  PT_CONT_CACHE=0: the same images, nothing allocated, nothing counted."""
    if name == "open":
        _, scene, prof = open_case()
        want = open_want(oracle, scene, prof)
    else:
        scene, prof, want = spheres_case(pta, oracle, scene_cache, BOUNCES)
    g = pta.GpuScene(scene)
    steady(g, prof, want, name)
    g.close()
    monkeypatch.setenv("PT_CONT_CACHE", "0")
    g = pta.GpuScene(scene)
    for frame in range(6):
        assert_same(g.render(prof), want, (name, "off", frame))
        assert stats(g) == NONE, (name, frame, stats(g))
    assert fused_launches(g) == 4   # (the parent's kernel went on reading the bounce-1 hits)
    monkeypatch.delenv("PT_CONT_CACHE")
    for frame in range(3):   # switched on in mid-sequence: keyed at once, and - every chunk already loading its bounce-1 hits, no
        # launch that could store - nothing is stored and nothing loaded until the view is keyed again
        assert_same(g.render(prof), want, (name, "on again", frame))
        assert counts(stats(g)) == (1, 0, 0) and stats(g)["missing"] == 0, (name, frame, stats(g))
    g.close()


@gpu
def test_light_edits_keep_the_records(pta, oracle):
    """A recoloured light, a moved light: the records stay - no reset, no store - and every launch that reads the bounce-1 hits
    itself loads them (a moved light makes a new visibility key: its first frame has no such launch).  Another light count is a
    new view where the camera grid is rebuilt at another resolution; in this small scene it is not, so the records stay here
    too, and test_a_light_count_that_changes_the_camera_grid_starts_a_new_view forces the other case."""
    case, scene, prof = open_case()
    P = pta.PT_LIGHT_POINT
    cam = sb.make_camera(pta, **CAMERA)
    lights1 = sb.make_lights(pta, "point")
    recoloured = [sb._light(pta, P, tuple(lights1[0].vec), (20.0, 170.0, 90.0))]
    moved = [sb._light(pta, P, (-0.8, 2.9, 0.4), (20.0, 170.0, 90.0))]
    two = moved + [sb._light(pta, P, (-1.0, 3.0, 0.2), (60.0, 20.0, 90.0))]
    g = pta.GpuScene(scene)
    steady(g, prof, open_want(oracle, scene, prof), "start", frames=4)
    for what, lights in (("colour", recoloured), ("moved", moved), ("two", two), ("one", lights1)):
        before, res = stats(g), g.info().as_dict().get("cam_grid_res")
        g.set_lights(lights)
        rekeyed = g.info().as_dict().get("cam_grid_res") != res
        want = oracle_frame(oracle, sb.build(case, pta=pta, camera=cam, lights=lights), prof, walk=True)
        for frame in range(3):
            launches, loads = fused_launches(g), stats(g)["loads"]
            assert_same(g.render(prof), want, (what, frame))
            st = stats(g)
            print(what, frame, rekeyed, st)
            assert st["missing"] == 0 and st["loads"] - loads == fused_launches(g) - launches, (what, frame, st)
            if rekeyed:   # nothing, then zeroed and stored, then loaded
                assert counts(st) == (before["resets"] + (frame >= 1), before["stores"] + (frame >= 1), before["loads"] + (frame >= 2)), (what, frame, st, before)
            else:
                assert (st["resets"], st["stores"], st["cached"]) == (before["resets"], before["stores"], before["cached"]), (what, frame, st, before)
                if what == "colour":
                    assert st["loads"] == before["loads"] + 1 + frame, (what, frame, st, before)
        assert stats(g)["loads"] > before["loads"], (what, stats(g), before)
    g.close()


@gpu
def test_a_material_edit_rekeys(pta, oracle):
    """A table with other roughnesses gives other directions and throughputs - asserted on the CPU first, so that a stale
    record would show: the next frame neither loads nor stores, the one after zeroes and stores (from the kernel that loads
    camera hits and visibility), the third loads.  Back to the first table the same again."""
    case, scene, prof = open_case()
    cam = sb.make_camera(pta, **CAMERA)
    first_table = sb.case_materials(case, pta)
    other = sb.case_materials(case, pta)
    for m in other:
        m.roughness = min(1.0, 0.37 + 0.5 * m.roughness)
    first = open_want(oracle, scene, prof)
    want_other = shared(("cont", "other"), lambda: oracle_frame(oracle, sb.build(case, pta=pta, camera=cam, materials=other), prof, walk=True))
    assert not np.array_equal(first[1], want_other[1])
    g = pta.GpuScene(scene)
    steady(g, prof, first, "start", frames=4)
    resets, stores, loads = 1, 1, 2
    for what, table, want in (("other", other, want_other), ("first again", first_table, first)):
        g.set_materials(table)
        for frame, (dr, ds, dl) in enumerate([(0, 0, 0), (1, 1, 0), (0, 0, 1), (0, 0, 1)]):
            assert_same(g.render(prof), want, (what, frame))
            resets, stores, loads = resets + dr, stores + ds, loads + dl
            st = stats(g)
            assert counts(st) == (resets, stores, loads) and st["missing"] == 0, (what, frame, st)
    g.close()


@gpu
def test_a_camera_move_and_back_and_translucent_frames(pta, oracle):
    """A camera move starts an empty prefix in the same allocation: nothing, stored, loaded - and the same on the way back.  The
    frames of a translucent table leave the records and the numbers alone; the opaque table set again is a new material
    generation, as for the bounce-1 hits: nothing, stored, loaded."""
    case, scene, prof = open_case()
    cam1 = sb.make_camera(pta, **CAMERA)
    cam2 = sb.make_camera(pta, eye=(-0.9, 2.1, 2.9), target=(0.3, 0.3, -0.4), fov=0.8)
    opaque = sb.case_materials(case, pta)
    alpha = sb.case_materials(case._replace(factor_set="alpha"), pta)
    first = open_want(oracle, scene, prof)
    want2 = shared(("cont", "cam2"), lambda: oracle_frame(oracle, sb.build(case, pta=pta, camera=cam2), prof, walk=True))
    alpha_scene = sb.build(case, pta=pta, camera=cam1, materials=alpha)
    assert alpha_scene.translucent
    want_alpha = oracle_frame(oracle, alpha_scene, prof, walk=True)
    g = pta.GpuScene(scene)
    steady(g, prof, first, "start", frames=4)
    resets, stores, loads = 1, 1, 2
    for what, cam, want in (("moved", cam2, want2), ("back", cam1, first)):
        g.set_camera(cam)
        for frame, (dr, ds, dl) in enumerate([(0, 0, 0), (1, 1, 0), (0, 0, 1)]):
            assert_same(g.render(prof), want, (what, frame))
            resets, stores, loads = resets + dr, stores + ds, loads + dl
            st = stats(g)
            assert counts(st) == (resets, stores, loads) and st["missing"] == 0, (what, frame, st)
            assert st["cached"] == (0 if frame == 0 else st["items"]), (what, frame, st)
    before = stats(g)
    g.set_materials(alpha)
    for frame in range(2):
        assert_same(g.render(prof), want_alpha, ("translucent", frame))
        assert stats(g) == before, (frame, stats(g), before)
    g.set_materials(opaque)
    for frame, (dr, ds, dl) in enumerate([(0, 0, 0), (1, 1, 0), (1, 1, 1)]):
        assert_same(g.render(prof), first, ("opaque again", frame))
        st = stats(g)
        assert counts(st) == (before["resets"] + dr, before["stores"] + ds, before["loads"] + dl) and st["missing"] == 0, (frame, st)
    g.close()


@gpu
def test_shards(pta, oracle):
    """Ranks 0 and 1 of 2 with 32 x 32 tiles, a scene and two planes each: each rank's pixels are the unsharded frame's."""
    case, scene = h1.open_scene("point", BOUNCES)
    prof = sb.profile(case, 160, 96, SPP)
    want = shared(("children", "open"), lambda: oracle_frame(oracle, scene, prof))
    rgb, acc = np.zeros_like(want[0]), np.zeros_like(want[1])
    for r in range(2):
        o = pta.Opts.make(shard_rank=r, shard_count=2, tile_w=32, tile_h=32)
        m = pta.local_pixel_map(prof, o)
        g = pta.GpuScene(scene)
        for frame in range(4):
            rgb[m], acc[m] = g.render(prof, o)
        st = stats(g)
        assert st["items"] == st["cached"] >= len(m) * SPP and counts(st) == (1, 1, 2) and st["missing"] == 0, (r, st)
        g.close()
    assert_same((rgb, acc), want, "assembled")


@gpu
def test_one_bounce(pta, oracle):
    """bounces = 1: the ray that is loaded is the path's last."""
    case, scene = h1.open_scene("point", 1)
    prof = sb.profile(case, W, H, SPP)
    want = shared(("cont", "one bounce"), lambda: oracle_frame(oracle, scene, prof))
    g = pta.GpuScene(scene)
    steady(g, prof, want, "one bounce", frames=4)
    g.close()


# Switches that are read once per process or per scene: one child per setting.  A child renders `open` and `spheres` at
# 64 x 48 x 4, eight frames each, and prints a hash of every frame, the cache's numbers, the launches that read the bounce-1
# hits themselves and whether the scene has escape masks by then (the time their build took: `open`'s prove no miss, so the
# count of primitives with a clear bit stays 0 there).
CHILD = r"""
import hashlib, json, sys
import numpy as np
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(root)r + "/tests")
import __graft_entry__ as e
import scene_builder as sb
from test_prestaged_misses import open_scene
pta = e.load_package()
case, scene = open_scene("point", 5)
cases = {"open": (scene, sb.profile(case, 64, 48, 4)),
         "spheres": (pta.HostScene.load_isf(%(root)r + "/tests/golden/scenes/spheres/scene.isf"), pta.Profile.make(64, 48, 4, 5))}
res = {}
for name, (scene, prof) in cases.items():
    g = pta.GpuScene(scene)
    out = []
    for frame in range(8):
        rgb, acc = g.render(prof)
        sha = hashlib.sha1(np.ascontiguousarray(rgb, np.uint8).tobytes() + np.ascontiguousarray(acc, np.float32).tobytes()).hexdigest()
        out.append([sha, [int(v) for v in g.cont_cache_stats()], int(g.hit1_fused_stats()[0]), float(g.info().as_dict()["escape_build_seconds"]) > 0.0])
    g.close()
    res[name] = out
print("RESULT", json.dumps(res))
"""
# 16 384 items a frame (32 x 32 tiles: 64 x 64 x 4).  Chunks of 4 096 and room for 8 384 records: the first two chunks are
# stored and loaded, the other two run the parent's kernel.
# (PT_CONT_ESCAPE=1 everywhere but in its own case: the tests run the recorded escape answers whatever ships on)
SETTINGS = {
    "chunks": {"PT_WF_CHUNK": "4096"},
    "chunks-half-budget": {"PT_WF_CHUNK": "4096", "PT_CONT_CACHE_GIB": "0.00025"},
    "masks-before-the-store": {"PT_ESCAPE_AFTER": "0"},
    "masks-after-the-store": {"PT_ESCAPE_AFTER": "5"},
    "no-masks": {"PT_ESCAPE": "0"},
    "escape-answers-off": {"PT_ESCAPE_AFTER": "0", "PT_CONT_ESCAPE": "0"},
}


def sha_of(frame):
    return hashlib.sha1(np.ascontiguousarray(frame[0], np.uint8).tobytes() + np.ascontiguousarray(frame[1], np.float32).tobytes()).hexdigest()


@gpu
@pytest.mark.parametrize("setting", list(SETTINGS))
def test_chunks_a_partial_budget_and_escape_masks_that_come_late_or_never(pta, oracle, scene_cache, setting):
    """Several chunks: the planes grow as a prefix over them and every chunk loads; with room for about half of the items the
    chunks of the prefix load and the rest runs the parent's kernel.  PT_ESCAPE_AFTER=5: the masks are built after the records were
    stored - the mask generation differs, and the loading kernel evaluates the escape test itself, on the loaded ray.
    PT_ESCAPE_AFTER=0: the masks exist when the records are stored, so the loading launches take the recorded answers - and with
    PT_CONT_ESCAPE=0 they do not.  PT_ESCAPE=0: no masks at all."""
    _, scene, prof = open_case()
    want = {"open": sha_of(open_want(oracle, scene, prof)), "spheres": sha_of(spheres_case(pta, oracle, scene_cache, BOUNCES)[2])}
    env = {k: v for k, v in os.environ.items() if not k.startswith(("PT_WF_", "PT_CONT_", "PT_ESCAPE"))}
    env.update({"PT_CONT_ESCAPE": "1"}, **SETTINGS[setting])
    run = subprocess.run([sys.executable, "-c", CHILD % {"root": str(ROOT)}], env=env, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, (setting, run.stderr[-2000:])
    res = json.loads([ln for ln in run.stdout.splitlines() if ln.startswith("RESULT ")][0][7:])
    for name, frames in res.items():
        print(setting, name, frames)
        for frame, (sha, st, launches, masks) in enumerate(frames):
            st = dict(zip(NAMES, st))
            assert sha == want[name], (setting, name, frame, st)
            assert st["missing"] == 0, (setting, name, frame, st)
            if frame == 0:
                assert st == NONE, (setting, name, st)
                continue
            assert st["resets"] == 1 and st["stores"] >= 1, (setting, name, frame, st)
            if setting == "chunks":
                assert st["cached"] == st["items"] == 64 * 64 * SPP and st["stores"] >= 2 and st["loads"] == launches == st["stores"] * (frame - 1), (name, frame, st, launches)
            elif setting == "chunks-half-budget":
                assert 0 < st["cached"] <= 8384 and st["cached"] % 64 == 0 and st["bytes"] <= 0.00025 * 2 ** 30, (name, frame, st)
                assert st["loads"] == st["stores"] * (frame - 1) and (frame < 2 or st["loads"] < launches), (name, frame, st, launches)
            else:
                assert counts(st) == (1, 1, frame - 1) and st["loads"] == launches, (setting, name, frame, st, launches)
            if setting == "no-masks":
                assert not masks, (name, frame)
        if setting == "masks-after-the-store":   # (the premise: stored without masks, loaded with them)
            assert [f[3] for f in frames] == [False] * 5 + [True] * 3, (name, [f[3] for f in frames])
        if setting in ("masks-before-the-store", "escape-answers-off"):   # (the premise: stored with the masks the loads run under)
            assert all(f[3] for f in frames), (name, [f[3] for f in frames])


# A light count that changes the camera grid's resolution is a new view.  The resolution rule and the grids' budget are read
# once per process: with PT_OG_RES=2048 and room for two grids of that size, a second light (three grids) halves the
# resolution.  The child renders `open` with one light, then with two, and prints the resolutions and the cache's numbers.
CHILD_LIGHTS = r"""
import hashlib, json, sys
import numpy as np
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(root)r + "/tests")
import __graft_entry__ as e
import scene_builder as sb
from test_prestaged_misses import open_scene
pta = e.load_package()
case, scene = open_scene("point", 5)
prof = sb.profile(case, 64, 48, 4)
g = pta.GpuScene(scene)
out, res = [], [g.info().as_dict()["cam_grid_res"]]
def frames(n):
    for frame in range(n):
        rgb, acc = g.render(prof)
        sha = hashlib.sha1(np.ascontiguousarray(rgb, np.uint8).tobytes() + np.ascontiguousarray(acc, np.float32).tobytes()).hexdigest()
        out.append([sha, [int(v) for v in g.cont_cache_stats()]])
frames(4)
P = pta.PT_LIGHT_POINT
g.set_lights([sb._light(pta, P, (-0.8, 2.9, 0.4), (20.0, 170.0, 90.0)), sb._light(pta, P, (-1.0, 3.0, 0.2), (60.0, 20.0, 90.0))])
res.append(g.info().as_dict()["cam_grid_res"])
frames(3)
g.close()
print("RESULT", json.dumps({"frames": out, "res": res}))
"""


@gpu
def test_a_light_count_that_changes_the_camera_grid_starts_a_new_view(pta, oracle):
    """One light, then two: the camera grid is rebuilt at half the resolution, which is part of the key - the frame after the
    edit neither loads nor stores, the next zeroes and stores, the third loads; all three are the oracle's for two lights."""
    case, scene, prof = open_case()
    P = pta.PT_LIGHT_POINT
    two = [sb._light(pta, P, (-0.8, 2.9, 0.4), (20.0, 170.0, 90.0)), sb._light(pta, P, (-1.0, 3.0, 0.2), (60.0, 20.0, 90.0))]
    first = sha_of(open_want(oracle, scene, prof))
    want = sha_of(oracle_frame(oracle, sb.build(case, pta=pta, camera=sb.make_camera(pta, **CAMERA), lights=two), prof, walk=True))
    assert want != first
    env = {k: v for k, v in os.environ.items() if not k.startswith(("PT_WF_", "PT_CONT_", "PT_ESCAPE", "PT_OG_"))}
    env.update(PT_CONT_ESCAPE="1", PT_OG_RES="2048", PT_OG_BUDGET_GIB="0.6")
    run = subprocess.run([sys.executable, "-c", CHILD_LIGHTS % {"root": str(ROOT)}], env=env, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    out = json.loads([ln for ln in run.stdout.splitlines() if ln.startswith("RESULT ")][0][7:])
    print(out)
    assert out["res"] == [2048, 1024], out["res"]
    got = [(sha, counts(dict(zip(NAMES, st))), dict(zip(NAMES, st))["missing"]) for sha, st in out["frames"]]
    assert [g[0] for g in got] == [first] * 4 + [want] * 3, [g[0] for g in got]
    assert [g[1] for g in got] == [(0, 0, 0), (1, 1, 0), (1, 1, 1), (1, 1, 2), (1, 1, 2), (2, 2, 2), (2, 2, 3)], [g[1] for g in got]
    assert all(g[2] == 0 for g in got)
