"""The bounce-0 kernel that reads the bounce-1 hit cache itself (csrc/pt_wavefront.h, the third k_wf_shade_hits: GRIDX | 128;
csrc/pt_gpu.hip Chunk::hit1_fused).  In a chunk that loads its camera hits, its shadow visibility and its bounce-1 hits, the
kernel that makes the bounce-1 ray looks the ray's hit up where it is made: a survivor whose record says miss, with a
colour that is final, ends there - what wf_prestage_miss stages is its sample - and takes no queue record; every other
survivor gets its record and, at the same queue position, the hit word and (key, u, v) k_wf_hits_load would have copied,
or - an item without a record - an entry of bounce 1's exact list.  k_wf_hits_load is not launched for such a chunk.

What could go wrong: a path elided whose colour the shadow kernel still had to patch, a staged value that is not the one
the parent's kernels leave, a hit written beside its record, an item without a record taken for a miss or a hit, a frame
plan counted in an eliding frame whose queue 1 is too short for a frame that casts (or whose bounce 1 went inline because
its queue held hits only), a storing frame that elides, a chunk above the cache's mark that takes the variant.  Every frame
here is compared bit for bit - rgb8 and f32 accumulator - with the CPU oracle or with a render that has the switch or the
caches off, and every test reads the variant's own numbers (GpuScene.hit1_fused_stats): without them it would prove
nothing."""
import numpy as np
import pytest

import scene_builder as sb
import test_bounce1_hit_cache as h1
from test_bounce1_hit_cache import BOUNCES, H, SPP, W, open_case, open_want, shared
from test_kernel_resources import kernel_table
from test_prestaged_misses import CAMERA, assert_same, open_scene, oracle_frame

gpu = pytest.mark.gpu

NAMES = ("launches", "written", "elided", "unknown")


def fused(g):
    return dict(zip(NAMES, g.hit1_fused_stats()))


def records(st):
    """What a frame that casts writes to queue 1."""
    return st["written"] + st["elided"] + st["unknown"]


def delta(after, before):
    return {k: after[k] - before[k] for k in NAMES}


def steady(g, prof, want, what, frames=5, unknown=False):
    """The frames of a fresh scene: plain, storing, then the loading ones - one launch of the variant and one load each, and
    the same records every frame.  Returns one loading frame's numbers."""
    per_frame, before = None, fused(g)
    for frame in range(frames):
        assert_same(g.render(prof), want, (what, frame))
        st, c = fused(g), h1.stats(g)
        assert st["launches"] == max(0, frame - 1) and c["loads"] == max(0, frame - 1), (what, frame, st, c)
        d = delta(st, before)
        before = st
        if frame < 2:   # (a storing frame never elides)
            assert d == dict.fromkeys(NAMES, 0), (what, frame, d)
            continue
        assert (d["unknown"] > 0) == unknown and c["unknown"] == st["unknown"], (what, frame, d, c)
        if per_frame is None:
            per_frame = d
        assert d == per_frame, (what, frame, d, per_frame)
    return per_frame


@gpu
@pytest.mark.parametrize("name", ["spheres", "cube", "reflection", "open"])
def test_consecutive_frames(pta, oracle, scene_cache, name):
    """From the third frame on: one launch of the variant per frame, the loads as before, the same written + elided + unknown
    every frame and no more than the frame has items.  open: rays leave under a sky that is not black - paths are elided -
    and the survivors behind its long normals, which the shadow kernel patches, keep their records."""
    if name == "open":
        _, scene, prof = open_case()
        want = open_want(oracle, scene, prof)
    else:
        scene = scene_cache(name)
        prof = pta.Profile.make(W, H, SPP, 3)
        want = shared(("steady", name), lambda: oracle_frame(oracle, scene, prof))
    g = pta.GpuScene(scene)
    d = steady(g, prof, want, name)
    print(name, d)
    assert 0 < records(d) <= W * H * SPP, d
    if name == "open":
        assert d["elided"] > 0 and d["written"] > 0, d
    g.close()


@gpu
def test_a_directional_light_takes_the_variant_with_the_orthographic_branch(pta, oracle):
    """A point and a directional light: the kernel with the orthographic grid branch (GRIDX 15 | 32 | 64 | 128), which keeps the
    record's word alone and reads the rest of a hit's record again where it writes it."""
    case = sb.Case("fused-point-dir", "open", "none", "point_dir", "opaque", BOUNCES, "FILMIC", 0, False)
    scene = sb.build(case, camera=sb.make_camera(pta, **CAMERA))
    assert any(l.kind == pta.PT_LIGHT_DIRECTIONAL for l in sb.make_lights(pta, "point_dir"))
    prof = sb.profile(case, W, H, SPP)
    want = oracle_frame(oracle, scene, prof, walk=True)
    g = pta.GpuScene(scene)
    d = steady(g, prof, want, "point_dir")
    assert d["written"] > 0 and d["elided"] > 0, d
    g.close()


@gpu
def test_holes(pta, oracle, monkeypatch):
    """PT_HIT1_CACHE_HOLES=3: every third item has no record - its survivor keeps its queue record, is listed for the exact
    walker and counted, the same count every frame - and the frame is the oracle's.  The records of a frame are those of a
    frame without holes."""
    _, scene, prof = open_case()
    want = open_want(oracle, scene, prof)
    g = pta.GpuScene(scene)
    whole = steady(g, prof, want, "whole", frames=3)
    g.close()
    monkeypatch.setenv("PT_HIT1_CACHE_HOLES", "3")
    g = pta.GpuScene(scene)
    d = steady(g, prof, want, "holes", unknown=True)
    assert records(d) == records(whole) and d["elided"] < whole["elided"], (d, whole)
    g.close()


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
prof = sb.profile(case, 160, 96, 4)
g = pta.GpuScene(scene)
out = []
for frame in range(5):
    rgb, acc = g.render(prof)
    sha = hashlib.sha1(np.ascontiguousarray(rgb, np.uint8).tobytes() + np.ascontiguousarray(acc, np.float32).tobytes()).hexdigest()
    out.append([sha, [int(v) for v in g.hit1_cache_stats()], [int(v) for v in g.hit1_fused_stats()]])
print("RESULT", json.dumps({"frames": out}))
"""


@gpu
@pytest.mark.parametrize("setting", h1.SETTINGS, ids=lambda s: "-".join(f"{k[6:]}{v}" for k, v in s.items()) or "default")
def test_holes_with_the_shade_pass_split_or_not_and_both_exact_modes(oracle, setting):
    """The pipeline's switches are read once per process: one child per setting of test_bounce1_hit_cache.SETTINGS, the open
    scene at 160 x 96 with every third record left out.  Whatever the setting does at the other bounces, bounce 1 of the
    loading frames walks the variant's list alone and shades the queue in one pass."""
    import hashlib
    import json
    import os
    import subprocess
    import sys
    from pathlib import Path
    root = Path(__file__).resolve().parent.parent
    case, scene = open_scene("point", BOUNCES)
    want = shared(("children", "open"), lambda: oracle_frame(oracle, scene, sb.profile(case, 160, 96, SPP)))
    want_sha = hashlib.sha1(np.ascontiguousarray(want[0], np.uint8).tobytes() + np.ascontiguousarray(want[1], np.float32).tobytes()).hexdigest()
    env = {k: v for k, v in os.environ.items() if not k.startswith(("PT_WF_", "PT_HIT1_"))}
    env.update(setting, PT_HIT1_CACHE_HOLES="3")
    run = subprocess.run([sys.executable, "-c", CHILD % {"root": str(root)}], env=env, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, (setting, run.stderr[-2000:])
    res = json.loads([ln for ln in run.stdout.splitlines() if ln.startswith("RESULT ")][0][7:])
    print(setting, res)
    per_frame = None
    for frame, (sha, cache, st) in enumerate(res["frames"]):
        cache, st = dict(zip(h1.NAMES, cache)), dict(zip(NAMES, st))
        assert sha == want_sha, (setting, frame, cache, st)
        assert st["launches"] == cache["loads"] == max(0, frame - 1) and st["unknown"] == cache["unknown"], (setting, frame, cache, st)
        if frame >= 2:
            per_frame = per_frame or st
            assert st["unknown"] == per_frame["unknown"] * (frame - 1) > 0, (setting, frame, st)
            assert records(st) == records(per_frame) * (frame - 1), (setting, frame, st)


@gpu
def test_edits(pta, oracle):
    """Light moved, recoloured, counts 1 -> 2 -> 1: the variant goes on (a camera grid rebuilt at another resolution with the
    count re-keys: then it resumes with the loads).  Five lights: no visibility plane - the frames load through
    k_wf_hits_load and the variant's count stands still.  A material edit and a camera move re-key: no launch of the
    variant until the plane is stored again.  A translucent table never takes it."""
    case, scene, prof = open_case()
    P = pta.PT_LIGHT_POINT
    cam = sb.make_camera(pta, **CAMERA)
    cam2 = sb.make_camera(pta, eye=(-0.9, 2.1, 2.9), target=(0.3, 0.3, -0.4), fov=0.8)
    lights1 = sb.make_lights(pta, "point")
    recoloured = [sb._light(pta, P, tuple(lights1[0].vec), (20.0, 170.0, 90.0))]
    moved = [sb._light(pta, P, (-0.8, 2.9, 0.4), (20.0, 170.0, 90.0))]
    two = moved + [sb._light(pta, P, (-1.0, 3.0, 0.2), (60.0, 20.0, 90.0))]
    five = sb.make_lights(pta, "five")
    assert len(five) > 4
    opaque = sb.case_materials(case, pta)
    other = sb.case_materials(case, pta)
    for m in other:
        m.roughness = min(1.0, 0.37 + 0.5 * m.roughness)
    alpha = sb.case_materials(case._replace(factor_set="alpha"), pta)
    g = pta.GpuScene(scene)
    steady(g, prof, open_want(oracle, scene, prof), "start", frames=4)

    def frames(what, want, n):
        """n frames, each the oracle's: the launches of the variant and the cache's loads they added, frame by frame."""
        out = []
        for frame in range(n):
            before, loads = fused(g), h1.stats(g)["loads"]
            assert_same(g.render(prof), want, (what, frame))
            out.append((fused(g)["launches"] - before["launches"], h1.stats(g)["loads"] - loads))
        return out

    for what, lights in (("colour", recoloured), ("moved", moved), ("two", two), ("one", lights1)):
        res = g.info().as_dict().get("cam_grid_res")
        g.set_lights(lights)
        rekeyed = g.info().as_dict().get("cam_grid_res") != res
        want = oracle_frame(oracle, sb.build(case, pta=pta, camera=cam, lights=lights), prof, walk=True)
        got = frames(what, want, 3)
        # (a moved light or a new count makes a new visibility key: its plane is zeroed one frame later, and a frame
        # without the plane loads through k_wf_hits_load)
        assert got[2] == (1, 1) and all(l == 1 for _, l in got[0 if not rekeyed else 2:]), (what, rekeyed, got)
        assert all(n <= l for n, l in got), (what, got)
    g.set_lights(five)
    want = oracle_frame(oracle, sb.build(case, pta=pta, camera=cam, lights=five), prof, walk=True)
    got = frames("five", want, 4)
    assert all(n == 0 for n, _ in got) and got[2][1] == got[3][1] == 1, got
    g.set_lights(lights1)
    want1 = open_want(oracle, scene, prof)
    frames("one again", want1, 3)
    assert frames("one again, keyed", want1, 1) == [(1, 1)]
    g.set_materials(other)
    want = oracle_frame(oracle, sb.build(case, pta=pta, camera=cam, materials=other), prof, walk=True)
    assert frames("materials", want, 3) == [(0, 0), (0, 0), (1, 1)]
    g.set_camera(cam2)
    want = oracle_frame(oracle, sb.build(case, pta=pta, camera=cam2, materials=other), prof, walk=True)
    assert frames("camera", want, 3) == [(0, 0), (0, 0), (1, 1)]
    g.set_materials(alpha)
    want = oracle_frame(oracle, sb.build(case, pta=pta, camera=cam2, materials=alpha), prof, walk=True)
    assert frames("translucent", want, 3) == [(0, 0)] * 3
    g.close()


@gpu
def test_a_plan_counted_in_an_eliding_frame_equals_one_counted_with_the_switch_off(pta, oracle, monkeypatch):
    """A light edit drops the frame plan and keeps the records: the next plan is counted in a frame that elides.  It reads
    written + elided for bounce 1, so its queues, its inline rule and its last bounces are those of a frame that casts:
    PT_HIT1_FUSED=0 and then PT_HIT1_CACHE=0 render the oracle's frame with it and no queue runs full (the call after would
    fail), and a second scene that runs the sequence with PT_HIT1_FUSED=0 throughout has the same queue bytes and plan."""
    case, scene = open_scene("point", BOUNCES)
    prof = sb.profile(case, 160, 96, SPP)
    moved = [sb._light(pta, pta.PT_LIGHT_POINT, (-0.8, 2.9, 0.4), (20.0, 170.0, 90.0))]
    first = shared(("children", "open"), lambda: oracle_frame(oracle, scene, prof))
    want = oracle_frame(oracle, sb.build(case, pta=pta, camera=sb.make_camera(pta, **CAMERA), lights=moved), prof, walk=True)

    def sequence(switch_off):
        if switch_off:
            monkeypatch.setenv("PT_HIT1_FUSED", "0")
        g = pta.GpuScene(scene)
        seen = []

        def frames(what, w, n):
            for frame in range(n):
                assert_same(g.render(prof), w, (switch_off, what, frame))
                i = g.info().as_dict()
                seen.append((what, frame, i["queue_bytes"], i["frame_planned"]))

        frames("start", first, 4)
        g.set_lights(moved)
        frames("moved", want, 4)   # counted in the first, planned from the second on
        assert seen[-1][3] == 1, seen
        st = fused(g)
        assert (st["launches"] > 0 and st["elided"] > 0) != switch_off, (switch_off, st)
        monkeypatch.setenv("PT_HIT1_FUSED", "0")
        frames("switch off", want, 3)
        assert fused(g)["launches"] == st["launches"]
        monkeypatch.setenv("PT_HIT1_CACHE", "0")
        frames("cache off", want, 3)
        assert seen[-1][3] == 1, seen
        g.close()
        monkeypatch.delenv("PT_HIT1_CACHE")
        monkeypatch.delenv("PT_HIT1_FUSED")
        return seen

    assert sequence(False) == sequence(True)


@gpu
def test_chunks_sample_batches_and_a_partial_budget(pta, monkeypatch):
    """Small queues: two chunks of one pass over all eight samples, and - sample batches of two - four passes of one chunk
    each: every chunk below the mark takes the variant.  With room for about half of the items in the bounce-1 plane the
    prefix takes it and the rest casts.  Same bits as a frame with the caches switched off, in one pass."""
    case, scene = open_scene("point", BOUNCES)
    w, h, spp = 640, 360, 8
    items = 640 * 384 * spp
    prof = sb.profile(case, w, h, spp)
    one_pass = h1.uncached(pta, monkeypatch, scene, prof)
    monkeypatch.setenv("PT_QUEUE_GIB", "0.01")
    monkeypatch.setenv("PT_QUEUE_STEADY_GIB", "0.02")
    monkeypatch.setenv("PT_QUEUE_ONE_PASS_GIB", "0.02")
    whole = None
    for budget, batch in ((None, 0), (None, 2), ("0.015", 2)):
        if budget:
            monkeypatch.setenv("PT_HIT1_CACHE_GIB", budget)   # room for 1 006 592 items: two of the four batches
        g = pta.GpuScene(scene)
        before = fused(g)
        for frame in range(4):
            assert_same(g.render(prof, pta.Opts.make(sample_batch=batch)), one_pass, (budget, batch, frame))
            assert g.info().as_dict()["queue_chunk_items"] < items
            st, c = fused(g), h1.stats(g)
            d = delta(st, before)
            before = st
            if frame < 2:
                assert d == dict.fromkeys(NAMES, 0), (budget, batch, frame, d)
                continue
            assert d["launches"] >= 2 and d["unknown"] == 0 and d["elided"] > 0, (budget, batch, frame, d)
            assert st["launches"] == c["loads"], (budget, batch, frame, st, c)   # (every loading chunk took the variant)
            if budget is None:
                whole = whole or records(d)
                assert records(d) == whole, (batch, frame, d, whole)
            else:   # about half of the frame's records: the batches above the mark cast
                assert c["cached"] < items and 0.3 * whole < records(d) < 0.7 * whole, (frame, d, whole, c)
        g.close()


@gpu
def test_shards(pta, oracle):
    """Ranks 0 and 1 of 2 with 32 x 32 tiles, a scene and a plane each: each rank's pixels are the unsharded frame's."""
    case, scene = open_scene("point", BOUNCES)
    prof = sb.profile(case, 160, 96, SPP)
    want = shared(("children", "open"), lambda: oracle_frame(oracle, scene, prof))
    rgb, acc = np.zeros_like(want[0]), np.zeros_like(want[1])
    for r in range(2):
        o = pta.Opts.make(shard_rank=r, shard_count=2, tile_w=32, tile_h=32)
        m = pta.local_pixel_map(prof, o)
        g = pta.GpuScene(scene)
        for frame in range(4):
            rgb[m], acc[m] = g.render(prof, o)
        st = fused(g)
        assert st["launches"] == 2 and st["elided"] > 0 and st["unknown"] == 0 and records(st) <= 2 * len(m) * SPP, (r, st)
        g.close()
    assert_same((rgb, acc), want, "assembled")


@gpu
def test_switched_off_in_mid_sequence_and_on_again(pta, oracle, monkeypatch):
    """PT_HIT1_FUSED=0 between two frames: the loads go on - through k_wf_hits_load -, the variant's numbers stand still; on
    again it resumes at once: nothing was re-keyed.  The frames are the oracle's throughout."""
    _, scene, prof = open_case()
    want = open_want(oracle, scene, prof)
    g = pta.GpuScene(scene)
    per_frame = steady(g, prof, want, "on", frames=4)
    on, cache = fused(g), h1.stats(g)
    monkeypatch.setenv("PT_HIT1_FUSED", "0")
    for frame in range(2):
        assert_same(g.render(prof), want, ("off", frame))
    assert fused(g) == on and h1.stats(g) == dict(cache, loads=cache["loads"] + 2), (fused(g), h1.stats(g))
    monkeypatch.delenv("PT_HIT1_FUSED")
    for frame in range(2):
        assert_same(g.render(prof), want, ("on again", frame))
    assert delta(fused(g), on) == {k: 2 * v for k, v in per_frame.items()}, (fused(g), on, per_frame)
    assert h1.stats(g) == dict(cache, loads=cache["loads"] + 4), h1.stats(g)
    g.close()


def test_the_variants_keep_the_budget_of_the_kernel_they_replace(tmp_path):
    """From the built library: 128 vector registers, at most 8 B of scratch, LDS for four workgroups per CU."""
    t = kernel_table(tmp_path)
    for gridx in (11 | 32 | 64 | 128, 15 | 32 | 64 | 128):
        k = [v for name, v in t.items() if f"k_wf_shade_hitsILi{gridx}EE" in name]
        assert len(k) == 1, (gridx, [name for name in t if "k_wf_shade_hits" in name])
        print(gridx, k[0])
        assert k[0]["vgpr_count"] <= 128 and k[0]["private_segment_fixed_size"] <= 8 and k[0]["group_segment_fixed_size"] <= 40960, (gridx, k[0])
