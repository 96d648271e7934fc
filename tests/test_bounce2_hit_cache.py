"""The scene's cache of bounce-2 hits (csrc/pt_gpu.hip hit2_cache; the kernels are the bounce-1 hit cache's, k_wf_hits_store /
k_wf_hits_load in csrc/pt_wavefront.h, which work from the bounce they are launched for): in an opaque scene the bounce-2
ray of a work item is made from its bounce-1 hit, the material there and the item's random words - no light enters, and the
Russian roulette starts behind it - so its closest hit has the key of the bounce-1 hits: the view and the material table.
One more plane of 16-byte records, keyed, zeroed and stored by the same frame as the bounce-1 plane, loaded afterwards in
place of bounce 2's casts.

What could go wrong beyond the bounce-1 cache's list (tests/test_bounce1_hit_cache.py): the two planes or their counters
mixed up, the bounce-1 shade pass of a chunk that loads bounce 2 listing rays for the exact walker (they would be cast and
their hits written over the loaded ones - or the list of unknown casts would be too short), a plan counted in a loading
frame too short for a frame that casts, a store after bounce 3's casts rewrote the hit plane, one cache switched off
taking the other's records along.  Every frame here is compared bit for bit - f32 accumulator and rgb8 - with the CPU
oracle or with a render of the same sequence with the cache switched off, and every test reads both caches' numbers
(GpuScene.hit1_cache_stats, hit2_cache_stats).

An item without a record is made here by the study switch PT_HIT2_CACHE_HOLES: the escape masks of `open` prove no miss (the
reason given in tests/test_bounce1_hit_cache.py).  The natural case - a plane filled while the masks ended paths, read under
lights that keep them alive - is tests/test_masked_sequences.py, on the builder's `terrace` geometry, without the switch."""
import numpy as np
import pytest

import scene_builder as sb
import test_bounce1_hit_cache as h1
from test_prestaged_misses import CAMERA, assert_same, open_scene, oracle_frame

gpu = pytest.mark.gpu

W, H, SPP, BOUNCES = h1.W, h1.H, h1.SPP, h1.BOUNCES
NAMES, NONE = h1.NAMES, h1.NONE
shared, open_case, open_want = h1.shared, h1.open_case, h1.open_want


def stats(g):
    """(the bounce-1 cache's numbers, the bounce-2 cache's)"""
    return dict(zip(NAMES, g.hit1_cache_stats())), dict(zip(NAMES, g.hit2_cache_stats()))


def counts(st):
    return st["resets"], st["stores"], st["loads"]


def steady(g, prof, want, what, frames=5, unknown=False, bounce2=True):
    """The frames of a fresh scene: plain, then the one that keys and zeroes BOTH planes and stores both, then the loading
    ones - one load per plane and frame (the frame is one chunk).  bounce2=False: no path of the scene has a bounce-2 ray -
    the frame plan ends the chunk behind bounce 1, so the bounce-2 plane is keyed and marked full without a launch."""
    for frame in range(frames):
        assert_same(g.render(prof), want, (what, frame))
        s1, s2 = stats(g)
        if frame == 0:
            assert s1 == NONE and s2 == NONE, (what, frame, s1, s2)
            continue
        for st in (s1, s2):
            assert st["bytes"] == 16 * st["items"] > 0 and st["items"] == g.hit_cache_stats()[1], (what, frame, st)
            assert st["cached"] == st["items"], (what, frame, st)
        assert counts(s1) == (1, 1, frame - 1), (what, frame, s1, s2)
        assert counts(s2) == ((1, 1, frame - 1) if bounce2 else (1, 0, 0)), (what, frame, s1, s2)
        assert s1["unknown"] == 0 and (s2["unknown"] > 0) == (unknown and frame >= 2), (what, frame, s1, s2)


@gpu
@pytest.mark.parametrize("name", ["spheres", "cube", "reflection", "open"])
def test_consecutive_frames(pta, oracle, scene_cache, name):
    """Five frames.  Frame 0: nothing is allocated.  Frame 1: both planes keyed, zeroed once, stored.  From frame 2: one load
    per plane and frame, no item without a record.  cube: one convex body under a black sky - every ray that leaves its
    surface leaves the scene, no path has a bounce-2 ray."""
    if name == "open":
        _, scene, prof = open_case()
        want = open_want(oracle, scene, prof)
    else:
        scene = scene_cache(name)
        prof = pta.Profile.make(W, H, SPP, 3)
        want = shared(("steady", name), lambda: oracle_frame(oracle, scene, prof))
    g = pta.GpuScene(scene)
    assert not g.info().has_translucent
    steady(g, prof, want, name, bounce2=name != "cube")
    g.close()


@gpu
def test_light_edits_keep_the_records(pta, oracle):
    """A recoloured light, a moved light, light counts 1 -> 2 -> 1: both planes go on loading, no reset, no store - unless the
    camera grid's resolution changed with the count, which is part of the key: then the re-keying is asserted instead.
    Every frame equals the oracle for the new lights."""
    case, scene, prof = open_case()
    P = pta.PT_LIGHT_POINT
    cam = sb.make_camera(pta, **CAMERA)
    lights1 = sb.make_lights(pta, "point")
    recoloured = [sb._light(pta, P, tuple(lights1[0].vec), (20.0, 170.0, 90.0))]
    moved = [sb._light(pta, P, (-0.8, 2.9, 0.4), (20.0, 170.0, 90.0))]
    two = moved + [sb._light(pta, P, (-1.0, 3.0, 0.2), (60.0, 20.0, 90.0))]
    first = open_want(oracle, scene, prof)
    g = pta.GpuScene(scene)
    steady(g, prof, first, "start", frames=4)
    seen = [first]
    for what, lights in (("colour", recoloured), ("moved", moved), ("two", two), ("one", lights1)):
        before, res = stats(g), g.info().as_dict().get("cam_grid_res")
        g.set_lights(lights)
        rekeyed = g.info().as_dict().get("cam_grid_res") != res
        want = oracle_frame(oracle, sb.build(case, pta=pta, camera=cam, lights=lights), prof, walk=True)
        assert not np.array_equal(want[1], seen[-1][1]), what   # (the edit changed the image)
        seen.append(want)
        for frame in range(3):
            assert_same(g.render(prof), want, (what, frame))
            for st, b in zip(stats(g), before):
                if rekeyed:   # nothing, then zeroed and stored, then loaded
                    assert counts(st) == (b["resets"] + (frame >= 1), b["stores"] + (frame >= 1), b["loads"] + (frame >= 2)), (what, frame, st, b)
                else:   # (unknown casts are allowed: the escape masks end other paths early under other lights)
                    assert dict(st, unknown=0) == dict(b, unknown=0, loads=b["loads"] + 1 + frame), (what, frame, st, b)
    assert np.array_equal(seen[-1][1], first[1])
    g.close()


@gpu
def test_a_material_edit_and_a_camera_move_rekey(pta, oracle):
    """A table with other roughnesses, then another camera: the next frame neither loads nor stores, the one after zeroes and
    stores both planes, the third loads both.  Back to the first table and camera the same again - a stale record would show
    as another image."""
    case, scene, prof = open_case()
    cam1 = sb.make_camera(pta, **CAMERA)
    cam2 = sb.make_camera(pta, eye=(-0.9, 2.1, 2.9), target=(0.3, 0.3, -0.4), fov=0.8)
    first_table = sb.case_materials(case, pta)
    other = sb.case_materials(case, pta)
    for m in other:
        m.roughness = min(1.0, 0.37 + 0.5 * m.roughness)
    first = open_want(oracle, scene, prof)
    want_other = oracle_frame(oracle, sb.build(case, pta=pta, camera=cam1, materials=other), prof, walk=True)
    want_moved = oracle_frame(oracle, sb.build(case, pta=pta, camera=cam2, materials=other), prof, walk=True)
    assert not np.array_equal(first[1], want_other[1]) and not np.array_equal(want_other[1], want_moved[1])
    g = pta.GpuScene(scene)
    steady(g, prof, first, "start", frames=4)
    resets, stores, loads = 1, 1, 2

    def edit_table(t):
        g.set_materials(t)

    def edit_both(_):
        g.set_camera(cam1)
        g.set_materials(first_table)

    for what, edit, arg, want in (("other table", edit_table, other, want_other), ("other camera", g.set_camera, cam2, want_moved),
                                  ("first again", edit_both, None, first)):
        edit(arg)
        for frame, (dr, ds, dl) in enumerate([(0, 0, 0), (1, 1, 0), (0, 0, 1), (0, 0, 1)]):
            assert_same(g.render(prof), want, (what, frame))
            resets, stores, loads = resets + dr, stores + ds, loads + dl
            for st in stats(g):
                assert counts(st) + (st["unknown"],) == (resets, stores, loads, 0), (what, frame, st)
                assert st["cached"] == (0 if frame == 0 and what != "other table" else st["items"]), (what, frame, st)
    g.close()


@gpu
def test_bounce_counts_and_translucency(pta, oracle):
    """Profiles of one bounce never key the bounce-2 plane (the bounce-1 plane goes its way).  Bounces 5 -> 2 -> 5: the records
    stay - the bounce count is not in the key - and the frames of 2 bounces load them too.  A translucent table: neither
    plane is touched."""
    case, scene, prof = open_case()
    first = open_want(oracle, scene, prof)
    prof1, prof2 = sb.profile(case, W, H, SPP, bounces=1), sb.profile(case, W, H, SPP, bounces=2)
    want1, want2 = oracle_frame(oracle, scene, prof1), oracle_frame(oracle, scene, prof2)
    g = pta.GpuScene(scene)
    for frame in range(4):
        assert_same(g.render(prof1), want1, ("one bounce", frame))
        s1, s2 = stats(g)
        assert s2 == NONE and counts(s1) == ((0, 0, 0) if frame == 0 else (1, 1, frame - 1)), (frame, s1, s2)
    assert_same(g.render(prof), first, "five bounces, keyed at once")   # (the frame before had this key)
    s1, s2 = stats(g)
    assert counts(s1) == (1, 1, 3) and counts(s2) == (1, 1, 0) and s2["cached"] == s2["items"] == s1["items"], (s1, s2)
    loads = 0
    for what, p, want in (("five", prof, first), ("two", prof2, want2), ("two", prof2, want2), ("five", prof, first)):
        assert_same(g.render(p), want, what)
        loads += 1
        s1, s2 = stats(g)
        assert counts(s2) == (1, 1, loads) and counts(s1) == (1, 1, 3 + loads) and s2["unknown"] == 0, (what, s1, s2)
    alpha = sb.case_materials(case._replace(factor_set="alpha"), pta)
    alpha_scene = sb.build(case, pta=pta, camera=sb.make_camera(pta, **CAMERA), materials=alpha)
    assert alpha_scene.translucent
    want_alpha = oracle_frame(oracle, alpha_scene, prof, walk=True)
    before = stats(g)
    g.set_materials(alpha)
    for frame in range(3):
        assert_same(g.render(prof), want_alpha, ("translucent", frame))
        assert stats(g) == before, (frame, stats(g))
    g.close()
    g = pta.GpuScene(alpha_scene)   # translucent from the start: never keyed
    for frame in range(3):
        assert_same(g.render(prof), want_alpha, ("translucent scene", frame))
        assert stats(g) == (NONE, NONE), (frame, stats(g))
    g.close()


@gpu
def test_holes(pta, oracle, monkeypatch):
    """PT_HIT2_CACHE_HOLES=3: the storing launch of bounce 2 leaves out every third item, so the loading launches find items
    without a record, list them for the exact walker, and the frame is still the oracle's.  The bounce-1 plane has none."""
    _, scene, prof = open_case()
    want = open_want(oracle, scene, prof)
    monkeypatch.setenv("PT_HIT2_CACHE_HOLES", "3")
    g = pta.GpuScene(scene)
    steady(g, prof, want, "holes", unknown=True)
    s2 = stats(g)[1]
    per_frame = s2["unknown"] // 3
    assert s2["unknown"] == 3 * per_frame and 0 < per_frame <= W * H * SPP // 3 + 1, s2
    g.close()


# The pipeline's own switches are read once per process: one child per setting (as tests/test_bounce1_hit_cache.py).
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
    out.append([sha, [int(v) for v in g.hit1_cache_stats()], [int(v) for v in g.hit2_cache_stats()]])
g.render(prof, pta.Opts.make(flags=pta.PT_FLAG_COUNTERS))
c = g.counters().as_dict()
print("RESULT", json.dumps({"frames": out, "deferred": c["deferred_casts"], "exact": c["exact_casts"]}))
"""


@gpu
@pytest.mark.parametrize("setting", h1.SETTINGS, ids=lambda s: "-".join(f"{k[6:]}{v}" for k, v in s.items()) or "default")
def test_holes_with_the_shade_pass_split_or_not_and_both_exact_modes(oracle, setting):
    """PT_WF_SPLIT 1 and 0, PT_WF_EXACT 1 and 2, and an early hand-over to the wide walker, with every third record of the
    bounce-2 plane left out: the storing launch finds every final hit where that setting leaves it, the bounce-1 shade pass of
    a loading chunk lists nothing under PT_WF_EXACT=2, and the loading launches mark and list the items without a record as
    that setting's shade passes expect."""
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
    env = {k: v for k, v in os.environ.items() if not k.startswith(("PT_WF_", "PT_HIT1_", "PT_HIT2_"))}
    env.update(setting, PT_HIT2_CACHE_HOLES="3")
    run = subprocess.run([sys.executable, "-c", CHILD % {"root": str(root)}], env=env, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, (setting, run.stderr[-2000:])
    res = json.loads([ln for ln in run.stdout.splitlines() if ln.startswith("RESULT ")][0][7:])
    print(setting, res)
    for frame, (sha, s1, s2) in enumerate(res["frames"]):
        s1, s2 = dict(zip(NAMES, s1)), dict(zip(NAMES, s2))
        assert sha == want_sha, (setting, frame, s1, s2)
        if frame >= 1:
            assert counts(s1) == counts(s2) == (1, 1, frame - 1), (setting, frame, s1, s2)
            assert s1["unknown"] == 0 and (s2["unknown"] > 0) == (frame >= 2), (setting, frame, s1, s2)
    assert res["exact"] > 0, (setting, res)   # (the premise: rays the wavefront walker does not take exist in this frame)
    if setting.get("PT_WF_DEFER") == "2":
        assert res["deferred"] > 0, (setting, res)


@gpu
def test_chunks_sample_batches_and_a_partial_budget(pta, monkeypatch):
    """Small queues: two chunks of one pass over all eight samples, and - sample batches of two - four passes of one chunk
    each; the plane grows as a prefix over them.  With room for about half of the items the prefix loads and the rest casts
    as before, while the bounce-1 plane holds every item.  Same bits as a frame with both caches switched off, in one pass."""
    case, scene = open_scene("point", BOUNCES)
    w, h, spp = 640, 360, 8
    items = 640 * 384 * spp   # 1 966 080 (32 x 32 tiles): 31.5 MB of records
    prof = sb.profile(case, w, h, spp)
    one_pass = h1.uncached(pta, monkeypatch, scene, prof)   # (PT_HIT1_CACHE=0 takes the bounce-2 cache out of use too)
    monkeypatch.setenv("PT_QUEUE_GIB", "0.01")
    monkeypatch.setenv("PT_QUEUE_STEADY_GIB", "0.02")
    monkeypatch.setenv("PT_QUEUE_ONE_PASS_GIB", "0.02")
    for budget, batch in ((None, 0), (None, 2), ("0.015", 2)):
        if budget:
            monkeypatch.setenv("PT_HIT2_CACHE_GIB", budget)   # room for 1 006 592 items: two of the four batches
        g = pta.GpuScene(scene)
        loads = 0
        for frame in range(4):
            assert_same(g.render(prof, pta.Opts.make(sample_batch=batch)), one_pass, (budget, batch, frame))
            assert g.info().as_dict()["queue_chunk_items"] < items
            s1, s2 = stats(g)
            if frame == 0:
                assert s1 == NONE and s2 == NONE, (s1, s2)
                continue
            assert s1["cached"] == s1["items"] == items and s1["unknown"] == 0, (budget, batch, frame, s1)
            assert s2["items"] == items and s2["stores"] >= 1 and s2["resets"] == 1 and s2["unknown"] == 0, (budget, batch, frame, s2)
            if budget is None:
                assert s2["cached"] == items and s2["bytes"] == items * 16 and s2["loads"] == s1["loads"], (batch, frame, s1, s2)
            else:
                assert 0 < s2["cached"] <= 1006592 and s2["cached"] % 64 == 0 and s2["bytes"] <= 0.015 * 2 ** 30, (frame, s2)
                assert frame < 2 or 0 < s2["loads"] < s1["loads"], (frame, s1, s2)   # the rest of the frame casts bounce 2
            if frame >= 2:
                assert s2["loads"] > loads, (budget, batch, frame, s2)
            loads = s2["loads"]
        g.close()


@gpu
def test_switches(pta, oracle, monkeypatch):
    """PT_HIT1_CACHE=0 takes the bounce-2 cache out of use: nothing is allocated for either.  PT_HIT2_CACHE=0 in the middle of a
    sequence releases the bounce-2 plane and leaves the bounce-1 cache's numbers going as they were; switched on again it is
    keyed at once, stores, then loads."""
    _, scene, prof = open_case()
    want = open_want(oracle, scene, prof)
    monkeypatch.setenv("PT_HIT1_CACHE", "0")
    g = pta.GpuScene(scene)
    for frame in range(3):
        assert_same(g.render(prof), want, ("both off", frame))
        assert stats(g) == (NONE, NONE), (frame, stats(g))
    monkeypatch.delenv("PT_HIT1_CACHE")
    for frame in range(3):   # (the frame before had this key: keyed at once)
        assert_same(g.render(prof), want, ("on", frame))
        s1, s2 = stats(g)
        assert counts(s1) == counts(s2) == (1, 1, frame), (frame, s1, s2)
    monkeypatch.setenv("PT_HIT2_CACHE", "0")
    for frame in range(2):
        assert_same(g.render(prof), want, ("bounce 2 off", frame))
        s1, s2 = stats(g)
        assert (s2["bytes"], s2["items"], s2["cached"]) == (0, 0, 0) and counts(s2) == (1, 1, 2), (frame, s2)
        assert counts(s1) == (1, 1, 3 + frame) and s1["cached"] == s1["items"] > 0 and s1["unknown"] == 0, (frame, s1)
    monkeypatch.delenv("PT_HIT2_CACHE")
    for frame in range(3):
        assert_same(g.render(prof), want, ("bounce 2 on again", frame))
        s1, s2 = stats(g)
        assert counts(s2) == (2, 2, 2 + frame) and s2["cached"] == s2["items"] == s1["items"], (frame, s2)   # (keyed at once)
        assert counts(s1) == (1, 1, 5 + frame) and s2["unknown"] == 0, (frame, s1, s2)
    g.close()


@gpu
def test_a_plan_counted_in_a_loading_frame_serves_a_frame_that_casts(pta, oracle, monkeypatch):
    """A light edit drops the frame plan and keeps the records: the next plan is counted in a frame that loaded bounces 1 and
    2, whose lists for the exact walker were empty.  The cache switched off after that, the frame casts bounce 2 and lists
    its rays: the list must be long enough - same bits as the oracle, and the frame after it does not report a queue that
    ran full."""
    case, scene = open_scene("point", BOUNCES)
    prof = sb.profile(case, 160, 96, SPP)
    P = pta.PT_LIGHT_POINT
    moved = [sb._light(pta, P, (-0.8, 2.9, 0.4), (20.0, 170.0, 90.0))]
    want = oracle_frame(oracle, sb.build(case, pta=pta, camera=sb.make_camera(pta, **CAMERA), lights=moved), prof, walk=True)
    g = pta.GpuScene(scene)
    for frame in range(4):
        g.render(prof)
    assert counts(stats(g)[1]) == (1, 1, 2), stats(g)
    g.set_lights(moved)
    for frame in range(3):   # counted in the first, planned from the second on
        assert_same(g.render(prof), want, ("moved", frame))
    assert counts(stats(g)[1]) == (1, 1, 5) and g.info().as_dict()["frame_planned"] == 1, (stats(g), g.info().as_dict())
    monkeypatch.setenv("PT_HIT2_CACHE", "0")
    for frame in range(3):
        assert_same(g.render(prof), want, ("bounce 2 cast", frame))
    assert stats(g)[1]["bytes"] == 0 and counts(stats(g)[0]) == (1, 1, 8), stats(g)
    monkeypatch.setenv("PT_HIT1_CACHE", "0")
    for frame in range(3):
        assert_same(g.render(prof), want, ("both cast", frame))
    g.close()


@gpu
def test_shards(pta, oracle):
    """Ranks 0 and 1 of 2 with 32 x 32 tiles, a scene and two planes each: each rank's pixels are the unsharded frame's."""
    case, scene = open_scene("point", BOUNCES)
    w, h = 160, 96
    prof = sb.profile(case, w, h, SPP)
    want = oracle_frame(oracle, scene, prof)
    rgb, acc = np.zeros_like(want[0]), np.zeros_like(want[1])
    for r in range(2):
        o = pta.Opts.make(shard_rank=r, shard_count=2, tile_w=32, tile_h=32)
        m = pta.local_pixel_map(prof, o)
        g = pta.GpuScene(scene)
        for frame in range(4):
            rgb[m], acc[m] = g.render(prof, o)
        for st in stats(g):
            assert st["items"] == st["cached"] >= len(m) * SPP and counts(st) + (st["unknown"],) == (1, 1, 2, 0), (r, st)
        g.close()
    assert_same((rgb, acc), want, "assembled")
