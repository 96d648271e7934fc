"""The scene's cache of bounce-1 hits (csrc/pt_gpu.hip hit1_cache, csrc/pt_wavefront.h k_wf_hits_store / k_wf_hits_load): in
an opaque scene the bounce-1 ray of a work item is made from its camera hit, the material record there and words 2-3 of
its ChaCha block - no light enters - so the closest hit of that ray depends on the item enumeration, the camera, the
geometry and the materials, not on a light's position, kind, colour or count, nor on the bounce count.  One 16-byte
record per item keeps it (pack_hit with bit 28 of the word flipped: the zeroed plane says "never written"); the frames of
one view and material table store it once and load it afterwards, in place of bounce 1's casts.

What could go wrong: a stale record after a material edit or a camera move, a record of one item read for another, the hit
of a cast that was with the wide or the exact walker stored from the wrong plane, an item without a record read as a hit, a
record read beyond the budget or by another shard, a translucent frame taking the opaque record, the flags of the record
lost on the way, a frame on another stream reading before the plane was zeroed.  Every frame here is compared bit for bit
- f32 accumulator and rgb8 - with the CPU oracle or with a PT_HIT1_CACHE=0 render of the same sequence, and every test
reads the cache's own numbers (GpuScene.hit1_cache_stats): without them it would prove nothing.

An item without a record is made here by the study switch PT_HIT1_CACHE_HOLES.  The natural case - a path the escape masks
ended at bounce 0 while the plane was filled, alive under another light - cannot be built from the geometries of the shading
matrix: the masks of `open`, the one of them with normals long enough for the shadow queue and a background that is not
black, prove no miss at all (masked_casts is 0 in its instrumented frames under every light set), and nothing leaves the
closed ones.  It is built in tests/test_masked_sequences.py, on the builder's `terrace` geometry (kept out of the matrix),
whose masks do end paths: test_a_light_edit_revives_paths_the_masks_ended_while_the_planes_were_filled, no switch set."""
import numpy as np
import pytest

import scene_builder as sb
import test_camera_update as cu
from test_prestaged_misses import CAMERA, assert_same, open_scene, oracle_frame

gpu = pytest.mark.gpu

W, H, SPP, BOUNCES = 64, 48, 4, 5
NAMES = ("bytes", "items", "cached", "resets", "stores", "loads", "unknown")
NONE = dict.fromkeys(NAMES, 0)


def stats(g):
    return dict(zip(NAMES, g.hit1_cache_stats()))


_frames = {}


def shared(key, make):
    """A reference frame, made once, shared and left unchanged."""
    if key not in _frames:
        out = make()
        for a in out[:2]:
            a.setflags(write=False)
        _frames[key] = out
    return _frames[key]


def open_case():
    case, scene = open_scene("point", BOUNCES)
    return case, scene, sb.profile(case, W, H, SPP)


def open_want(oracle, scene, prof):
    return shared(("steady", "open"), lambda: oracle_frame(oracle, scene, prof))


def steady(g, prof, want, what, frames=5, opts=None, unknown=False):
    """The frames of a fresh scene: plain, then the one that keys and zeroes the plane and stores, then the loading ones - one
    load per frame (the frame is one chunk)."""
    for frame in range(frames):
        assert_same(g.render(prof, opts), want, (what, frame))
        st = stats(g)
        if frame == 0:
            assert st == NONE, (what, frame, st)
            continue
        assert st["bytes"] == 16 * st["items"] > 0 and st["items"] == g.hit_cache_stats()[1], (what, frame, st)
        assert st["cached"] == st["items"], (what, frame, st)
        assert (st["resets"], st["stores"], st["loads"]) == (1, 1, frame - 1), (what, frame, st)
        assert (st["unknown"] > 0) == (unknown and frame >= 2), (what, frame, st)


@gpu
@pytest.mark.parametrize("name", ["spheres", "cube", "reflection", "open"])
def test_consecutive_frames(pta, oracle, scene_cache, name):
    """Five frames.  Frame 0: nothing is allocated.  Frame 1: keyed, zeroed once, stored.  From frame 2: one load per frame,
    no item without a record, every item below the mark."""
    if name == "open":
        _, scene, prof = open_case()
        want = open_want(oracle, scene, prof)
    else:
        scene = scene_cache(name)
        prof = pta.Profile.make(W, H, SPP, 3)
        want = shared(("steady", name), lambda: oracle_frame(oracle, scene, prof))
    g = pta.GpuScene(scene)
    assert not g.info().has_translucent
    steady(g, prof, want, name)
    g.close()


@gpu
def test_light_edits_keep_the_records(pta, oracle):
    """A moved light, a recoloured light, light counts 1 -> 2 -> 1: the loads go on, no reset, no store - unless the camera
    grid's resolution changed with the count, which is part of the key: then the re-keying is asserted instead.  Every frame
    equals the oracle for the new lights."""
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
            st = stats(g)
            if rekeyed:   # nothing, then zeroed and stored, then loaded
                assert (st["resets"], st["stores"], st["loads"]) == (before["resets"] + (frame >= 1), before["stores"] + (frame >= 1),
                                                                    before["loads"] + (frame >= 2)), (what, frame, st, before)
            else:   # (unknown casts may appear: the escape masks end other paths at bounce 0 under other lights)
                assert dict(st, unknown=0) == dict(before, unknown=0, loads=before["loads"] + 1 + frame), (what, frame, st, before)
    assert np.array_equal(seen[-1][1], first[1])
    g.close()


@gpu
def test_a_material_edit_rekeys(pta, oracle):
    """A table with other roughnesses gives other directions: the next frame neither loads nor stores, the one after zeroes
    and stores, the third loads.  Back to the first table the same again - a stale record would show as another image."""
    case, scene, prof = open_case()
    cam = sb.make_camera(pta, **CAMERA)
    first_table = sb.case_materials(case, pta)
    other = sb.case_materials(case, pta)
    for m in other:
        m.roughness = min(1.0, 0.37 + 0.5 * m.roughness)
    first = open_want(oracle, scene, prof)
    want_other = oracle_frame(oracle, sb.build(case, pta=pta, camera=cam, materials=other), prof, walk=True)
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
            assert (st["resets"], st["stores"], st["loads"], st["unknown"]) == (resets, stores, loads, 0), (what, frame, st)
    g.close()


@gpu
def test_camera_moves_translucency_and_frames_without_a_bounce(pta, oracle):
    """A camera move re-keys like a material edit; a camera path - a move before every frame - never allocates.  A translucent
    table stops the cache, the return to opaque resumes it (re-keyed: the table is a new one).  Frames of no bounce leave it
    alone."""
    case, scene, prof = open_case()
    cam1 = sb.make_camera(pta, **CAMERA)
    cam2 = sb.make_camera(pta, eye=(-0.9, 2.1, 2.9), target=(0.3, 0.3, -0.4), fov=0.8)
    opaque = sb.case_materials(case, pta)
    alpha = sb.case_materials(case._replace(factor_set="alpha"), pta)
    first = open_want(oracle, scene, prof)
    want2 = oracle_frame(oracle, sb.build(case, pta=pta, camera=cam2), prof, walk=True)
    alpha_scene = sb.build(case, pta=pta, camera=cam2, materials=alpha)
    assert alpha_scene.translucent
    want_alpha = oracle_frame(oracle, alpha_scene, prof, walk=True)
    prof0 = sb.profile(case, W, H, SPP, bounces=0)
    want0 = oracle_frame(oracle, sb.build(case, pta=pta, camera=cam2), prof0)
    g = pta.GpuScene(scene)
    for k in range(4):   # a path: never the same camera twice in a row
        g.set_camera(cam2 if k & 1 else cam1)
        assert_same(g.render(prof), want2 if k & 1 else first, ("path", k))
        assert stats(g) == NONE, (k, stats(g))
    g.set_camera(cam1)
    steady(g, prof, first, "first camera", frames=4)
    g.set_camera(cam2)
    for frame, (r, s, l) in enumerate([(1, 1, 2), (2, 2, 2), (2, 2, 3)]):
        assert_same(g.render(prof), want2, ("moved", frame))
        st = stats(g)
        assert (st["resets"], st["stores"], st["loads"]) == (r, s, l), (frame, st)
        assert st["cached"] == (0 if frame == 0 else st["items"]), (frame, st)
    before = stats(g)
    for frame in range(2):
        assert_same(g.render(prof0), want0, ("no bounce", frame))
        assert stats(g) == before, (frame, stats(g))
    assert_same(g.render(prof), want2, "bounces again")
    assert stats(g) == dict(before, loads=before["loads"] + 1), stats(g)
    before = stats(g)
    g.set_materials(alpha)
    for frame in range(2):
        assert_same(g.render(prof), want_alpha, ("translucent", frame))
        assert stats(g) == before, (frame, stats(g))
    g.set_materials(opaque)
    for frame, (dr, ds, dl) in enumerate([(0, 0, 0), (1, 1, 0), (1, 1, 1)]):
        assert_same(g.render(prof), want2, ("opaque again", frame))
        st = stats(g)
        assert (st["resets"], st["stores"], st["loads"]) == (before["resets"] + dr, before["stores"] + ds, before["loads"] + dl), (frame, st)
    g.close()


@gpu
def test_holes(pta, oracle, monkeypatch):
    """PT_HIT1_CACHE_HOLES=3: the storing launch leaves out every third item, so the loading launches find items without a
    record, list them for the exact walker, and the frame is still the oracle's."""
    _, scene, prof = open_case()
    want = open_want(oracle, scene, prof)
    monkeypatch.setenv("PT_HIT1_CACHE_HOLES", "3")
    g = pta.GpuScene(scene)
    steady(g, prof, want, "holes", unknown=True)
    per_frame = stats(g)["unknown"] // 3
    assert stats(g)["unknown"] == 3 * per_frame and 0 < per_frame <= W * H * SPP // 3 + 1, stats(g)
    g.close()


# The pipeline's own switches are read once per process: one child per setting.  A child renders the `open` scene at
# 160 x 96 - five frames with every third record left out, then an instrumented frame - and prints a hash of every frame,
# the cache's numbers and how many casts went through the wide and the exact walker.
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
    out.append([sha, [int(v) for v in g.hit1_cache_stats()]])
g.render(prof, pta.Opts.make(flags=pta.PT_FLAG_COUNTERS))
c = g.counters().as_dict()
print("RESULT", json.dumps({"frames": out, "deferred": c["deferred_casts"], "exact": c["exact_casts"]}))
"""
SETTINGS = [
    {},                                            # the shade pass split, k_wf_trace lists the rays it does not take
    {"PT_WF_SPLIT": "0"},                          # one shade pass: every hit in the chunk's own plane
    {"PT_WF_EXACT": "2"},                          # the shade pass lists those rays (a loading chunk's bounce 0: none)
    {"PT_WF_EXACT": "2", "PT_WF_SPLIT": "0"},
    {"PT_WF_DEFER": "2"},                          # many casts through the wide walker: their hits are in the hand-over list's plane
    {"PT_WF_DEFER": "2", "PT_WF_EXACT": "2"},
]


@gpu
@pytest.mark.parametrize("setting", SETTINGS, ids=lambda s: "-".join(f"{k[6:]}{v}" for k, v in s.items()) or "default")
def test_holes_with_the_shade_pass_split_or_not_and_both_exact_modes(oracle, setting):
    """PT_WF_SPLIT 1 and 0, PT_WF_EXACT 1 and 2, and an early hand-over to the wide walker: the storing launch finds every
    final hit where that setting leaves it (the chunk's plane, the hand-over list's plane, the exact list's words), and the
    loading launches mark and list the items without a record as that setting's shade passes expect."""
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
    for frame, (sha, st) in enumerate(res["frames"]):
        st = dict(zip(NAMES, st))
        assert sha == want_sha, (setting, frame, st)
        if frame >= 1:
            assert (st["resets"], st["stores"], st["loads"]) == (1, 1, frame - 1) and (st["unknown"] > 0) == (frame >= 2), (setting, frame, st)
    assert res["exact"] > 0, (setting, res)   # (the premise: rays the wavefront walker does not take exist in this frame)
    if setting.get("PT_WF_DEFER") == "2":
        assert res["deferred"] > 0, (setting, res)


def uncached(pta, monkeypatch, scene, prof, opts=None):
    monkeypatch.setenv("PT_HIT1_CACHE", "0")
    g = pta.GpuScene(scene)
    out = [g.render(prof, opts) for _ in range(3)][-1]
    assert stats(g) == NONE
    g.close()
    monkeypatch.delenv("PT_HIT1_CACHE")
    return out


@gpu
def test_chunks_sample_batches_and_a_partial_budget(pta, monkeypatch):
    """Small queues: the frame runs in two chunks of one pass over all eight samples, and - sample batches of two - in four
    passes of one chunk each; the plane grows as a prefix over them.  With room for about half of the items the rest casts
    as before.  Same bits as a frame with the cache switched off, in one pass."""
    case, scene = open_scene("point", BOUNCES)
    w, h, spp = 640, 360, 8
    items = 640 * 384 * spp   # 1 966 080 (32 x 32 tiles): 31.5 MB of records
    prof = sb.profile(case, w, h, spp)
    one_pass = uncached(pta, monkeypatch, scene, prof)
    monkeypatch.setenv("PT_QUEUE_GIB", "0.01")
    monkeypatch.setenv("PT_QUEUE_STEADY_GIB", "0.02")
    monkeypatch.setenv("PT_QUEUE_ONE_PASS_GIB", "0.02")
    for budget, batch in ((None, 0), (None, 2), ("0.015", 2)):
        if budget:
            monkeypatch.setenv("PT_HIT1_CACHE_GIB", budget)   # room for 1 006 592 items: two of the four batches
        g = pta.GpuScene(scene)
        loads = 0
        for frame in range(4):
            assert_same(g.render(prof, pta.Opts.make(sample_batch=batch)), one_pass, (budget, batch, frame))
            assert g.info().as_dict()["queue_chunk_items"] < items
            st = stats(g)
            if frame == 0:
                assert st == NONE, st
                continue
            assert st["items"] == items and st["stores"] >= 1 and st["resets"] == 1 and st["unknown"] == 0, (budget, batch, frame, st)
            if budget is None:
                assert st["cached"] == items and st["bytes"] == items * 16, (batch, frame, st)
            else:
                assert 0 < st["cached"] <= 1006592 and st["cached"] % 64 == 0 and st["bytes"] <= 0.015 * 2 ** 30, (frame, st)
            if frame >= 2:
                assert st["loads"] > loads, (budget, batch, frame, st)
            loads = st["loads"]
        g.close()


@gpu
def test_shards(pta, oracle):
    """Ranks 0 and 1 of 2 with 32 x 32 tiles, a scene and a plane each: each rank's pixels are the unsharded frame's."""
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
        st = stats(g)
        assert st["items"] == st["cached"] >= len(m) * SPP and (st["resets"], st["stores"], st["loads"], st["unknown"]) == (1, 1, 2, 0), (r, st)
        g.close()
    assert_same((rgb, acc), want, "assembled")


@gpu
def test_frames_in_flight_on_two_streams(pta, oracle):
    """Six frames enqueued without a host wait, alternating between two streams: the plane is zeroed and filled on one stream
    and first read on the other."""
    import torch
    _, scene, prof = open_case()
    want = open_want(oracle, scene, prof)
    n = W * H
    outs = [(torch.empty(n * 3, dtype=torch.uint8, device="cuda"), torch.empty(n * 3, dtype=torch.float32, device="cuda")) for _ in range(6)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    g = pta.GpuScene(scene)
    for k, (rgb, acc) in enumerate(outs):
        st = streams[k & 1]
        st.wait_stream(streams[(k & 1) ^ 1])
        g.render_device(prof, pta.Opts.make(), rgb.data_ptr(), acc.data_ptr(), st.cuda_stream)
    for st in streams:
        st.synchronize()
    for k, (rgb, acc) in enumerate(outs):
        assert_same((rgb.cpu().numpy().reshape(-1, 3), acc.cpu().numpy().reshape(-1, 3)), want, k)
    st = stats(g)
    assert (st["resets"], st["stores"], st["loads"], st["unknown"]) == (1, 1, 4, 0), st
    g.close()


@gpu
def test_switched_off(pta, oracle, monkeypatch):
    """PT_HIT1_CACHE=0: same bits, nothing allocated, and the launches of a frame without the cache - one stage launch fewer
    than the storing frame; switched off on a scene that has a plane: released."""
    _, scene, prof = open_case()
    want = open_want(oracle, scene, prof)
    timing = pta.Opts.make(flags=pta.PT_FLAG_TIMING)
    monkeypatch.setenv("PT_HIT1_CACHE", "0")
    g = pta.GpuScene(scene)
    off = []
    for frame in range(4):
        assert_same(g.render(prof, timing), want, ("off", frame))
        assert stats(g) == NONE
        off.append((g.timing().launches, g.timing().stage_launches))
    monkeypatch.delenv("PT_HIT1_CACHE")
    on = []
    for frame in range(3):   # (the frame before had this key: keyed at once)
        assert_same(g.render(prof, timing), want, ("on", frame))
        on.append((g.timing().launches, g.timing().stage_launches))
    st = stats(g)
    assert st["bytes"] > 0 and (st["resets"], st["stores"], st["loads"]) == (1, 1, 2), st
    print("launches, stage launches: off", off, "on", on)
    assert on[0] == (off[-1][0], off[-1][1] + 1), (on, off)       # the storing frame: the parent's launches + the store
    assert on[1] == off[-1] and on[2] == on[1], (on, off)          # a loading frame: the load in place of the trace stage
    monkeypatch.setenv("PT_HIT1_CACHE", "0")
    assert_same(g.render(prof, timing), want, "off again")
    assert stats(g)["bytes"] == 0 and stats(g)["items"] == 0
    assert (g.timing().launches, g.timing().stage_launches) == off[-1]
    g.close()


@gpu
@pytest.mark.parametrize("name", ["spheres", "cube"])
def test_record_round_trip_on_the_golden_scenes(pta, monkeypatch, name):
    """Sphere entry and exit hits (bits 31 and 29 of a record's first word), back faces (bit 30), the miss word and primitive
    0 (a word that is zero before bit 28 is flipped): the rays that leave the spheres and the cube's faces in every direction
    meet all of them.  Stored-then-loaded frames equal the frames of a scene with the cache switched off."""
    prof = pta.Profile.make(96, 64, SPP, 3)
    want = uncached(pta, monkeypatch, cu.load(pta, name), prof)
    g = pta.GpuScene(cu.load(pta, name))
    for frame in range(4):
        assert_same(g.render(prof), want, (name, frame))
    st = stats(g)
    assert st == dict(bytes=16 * 96 * 64 * SPP, items=96 * 64 * SPP, cached=96 * 64 * SPP, resets=1, stores=1, loads=2, unknown=0), st
    g.close()
