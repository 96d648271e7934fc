"""The scene's cache of camera hits (csrc/pt_gpu.hip HitCache, csrc/pt_wavefront.h k_wf_shade_hits): the closest hit of a
camera ray depends on the item enumeration, the camera and the geometry - not on the lights, the bounce count or, in an
opaque scene, the materials - so a frame that directly follows another of the same view stores the casts' results, and the
bounce-0 kernel of the later frames loads them instead of casting.

What could go wrong: a stale record after the camera moved or the enumeration changed, a record read above the stored prefix
or beyond the budget, a shard reading another shard's records, a record format that does not survive the round trip (sphere
entry and exit hits, back faces, "no hit"), a culled wavefront's slot read as a hit, a translucent frame taking the opaque
cast's result, a frame on another stream loading before the store has finished.  Every frame here is compared bit for bit -
f32 accumulator and rgb8 - with the CPU oracle or with a render that has the cache switched off, and every test reads the
cache's own numbers (GpuScene.hit_cache_stats): without them it would prove nothing."""
import numpy as np
import pytest

import scene_builder as sb
import test_camera_update as cu
import test_kernel_resources as kr
from test_prestaged_misses import CAMERA, COUNTERS, assert_same, open_scene, oracle_frame

gpu = pytest.mark.gpu

W, H, SPP, BOUNCES = 160, 96, 4, 5
ITEMS = W * H * SPP   # 61 440: 160 x 96 is whole 32 x 32 tiles
NONE = dict(bytes=0, items=0, cached=0, stores=0, loads=0)


def stats(g):
    return dict(zip(("bytes", "items", "cached", "stores", "loads"), g.hit_cache_stats()))


def full(stores, loads, items=ITEMS):
    return dict(bytes=items * 16, items=items, cached=items, stores=stores, loads=loads)


def uncached(pta, monkeypatch, scene, prof, opts=None):
    """The frame of a fresh scene with the cache switched off."""
    monkeypatch.setenv("PT_HIT_CACHE", "0")
    g = pta.GpuScene(scene)
    out = g.render(prof, opts)
    out = g.render(prof, opts)   # (a second frame of the view: the one that would store)
    assert stats(g) == NONE
    g.close()
    monkeypatch.delenv("PT_HIT_CACHE")
    return out


@gpu
@pytest.mark.parametrize("name,flags", [("point", 0), ("point", 4), ("alpha-five", 0)])
def test_consecutive_frames_load_the_cache_and_equal_the_oracle(pta, oracle, monkeypatch, name, flags):
    """Five frames, an instrumented one and one more.  The fused pipeline on the opaque scene: nothing in frame 0, one word
    fill and one store in frame 1, one load per frame after that; the counters frame casts and leaves the cache alone.
    The KD-tree pipeline and the translucent scene never store and never load.  Same bits everywhere."""
    case, scene = open_scene(name, BOUNCES)
    prof = sb.profile(case, W, H, SPP)
    want = oracle_frame(oracle, scene, prof, walk=True)
    opts = pta.Opts.make(flags=flags)
    used = name == "point" and flags == 0
    assert_same(uncached(pta, monkeypatch, scene, prof, opts), want, (name, flags, "uncached"))
    g = pta.GpuScene(scene)
    for frame in range(5):
        assert_same(g.render(prof, opts), want, (name, flags, frame))
        st = stats(g)
        if not used or frame == 0:
            assert st == NONE, (name, flags, frame, st)
        else:
            assert st == full(1, frame - 1), (name, flags, frame, st)
            assert g.rng_cache_stats()[3] == 1
    before = stats(g)
    got = g.render(prof, pta.Opts.make(flags=flags | pta.PT_FLAG_COUNTERS))
    assert_same(got, want, (name, flags, "counters"))
    c = g.counters().as_dict()
    assert {k: c[k] for k in COUNTERS} == {k: want[2][k] for k in COUNTERS}, (name, flags)
    assert stats(g) == before
    assert_same(g.render(prof, opts), want, (name, flags, "after counters"))
    assert stats(g) == (full(1, 4) if used else NONE)
    g.close()


@gpu
def test_directional_light_variants(pta, oracle):
    """Point and directional lights: the variants with the orthographic branch (15 | 16, 15 | 32) store and load."""
    case, scene = open_scene("five", BOUNCES)
    prof = sb.profile(case, W, H, SPP)
    want = oracle_frame(oracle, scene, prof, walk=True)
    g = pta.GpuScene(scene)
    for frame in range(4):
        assert_same(g.render(prof), want, frame)
        assert stats(g) == (NONE if frame == 0 else full(1, frame - 1)), (frame, stats(g))
    g.close()


@gpu
def test_edits(pta, oracle):
    """Light and material edits keep the view: no new store, the loads go on.  A camera move empties the cache: the next
    frame neither stores nor loads, the one after stores, then loads - and the same again back at the first camera, where a
    stale record would show as a different image.  Every frame is a fresh scene's in that state and the oracle's.  A light
    edit that changes the camera grid's resolution (the light count sets it) starts a new view as a camera move does."""
    case, scene = open_scene("point", BOUNCES)
    prof = sb.profile(case, W, H, SPP)
    cam1 = sb.make_camera(pta, **CAMERA)
    cam2 = sb.make_camera(pta, eye=(-0.9, 2.1, 2.9), target=(0.3, 0.3, -0.4), fov=0.8)
    lights2 = [sb._light(pta, pta.PT_LIGHT_POINT, (-0.8, 2.9, 0.4), (120.0, 130.0, 150.0))]
    mats2 = sb.case_materials(case._replace(factor_set="glow"), pta)
    g = pta.GpuScene(scene)
    want = oracle_frame(oracle, scene, prof)
    for frame in range(3):
        assert_same(g.render(prof), want, ("start", frame))
    assert stats(g) == full(1, 1)
    stores, loads = 1, 1
    seen = [want]

    def check(what, state, new_view):
        nonlocal stores, loads
        fresh_scene = sb.build(case, pta=pta, **state)
        assert not fresh_scene.translucent
        want = oracle_frame(oracle, fresh_scene, prof, walk=True)
        fresh = pta.GpuScene(fresh_scene)
        assert_same(fresh.render(prof), want, (what, "fresh"))
        fresh.close()
        for frame in range(3 if new_view else 2):
            assert_same(g.render(prof), want, (what, frame))
            st = stats(g)
            if new_view and frame == 0:     # neither: the records are another view's, and a first frame never stores
                assert (st["stores"], st["loads"]) == (stores, loads), (what, frame, st)
                continue
            if new_view and frame == 1:
                stores += 1
            else:
                loads += 1
            assert st == full(stores, loads), (what, frame, st)
        assert not np.array_equal(want[1], seen[-1][1]), what   # (the edit changed the image)
        seen.append(want)

    g.set_lights(lights2)
    check("lights", dict(camera=cam1, lights=lights2), False)
    g.set_materials(mats2)
    check("materials", dict(camera=cam1, lights=lights2, materials=mats2), False)
    g.set_camera(cam2)
    check("camera", dict(camera=cam2, lights=lights2, materials=mats2), True)
    g.set_camera(cam1)
    check("first camera again", dict(camera=cam1, lights=lights2, materials=mats2), True)
    res = g.info().cam_grid_res
    lights3 = sb.make_lights(pta, "point_dir")
    g.set_lights(lights3)
    check("light count", dict(camera=cam1, lights=lights3, materials=mats2), g.info().cam_grid_res != res)
    g.close()


@gpu
def test_translucency_stops_the_cache_and_the_return_to_opaque_loads_again(pta, oracle):
    """A material edit that makes the scene translucent: the ALPHA variants run, nothing is stored or loaded.  Back to the
    opaque table the records are still that camera's opaque casts: the first frame loads them again (no new store)."""
    case, scene = open_scene("point", BOUNCES)
    prof = sb.profile(case, W, H, SPP)
    opaque = sb.case_materials(case, pta)
    alpha = sb.case_materials(case._replace(factor_set="alpha"), pta)
    cam = sb.make_camera(pta, **CAMERA)
    want = oracle_frame(oracle, scene, prof)
    alpha_scene = sb.build(case, pta=pta, camera=cam, materials=alpha)
    assert alpha_scene.translucent
    want_alpha = oracle_frame(oracle, alpha_scene, prof, walk=True)
    g = pta.GpuScene(scene)
    for frame in range(3):
        assert_same(g.render(prof), want, ("start", frame))
    assert stats(g) == full(1, 1)
    g.set_materials(alpha)
    for frame in range(2):
        assert_same(g.render(prof), want_alpha, ("translucent", frame))
        assert stats(g) == full(1, 1), (frame, stats(g))
    g.set_materials(opaque)
    for frame in range(2):
        assert_same(g.render(prof), want, ("opaque again", frame))
        assert stats(g) == full(1, 2 + frame), (frame, stats(g))
    g.close()


@gpu
def test_change_of_enumeration(pta, oracle):
    """A A A B B B A A A (B: twice the samples - every jitter differs): the cache follows an enumeration at its second
    consecutive frame, as the word cache does, and loads at the third.  A B A B A B: never allocated.  Same bits."""
    case, scene = open_scene("point", BOUNCES)
    profs = {"A": sb.profile(case, W, H, SPP), "B": sb.profile(case, W, H, 2 * SPP)}
    want = {k: oracle_frame(oracle, scene, p) for k, p in profs.items()}
    items = {"A": ITEMS, "B": 2 * ITEMS}
    g = pta.GpuScene(scene)
    keyed, stores, loads = None, 0, 0
    for n, k in enumerate("AAABBBAAA"):
        assert_same(g.render(profs[k]), want[k], (n, k))
        if n % 3 == 1:
            keyed, stores = k, stores + 1
        elif n % 3 == 2:
            loads += 1
        st = stats(g)
        if keyed is None:
            assert st == NONE, (n, k, st)
        else:   # (the allocation of a larger enumeration is kept for a smaller one: not the bytes)
            assert (st["items"], st["cached"], st["stores"], st["loads"]) == (items[keyed], items[keyed], stores, loads), (n, k, st)
        assert g.rng_cache_stats()[1] == st["items"]
    g.close()
    g = pta.GpuScene(scene)
    for n, k in enumerate("ABABAB"):
        assert_same(g.render(profs[k]), want[k], (n, k))
        assert stats(g) == NONE, (n, k)
    g.close()


@gpu
def test_chunks_sample_batches_and_a_partial_budget(pta, monkeypatch):
    """Small queues: the frame runs in two chunks of one pass over all eight samples, and - sample batches of two - in four
    passes of one chunk each; the cache grows as a prefix over them.  With room for about half of the items the rest casts
    as before.  Same bits as an uncached frame in one pass."""
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
            monkeypatch.setenv("PT_HIT_CACHE_GIB", budget)   # room for 1 006 592 items: two of the four batches
        g = pta.GpuScene(scene)
        loads = 0
        for frame in range(4):
            assert_same(g.render(prof, pta.Opts.make(sample_batch=batch)), one_pass, (budget, batch, frame))
            assert g.info().as_dict()["queue_chunk_items"] < items
            st = stats(g)
            if frame == 0:
                assert st == NONE, st
                continue
            assert st["items"] == items and st["stores"] >= 1, (budget, batch, frame, st)
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
    """Ranks 0 and 1 of 2 with 32 x 32 tiles, a scene each, three frames: each rank's pixels are the unsharded frame's, from
    its own records."""
    case, scene = open_scene("point", BOUNCES)
    prof = sb.profile(case, W, H, SPP)
    want = oracle_frame(oracle, scene, prof)
    cached = 0
    for r in range(2):
        o = pta.Opts.make(shard_rank=r, shard_count=2, tile_w=32, tile_h=32)
        m = pta.local_pixel_map(prof, o)
        g = pta.GpuScene(scene)
        for frame in range(3):
            rgb, acc = g.render(prof, o)
            assert_same((rgb, acc), (want[0][m], want[1][m]), (r, frame))
        st = stats(g)
        assert st == full(1, 1, len(m) * SPP), (r, st)
        cached += st["cached"]
        g.close()
    assert cached == ITEMS


@gpu
def test_frames_in_flight_on_two_streams(pta, oracle):
    """Six frames enqueued without a host wait, alternating between two streams: the second stores on its stream, the third
    loads on the other.  (Each stream waits on the device for the frame before it - the scene's queues are one frame's at a
    time - so this shows that frames in flight on two streams get the right records, not that the library's own wait for
    the store event is needed.)"""
    import torch
    case, scene = open_scene("point", BOUNCES)
    prof = sb.profile(case, W, H, SPP)
    want = oracle_frame(oracle, scene, prof)
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
    assert stats(g) == full(1, 4)
    g.close()


@gpu
@pytest.mark.parametrize("name", ["spheres", "cube"])
def test_record_formats_of_the_golden_scenes(pta, monkeypatch, name):
    """Sphere entry and exit hits (bits 31 and 29 of a record's first word) and back faces (bit 30): four frames of the
    golden scenes equal a render with the cache switched off."""
    prof = pta.Profile.make(96, 64, 4, 3)
    want = uncached(pta, monkeypatch, cu.load(pta, name), prof)
    g = pta.GpuScene(cu.load(pta, name))
    for frame in range(4):
        assert_same(g.render(prof), want, (name, frame))
    assert stats(g) == full(1, 2, 96 * 64 * 4)
    g.close()


@gpu
def test_empty_blocks_and_misses_beside_the_cache(pta, monkeypatch):
    """A small object far from the camera: some 8 x 8 blocks are empty - their wavefronts are culled, they neither store nor
    load - and some samples of the live blocks miss (the "no hit" record)."""
    prof = pta.Profile.make(160, 96, 4, 3)
    host = cu.load(pta, "ps5")
    far = cu.cameras(pta, host)["far"]
    host.set_camera(far)
    want = uncached(pta, monkeypatch, host, prof)
    g = pta.GpuScene(host)
    for frame in range(4):
        assert_same(g.render(prof), want, frame)
    assert stats(g) == full(1, 2, 160 * 96 * 4)
    blocks, empty = g.cull_stats()
    assert_same(g.render(prof, pta.Opts.make(flags=pta.PT_FLAG_COUNTERS)), want, "counters")   # (counts the empty blocks the long way)
    c = g.counters().as_dict()
    assert 0 < empty < blocks, (blocks, empty)
    assert c["samples"] - c["bounce0_hits"] > empty * 64 * 4, (c["samples"], c["bounce0_hits"], empty)   # misses in live blocks
    assert c["bounce0_hits"] > 0
    assert stats(g) == full(1, 2, 160 * 96 * 4)
    g.close()


VARIANTS = {"store": "k_wf_shade_hitsILi27EE", "load": "k_wf_shade_hitsILi43EE",
            "store, directional": "k_wf_shade_hitsILi31EE", "load, directional": "k_wf_shade_hitsILi47EE"}


def test_the_new_variants_keep_four_waves_without_scratch(tmp_path):
    """The four kernels exist; the two of point-light scenes (Li27, Li43) allocate at most 128 registers - four waves per
    SIMD - and at most 16 B of scratch, with the parking array in a quarter of a CU's LDS."""
    t = kr.kernel_table(tmp_path)
    for what, name in VARIANTS.items():
        k = kr.find(t, name)
        print(what, name, k)
        if "directional" not in what:
            assert k["vgpr_count"] <= 128, (what, k)
            assert k["private_segment_fixed_size"] <= 16, (what, k)
            assert k["group_segment_fixed_size"] <= 40960, (what, k)


@gpu
def test_the_runtime_places_four_workgroups_per_cu(pta):
    store, load = pta.kernel_occupancy(2), pta.kernel_occupancy(3)
    print("workgroups per CU: store", store, "load", load)
    assert store >= 4 and load >= 4, (store, load)
