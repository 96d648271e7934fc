"""The scene's cache of bounce-0 shadow visibility (csrc/pt_gpu.hip VisCache, csrc/pt_wavefront.h k_wf_shade_hits<.. | 64>): in
an opaque scene the answer of a bounce-0 shadow cast - og_blocked for one work item and one light - depends on the item's
camera hit, the light's kind and position and the geometry, not on the materials, the light's colour or the bounces.  One
byte per item keeps it, two bits per light (0 unknown, 1 not blocked, 2 blocked); the variant of the bounce-0 kernel that
loads the camera hits reads the byte, casts for the lights it finds unknown and writes the byte back.

What could go wrong: a stale bit after a light or the camera moved, a bit of one light read for another, a moot light's
unknown bits taken for "not blocked" once a material edit makes the light live, a byte read beyond the budget or by another
shard, a translucent frame taking the opaque answer, the radiance of a known light computed with other operands than
og_light_radiance's, a frame on another stream reading before the plane was zeroed.  Every frame here is compared bit for
bit - f32 accumulator and rgb8 - with the CPU oracle or with a PT_VIS_CACHE=0 render of the same sequence, and every test
reads the cache's own numbers (GpuScene.vis_cache_stats): without them it would prove nothing."""
import numpy as np
import pytest

import scene_builder as sb
import test_kernel_resources as kr
from test_prestaged_misses import CAMERA, assert_same, open_scene, oracle_frame

gpu = pytest.mark.gpu

W, H, SPP, BOUNCES = 64, 48, 4, 5
NONE = dict(bytes=0, items=0, resets=0, launches=0)


def stats(g):
    return dict(zip(("bytes", "items", "resets", "launches"), g.vis_cache_stats()))


def hit_loads(g):
    return g.hit_cache_stats()[4]


_frames = {}


def shared(key, make):
    """A reference frame, made once, shared and left unchanged."""
    if key not in _frames:
        out = make()
        for a in out[:2]:
            a.setflags(write=False)
        _frames[key] = out
    return _frames[key]


def steady(g, prof, want, what, frames=6, opts=None):
    """The frames of a fresh scene: plain, then the one that stores the hits and zeroes the plane, then the filling launch,
    then the reading ones - one launch of the variant per frame (the frame is one chunk)."""
    for frame in range(frames):
        assert_same(g.render(prof, opts), want, (what, frame))
        st = stats(g)
        if frame == 0:
            assert st == NONE, (what, frame, st)
        else:
            assert st["bytes"] == st["items"] > 0 and st["items"] == g.hit_cache_stats()[1], (what, frame, st)
            assert (st["resets"], st["launches"]) == (1, max(0, frame - 1)), (what, frame, st)
            assert hit_loads(g) == st["launches"], (what, frame)


def long_normals(pta):
    """Corner normals of the `open` geometry longer than the light grids' margin covers (|n|^2 > 1.5^2: such a surface takes
    the shadow queue, beside the cache)."""
    tris, _ = sb.make_geometry(pta, "open")
    t = np.asarray(tris, np.float32).reshape(len(tris), 3, 8)
    return int(((t[:, :, 3:6] ** 2).sum(axis=2) > 2.25).sum())


@gpu
@pytest.mark.parametrize("name", ["spheres", "cube", "reflection", "open"])
def test_consecutive_frames(pta, oracle, scene_cache, name):
    """Six frames.  spheres: sphere occluders and four point lights (all four bit pairs); cube and reflection: a black
    background (reflection: two meshes that shadow each other); open: the builder's scene, whose floor has normals too long
    for the grids - those surfaces take the shadow queue beside the cache.  (The golden scene with a directional light,
    head, has an opacity texture: it is translucent and never uses the cache; test_directional_lights_... has variant 111.)"""
    if name == "open":
        assert long_normals(pta) > 0
        case, scene = open_scene("point", BOUNCES)
        prof = sb.profile(case, W, H, SPP)
    else:
        scene = scene_cache(name)
        prof = pta.Profile.make(W, H, SPP, 3)
        if name in ("cube", "reflection"):
            assert list(scene.desc.contents.background) == [0.0, 0.0, 0.0]
    want = shared(("steady", name), lambda: oracle_frame(oracle, scene, prof))
    g = pta.GpuScene(scene)
    assert not g.info().has_translucent
    steady(g, prof, want, name)
    g.close()


def skipped(pta, scene, prof, want):
    """Lights the kernels skipped as moot in one instrumented frame."""
    g = pta.GpuScene(scene)
    assert_same(g.render(prof, pta.Opts.make(flags=pta.PT_FLAG_COUNTERS)), want, "counters")
    n = g.counters().as_dict()["shadow_skipped"]
    g.close()
    return n


@gpu
def test_a_moot_light_becomes_live(pta, oracle):
    """ct_eval_direct is diffuse + specular + EMISSIVE: on a surface that faces away from the light the first two are exactly
    zero, so without emission the light is moot there - skipped, its bits left unknown while four frames fill and read the
    plane.  The `glow` table makes the wall, the panel and the ball emissive: the term is the emission, the light is live,
    the lanes find `unknown`, cast and fill - same bits as the oracle, and no reset.  (The premise, from instrumented
    frames: lights are skipped under the first table, fewer under the second.)"""
    case, scene = open_scene("point", BOUNCES)
    prof = sb.profile(case, W, H, SPP)
    glow = sb.case_materials(case._replace(factor_set="glow"), pta)
    glow_scene = sb.build(case, pta=pta, camera=sb.make_camera(pta, **CAMERA), materials=glow)
    assert not glow_scene.translucent
    want = shared(("steady", "open"), lambda: oracle_frame(oracle, scene, prof))
    want_glow = oracle_frame(oracle, glow_scene, prof, walk=True)
    assert not np.array_equal(want[1], want_glow[1])
    n_first, n_glow = skipped(pta, scene, prof, want), skipped(pta, glow_scene, prof, want_glow)
    print("lights skipped as moot:", n_first, "with emission:", n_glow)
    assert n_first > n_glow >= 0 and n_first > 0, (n_first, n_glow)
    g = pta.GpuScene(scene)
    steady(g, prof, want, "first table", frames=4)
    g.set_materials(glow)
    for frame in range(3):
        assert_same(g.render(prof), want_glow, ("glow", frame))
        assert stats(g)["resets"] == 1 and stats(g)["launches"] == 3 + frame, (frame, stats(g))
    g.close()


@gpu
def test_edits(pta, oracle):
    """A colour-only light edit keeps the plane: no reset, the launches go on.  A moved light: the next frame runs no launch
    of the variant, the one after zeroes the plane and launches (the hits are still loaded).  A camera move: nothing in the
    next frame, the one after stores the hits and zeroes the plane, the third launches.  Back at the first camera and
    light the same again - a stale bit would show as another image.  Light counts 2, 5, 1: no launch with five."""
    case, scene = open_scene("point", BOUNCES)
    prof = sb.profile(case, W, H, SPP)
    P = pta.PT_LIGHT_POINT
    cam1 = sb.make_camera(pta, **CAMERA)
    cam2 = sb.make_camera(pta, eye=(-0.9, 2.1, 2.9), target=(0.3, 0.3, -0.4), fov=0.8)
    lights1 = sb.make_lights(pta, "point")
    recoloured = [sb._light(pta, P, tuple(lights1[0].vec), (20.0, 170.0, 90.0))]
    moved = [sb._light(pta, P, (-0.8, 2.9, 0.4), (20.0, 170.0, 90.0))]
    first = shared(("steady", "open"), lambda: oracle_frame(oracle, scene, prof))
    g = pta.GpuScene(scene)
    steady(g, prof, first, "start", frames=4)
    resets, launches = 1, 2
    seen = [first]

    def check(what, state, deltas):
        """deltas: per frame, (planes zeroed, launches of the variant)."""
        nonlocal resets, launches
        want = oracle_frame(oracle, sb.build(case, pta=pta, **state), prof, walk=True)
        for frame, (dr, dl) in enumerate(deltas):
            assert_same(g.render(prof), want, (what, frame))
            resets, launches = resets + dr, launches + dl
            assert (stats(g)["resets"], stats(g)["launches"]) == (resets, launches), (what, frame, stats(g))
        assert not np.array_equal(want[1], seen[-1][1]), what   # (the edit changed the image)
        seen.append(want)

    g.set_lights(recoloured)
    check("colour", dict(camera=cam1, lights=recoloured), [(0, 1), (0, 1)])
    g.set_lights(moved)
    check("moved", dict(camera=cam1, lights=moved), [(0, 0), (1, 1), (0, 1)])
    g.set_camera(cam2)
    check("camera", dict(camera=cam2, lights=moved), [(0, 0), (1, 0), (0, 1), (0, 1)])
    g.set_camera(cam1)
    g.set_lights(lights1)
    check("first camera and light", dict(camera=cam1, lights=lights1), [(0, 0), (1, 0), (0, 1), (0, 1)])
    assert np.array_equal(seen[-1][1], first[1])
    for name in ("point_dir", "five", "point"):
        lights = sb.make_lights(pta, name)
        g.set_lights(lights)
        want = oracle_frame(oracle, sb.build(case, pta=pta, camera=cam1, lights=lights), prof, walk=True)
        before = stats(g)["launches"]
        for frame in range(4):
            assert_same(g.render(prof), want, (name, frame))
        assert (stats(g)["launches"] == before) == (name == "five"), (name, before, stats(g))
    g.close()


@gpu
def test_directional_lights_and_all_four_bit_pairs(pta, oracle):
    """Two point and two directional lights: variant 111, every bit pair of the byte in use."""
    case, _ = open_scene("point", BOUNCES)
    P, D = pta.PT_LIGHT_POINT, pta.PT_LIGHT_DIRECTIONAL
    lights = [sb._light(pta, D, 10.0 * sb._unit([-0.3, -0.9, -0.25]), (0.5, 0.6, 0.7)), sb.make_lights(pta, "point")[0],
              sb._light(pta, D, sb._unit([0.5, -0.7, 0.2]), (0.3, 0.2, 0.4)), sb._light(pta, P, (-1.0, 3.0, 0.2), (60.0, 20.0, 90.0))]
    scene = sb.build(case, pta=pta, camera=sb.make_camera(pta, **CAMERA), lights=lights)
    prof = sb.profile(case, W, H, SPP)
    g = pta.GpuScene(scene)
    steady(g, prof, oracle_frame(oracle, scene, prof, walk=True), "four lights")
    g.close()


@gpu
def test_translucency_stops_the_cache_and_the_return_to_opaque_reads_it(pta, oracle):
    case, scene = open_scene("point", BOUNCES)
    prof = sb.profile(case, W, H, SPP)
    opaque = sb.case_materials(case, pta)
    alpha = sb.case_materials(case._replace(factor_set="alpha"), pta)
    alpha_scene = sb.build(case, pta=pta, camera=sb.make_camera(pta, **CAMERA), materials=alpha)
    assert alpha_scene.translucent
    want = shared(("steady", "open"), lambda: oracle_frame(oracle, scene, prof))
    want_alpha = oracle_frame(oracle, alpha_scene, prof, walk=True)
    g = pta.GpuScene(scene)
    steady(g, prof, want, "start", frames=4)
    before = stats(g)
    g.set_materials(alpha)
    for frame in range(2):
        assert_same(g.render(prof), want_alpha, ("translucent", frame))
        assert stats(g) == before, (frame, stats(g))
    g.set_materials(opaque)
    for frame in range(2):
        assert_same(g.render(prof), want, ("opaque again", frame))
        assert stats(g) == dict(before, launches=before["launches"] + 1 + frame), (frame, stats(g))
    g.close()


@gpu
def test_chunks_sample_batches_and_a_partial_budget(pta, monkeypatch):
    """Small queues: two chunks of one pass, and - sample batches of two - four passes of one chunk each.  With room for
    about half of the items the chunks above the plane's stride run the plain loading variant.  Same bits as a frame with
    the cache switched off, in one pass."""
    case, scene = open_scene("point", BOUNCES)
    w, h, spp = 640, 360, 8
    items = 640 * 384 * spp   # 1 966 080 (32 x 32 tiles)
    prof = sb.profile(case, w, h, spp)
    monkeypatch.setenv("PT_VIS_CACHE", "0")
    g = pta.GpuScene(scene)
    one_pass = [g.render(prof) for _ in range(4)][-1]
    assert stats(g) == NONE and hit_loads(g) == 2
    g.close()
    monkeypatch.delenv("PT_VIS_CACHE")
    monkeypatch.setenv("PT_QUEUE_GIB", "0.01")
    monkeypatch.setenv("PT_QUEUE_STEADY_GIB", "0.02")
    monkeypatch.setenv("PT_QUEUE_ONE_PASS_GIB", "0.02")
    for budget, batch in ((None, 0), (None, 2), ("0.00095", 2)):
        if budget:
            monkeypatch.setenv("PT_VIS_CACHE_GIB", budget)   # room for 1 020 032 items: two of the four batches
        g = pta.GpuScene(scene)
        for frame in range(5):
            l0, h0 = stats(g)["launches"], hit_loads(g)
            assert_same(g.render(prof, pta.Opts.make(sample_batch=batch)), one_pass, (budget, batch, frame))
            assert g.info().as_dict()["queue_chunk_items"] < items
            st = stats(g)
            dl, dh = st["launches"] - l0, hit_loads(g) - h0
            if frame < 2:
                assert dl == 0, (budget, batch, frame, st)
                continue
            assert st["items"] == items and st["resets"] == 1, (budget, batch, frame, st)
            if budget is None:
                assert st["bytes"] == items and dl == dh > 0, (batch, frame, st, dl, dh)
            else:   # the batches below the stride take the variant, the others load their hits and cast
                assert st["bytes"] == 1020032 and 0 < dl < dh, (frame, st, dl, dh)
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
        for frame in range(5):
            rgb[m], acc[m] = g.render(prof, o)
        assert stats(g) == dict(bytes=len(m) * SPP, items=len(m) * SPP, resets=1, launches=3), (r, stats(g))
        g.close()
    assert_same((rgb, acc), want, "assembled")


@gpu
def test_frames_in_flight_on_two_streams(pta, oracle):
    """Six frames enqueued without a host wait, alternating between two streams: the plane is zeroed on one stream and filled
    on the other."""
    import torch
    case, scene = open_scene("point", BOUNCES)
    prof = sb.profile(case, W, H, SPP)
    want = shared(("steady", "open"), lambda: oracle_frame(oracle, scene, prof))
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
    assert (stats(g)["resets"], stats(g)["launches"]) == (1, 4) and hit_loads(g) == 4, stats(g)
    g.close()


@gpu
def test_switched_off(pta, oracle, monkeypatch):
    """PT_VIS_CACHE=0: same bits, nothing allocated; switched off on a scene that has a plane: released."""
    case, scene = open_scene("point", BOUNCES)
    prof = sb.profile(case, W, H, SPP)
    want = shared(("steady", "open"), lambda: oracle_frame(oracle, scene, prof))
    monkeypatch.setenv("PT_VIS_CACHE", "0")
    g = pta.GpuScene(scene)
    for frame in range(4):
        assert_same(g.render(prof), want, ("off", frame))
        assert stats(g) == NONE
    assert hit_loads(g) == 2
    monkeypatch.delenv("PT_VIS_CACHE")
    steady_from = stats(g)
    for frame in range(3):   # (the frame before had this key: keyed at once)
        assert_same(g.render(prof), want, ("on", frame))
    assert stats(g)["bytes"] > 0 and stats(g)["launches"] == 3 and steady_from == NONE
    monkeypatch.setenv("PT_VIS_CACHE", "0")
    assert_same(g.render(prof), want, "off again")
    assert stats(g)["bytes"] == 0 and stats(g)["items"] == 0
    g.close()


VARIANTS = {"k_wf_shade_hitsILi107EE": "k_wf_shade_hitsILi43EE", "k_wf_shade_hitsILi111EE": "k_wf_shade_hitsILi47EE"}


def test_the_variants_keep_four_waves_and_the_scratch_of_the_loading_ones(tmp_path):
    t = kr.kernel_table(tmp_path)
    for name, plain in VARIANTS.items():
        k, p = kr.find(t, name), kr.find(t, plain)
        print(name, k, plain, p)
        assert k["vgpr_count"] <= 128, (name, k)
        assert k["private_segment_fixed_size"] <= p["private_segment_fixed_size"], (name, k, p)
        assert k["group_segment_fixed_size"] <= 40960, (name, k)


@gpu
def test_the_runtime_places_four_workgroups_per_cu(pta):
    point, directional = pta.kernel_occupancy(4), pta.kernel_occupancy(5)
    print("workgroups per CU: 107", point, "111", directional)
    assert point >= 4 and directional >= 4, (point, directional)
