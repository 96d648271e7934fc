"""The scene's cache of bounce-1 shadow visibility (csrc/pt_gpu.hip vis1_cache, csrc/pt_grid_kernels.h k_og_shadow_vis): the
answer of a shadow cast from a bounce-1 hit - og_light_blocked for one shadow record and one light - depends on that hit
(the view, the material table, the item's words: the bounce-1 hit cache's key) and on the light's kind and position, not on
its colour or intensity.  One byte per item keeps it, in the encoding of the bounce-0 cache (two bits per light: 0 unknown,
1 not blocked, 2 blocked), found by the record's slot in its batch's staging area; the variant of k_og_shadow that reads
the byte casts for the lights it finds unknown and writes the byte back.

What could go wrong: a stale bit after a light moved, a material changed or the camera moved; a bit of one light read for
another; the byte of one sample read for another (the slot is not the item: a chunk of a batch sees slots of the whole
batch); a byte beyond the budget; the radiance of a known light computed with other operands than og_light_radiance's; a
long-normal surface losing its way to the off-grid kernel; the plane zeroed on the frame's stream while the side stream
still reads it.  Every frame here is compared bit for bit - f32 accumulator and rgb8 - with the CPU oracle or with a
PT_VIS1_CACHE=0 render of the same sequence, and every test reads the cache's own numbers (GpuScene.vis1_cache_stats).

The variant is launched where bounce 1's shadow records have a launch of their own (k_og_shadow).  Where the frame plan
found nearly every bounce-1 ray reaching a lit surface it casts inside the shade kernel instead, and the cache stays
keyed and unused; none of the scenes here is one of those, as the launch counts show.

Under one key a moot light stays moot - the term that decides it is made of the hit, the material and the light's
direction, all in the key - so, unlike the bounce-0 cache, no edit turns unknown bits of a moot light live without a reset.
A light made black is NOT moot (its term is not zero, its radiance is): it is cast, and the answer is right for the colour
that comes back."""
import numpy as np
import pytest

import scene_builder as sb
import test_kernel_resources as kr
import test_shadow_visibility_cache as v0
from test_prestaged_misses import CAMERA, assert_same, open_scene, oracle_frame

gpu = pytest.mark.gpu

W, H, SPP, BOUNCES = 64, 48, 4, 5
NAMES = ("bytes", "items", "resets", "launches")
NONE = dict.fromkeys(NAMES, 0)
shared = v0.shared


def stats(g):
    return dict(zip(NAMES, g.vis1_cache_stats()))


def hit1_items(g):
    return g.hit1_cache_stats()[1]


def chunks(g):
    """Chunks rendered so far by the frames the bounce-1 hit cache served: each of them stored or loaded."""
    return g.hit1_cache_stats()[4] + g.hit1_cache_stats()[5]


def open_case(lights="point"):
    case, scene = open_scene(lights, BOUNCES)
    return case, scene, sb.profile(case, W, H, SPP)


def steady(g, prof, want, what, frames=5):
    """The frames of a fresh scene: plain, then the one that keys the bounce-1 hits and with them this plane - zeroed once,
    and already filled by that frame's launch - then one launch of the variant per frame (the frame is one chunk), no
    further reset."""
    for frame in range(frames):
        assert_same(g.render(prof), want, (what, frame))
        st = stats(g)
        if frame == 0:
            assert st == NONE, (what, frame, st)
            continue
        assert st["bytes"] == st["items"] == hit1_items(g) > 0, (what, frame, st)
        assert (st["resets"], st["launches"]) == (1, frame), (what, frame, st)


@gpu
@pytest.mark.parametrize("name", ["spheres", "cube", "reflection", "open"])
def test_consecutive_frames(pta, oracle, scene_cache, name):
    """Five frames.  spheres: four point lights, all four bit pairs; open: the builder's scene, whose floor has normals too long
    for the light grids - those records go to the off-grid kernel beside the cache."""
    if name == "open":
        assert v0.long_normals(pta) > 0
        _, scene, prof = open_case()
    else:
        scene = scene_cache(name)
        prof = pta.Profile.make(W, H, SPP, 3)
    want = shared(("steady", name), lambda: oracle_frame(oracle, scene, prof))
    g = pta.GpuScene(scene)
    assert not g.info().has_translucent
    steady(g, prof, want, name)
    g.close()


@gpu
def test_edits(pta, oracle):
    """A colour edit keeps the plane: no reset, the launches go on, the image is the oracle's for the new colour.  A moved
    light whose shadows fall elsewhere, a second light, a material edit, a camera move: the next frame launches the plain
    kernel, the one after zeroes the plane and launches the variant.  Back at the first state the same again - a stale bit
    would show as another image."""
    case, scene, prof = open_case()
    P = pta.PT_LIGHT_POINT
    cam1 = sb.make_camera(pta, **CAMERA)
    cam2 = sb.make_camera(pta, eye=(-0.9, 2.1, 2.9), target=(0.3, 0.3, -0.4), fov=0.8)
    lights1 = sb.make_lights(pta, "point")
    recoloured = [sb._light(pta, P, tuple(lights1[0].vec), (20.0, 170.0, 90.0))]
    brighter = [sb._light(pta, P, tuple(lights1[0].vec), (60.0, 510.0, 270.0))]
    moved = [sb._light(pta, P, (-0.8, 2.9, 0.4), (60.0, 510.0, 270.0))]
    two = moved + [sb._light(pta, P, (-1.0, 3.0, 0.2), (60.0, 20.0, 90.0))]
    table1 = sb.case_materials(case, pta)
    rough = sb.case_materials(case, pta)
    for m in rough:
        m.roughness = min(1.0, 0.37 + 0.5 * m.roughness)
    first = shared(("steady", "open"), lambda: oracle_frame(oracle, scene, prof))
    g = pta.GpuScene(scene)
    steady(g, prof, first, "start", frames=4)
    resets, launches = 1, 3
    seen = [first]
    KEPT, REKEYED = [(0, 1), (0, 1)], [(0, 0), (1, 1), (0, 1)]

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
    check("colour", dict(camera=cam1, lights=recoloured), KEPT)
    g.set_lights(brighter)
    check("intensity", dict(camera=cam1, lights=brighter), KEPT)
    g.set_lights(moved)
    check("moved", dict(camera=cam1, lights=moved), REKEYED)
    g.set_lights(two)
    check("two lights", dict(camera=cam1, lights=two), REKEYED)
    g.set_materials(rough)
    check("materials", dict(camera=cam1, lights=two, materials=rough), REKEYED)
    g.set_camera(cam2)
    check("camera", dict(camera=cam2, lights=two, materials=rough), REKEYED)
    g.set_camera(cam1)
    g.set_materials(table1)
    g.set_lights(lights1)
    check("first state", dict(camera=cam1, lights=lights1), REKEYED)
    assert np.array_equal(seen[-1][1], first[1])
    g.close()


@gpu
def test_a_light_made_black_and_lit_again(pta, oracle):
    """Two point lights; the second turns black - a colour edit: the plane stays - and comes back with another colour.  While
    it is black its radiance is zero and its term is not: the casts are made and kept, and what was found holds for the new
    colour.  No reset in between, every frame the oracle's."""
    case, _, prof = open_case()
    P = pta.PT_LIGHT_POINT
    cam = sb.make_camera(pta, **CAMERA)
    a = sb._light(pta, P, (-0.8, 2.9, 0.4), (20.0, 170.0, 90.0))
    pos_b = (-1.0, 3.0, 0.2)
    sets = [("lit", [a, sb._light(pta, P, pos_b, (60.0, 20.0, 90.0))]), ("black", [a, sb._light(pta, P, pos_b, (0.0, 0.0, 0.0))]),
            ("lit again", [a, sb._light(pta, P, pos_b, (90.0, 80.0, 10.0))])]
    g = pta.GpuScene(sb.build(case, pta=pta, camera=cam, lights=sets[0][1]))
    launches, images = 0, []
    for k, (what, lights) in enumerate(sets):
        if k:
            g.set_lights(lights)
        want = oracle_frame(oracle, sb.build(case, pta=pta, camera=cam, lights=lights), prof, walk=True)
        images.append(want[1])
        for frame in range(4 if k == 0 else 2):
            assert_same(g.render(prof), want, (what, frame))
            launches += (k, frame) != (0, 0)
            assert (stats(g)["resets"], stats(g)["launches"]) == (0 if (k, frame) == (0, 0) else 1, launches), (what, frame, stats(g))
    assert not np.array_equal(images[0], images[1]) and not np.array_equal(images[1], images[2])
    g.close()


@gpu
def test_five_lights_and_a_directional_light(pta, oracle):
    """Five lights: the byte has room for four - the cache is not used, its numbers stand still.  A point and a directional
    light: the variant with the orthographic branch, equal to the oracle."""
    case, scene, prof = open_case()
    cam = sb.make_camera(pta, **CAMERA)
    first = shared(("steady", "open"), lambda: oracle_frame(oracle, scene, prof))
    g = pta.GpuScene(scene)
    steady(g, prof, first, "start", frames=3)
    for name in ("five", "point_dir"):
        lights = sb.make_lights(pta, name)
        g.set_lights(lights)
        want = oracle_frame(oracle, sb.build(case, pta=pta, camera=cam, lights=lights), prof, walk=True)
        before = stats(g)
        for frame in range(4):
            assert_same(g.render(prof), want, (name, frame))
        st = stats(g)
        if name == "five":
            assert st == before, (before, st)
        else:   # nothing, then zeroed and launched, then launched
            assert (st["resets"], st["launches"]) == (before["resets"] + 1, before["launches"] + 3), (before, st)
    g.close()
    lights = sb.make_lights(pta, "point_dir")   # ... and from a scene's first frame on
    scene = sb.build(case, pta=pta, camera=cam, lights=lights)
    g = pta.GpuScene(scene)
    steady(g, prof, oracle_frame(oracle, scene, prof, walk=True), "point_dir")
    g.close()


@gpu
def test_switched_off(pta, oracle, monkeypatch):
    """PT_VIS1_CACHE=0: same bits, nothing allocated; switched on: keyed at once; switched off on a scene that has a plane:
    released, and the bounce-1 hit cache goes on loading."""
    _, scene, prof = open_case()
    want = shared(("steady", "open"), lambda: oracle_frame(oracle, scene, prof))
    monkeypatch.setenv("PT_VIS1_CACHE", "0")
    g = pta.GpuScene(scene)
    for frame in range(4):
        assert_same(g.render(prof), want, ("off", frame))
        assert stats(g) == NONE
    monkeypatch.delenv("PT_VIS1_CACHE")
    for frame in range(3):   # (the frame before had this key: keyed at once)
        assert_same(g.render(prof), want, ("on", frame))
        assert (stats(g)["resets"], stats(g)["launches"]) == (1, 1 + frame), (frame, stats(g))
    loads = g.hit1_cache_stats()[5]
    monkeypatch.setenv("PT_VIS1_CACHE", "0")
    for frame in range(2):
        assert_same(g.render(prof), want, ("off again", frame))
        st = stats(g)
        assert (st["bytes"], st["items"], st["resets"], st["launches"]) == (0, 0, 1, 3), (frame, st)
    assert g.hit1_cache_stats()[5] == loads + 2
    g.close()


@gpu
def test_chunks_sample_batches_and_a_partial_budget(pta, monkeypatch):
    """Small queues: two chunks of one pass - both read slots of the whole batch - and, sample batches of two, four passes of
    one chunk each.  With room for about half of the items the batches above the plane's stride run the plain kernel.  Same
    bits as a frame with the cache switched off, in one pass."""
    case, scene = open_scene("point", BOUNCES)
    w, h, spp = 640, 360, 8
    items = 640 * 384 * spp   # 1 966 080 (32 x 32 tiles)
    prof = sb.profile(case, w, h, spp)
    monkeypatch.setenv("PT_VIS1_CACHE", "0")
    g = pta.GpuScene(scene)
    one_pass = [g.render(prof) for _ in range(3)][-1]
    assert stats(g) == NONE
    g.close()
    monkeypatch.delenv("PT_VIS1_CACHE")
    monkeypatch.setenv("PT_QUEUE_GIB", "0.01")
    monkeypatch.setenv("PT_QUEUE_STEADY_GIB", "0.02")
    monkeypatch.setenv("PT_QUEUE_ONE_PASS_GIB", "0.02")
    for budget, batch in ((None, 0), (None, 2), ("0.00095", 2)):
        if budget:
            monkeypatch.setenv("PT_VIS1_CACHE_GIB", budget)   # room for 1 020 032 items: two of the four batches
        g = pta.GpuScene(scene)
        for frame in range(4):
            l0, c0 = stats(g)["launches"], chunks(g)
            assert_same(g.render(prof, pta.Opts.make(sample_batch=batch)), one_pass, (budget, batch, frame))
            assert g.info().as_dict()["queue_chunk_items"] < items
            st = stats(g)
            dl, dc = st["launches"] - l0, chunks(g) - c0
            if frame == 0:
                assert st == NONE, st
                continue
            assert st["items"] == items and st["resets"] == 1 and st["bytes"] == (1020032 if budget else items), (budget, batch, frame, st)
            if budget is None:
                assert dl == dc >= 2, (batch, frame, st, dl, dc)
            else:   # the batches below the stride take the variant, the others the plain kernel
                assert 0 < dl < dc, (frame, st, dl, dc)
        g.close()


@gpu
def test_a_frame_on_a_second_stream_after_a_rekey(pta, oracle):
    """Frames enqueued without a host wait, alternating between two streams, a moved light in the middle: the plane is read and
    filled on the side stream of one frame, zeroed for the new key on the stream of a later one and read again from the
    other.  Every frame the oracle's for its light."""
    import torch
    case, scene, prof = open_case()
    moved = [sb._light(pta, pta.PT_LIGHT_POINT, (-0.8, 2.9, 0.4), (20.0, 170.0, 90.0))]
    want = [shared(("steady", "open"), lambda: oracle_frame(oracle, scene, prof)),
            oracle_frame(oracle, sb.build(case, pta=pta, camera=sb.make_camera(pta, **CAMERA), lights=moved), prof, walk=True)]
    n = W * H
    outs = [(torch.empty(n * 3, dtype=torch.uint8, device="cuda"), torch.empty(n * 3, dtype=torch.float32, device="cuda")) for _ in range(9)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    g = pta.GpuScene(scene)
    for k, (rgb, acc) in enumerate(outs):
        if k == 4:
            g.set_lights(moved)
        st = streams[k & 1]
        st.wait_stream(streams[(k & 1) ^ 1])
        g.render_device(prof, pta.Opts.make(), rgb.data_ptr(), acc.data_ptr(), st.cuda_stream)
    for st in streams:
        st.synchronize()
    for k, (rgb, acc) in enumerate(outs):
        assert_same((rgb.cpu().numpy().reshape(-1, 3), acc.cpu().numpy().reshape(-1, 3)), want[k >= 4], k)
    assert (stats(g)["resets"], stats(g)["launches"]) == (2, 3 + 4), stats(g)   # frames 1-3, then 5-8
    g.close()


def test_the_kernel_keeps_eight_waves_without_scratch(tmp_path):
    """The built library's record of k_og_shadow_vis (point lights only): at most 64 vector registers - k_og_shadow's
    occupancy class - and no scratch."""
    t = kr.kernel_table(tmp_path)
    k = kr.find(t, "k_og_shadow_visILb0EE")
    print(k)
    assert k["vgpr_count"] <= 64 and k["private_segment_fixed_size"] == 0, k
