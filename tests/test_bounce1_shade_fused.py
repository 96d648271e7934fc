"""The bounce-1 shade pass that reads the bounce-1 shadow visibility and the bounce-2 hit cache itself (csrc/pt_wavefront.h
k_wf_shade_fused, GRIDX 256 and 256 | 512; csrc/pt_gpu.hip Chunk::b1_fused).  In a chunk whose sample batch has visibility bytes
the pass looks a hit's byte up by the record's out_slot: where every live light has known bits it adds them itself, in light
order, and writes no shadow record - the colour is final, the miss is staged there, the escape-mask rule ends the path there;
any other hit goes to the shadow queue whole and k_og_shadow_vis casts, fills the byte and retires it.  Where the chunk loads
its bounce-2 hits the same launch answers its survivors' casts from that plane, as the bounce-0 kernel does one bounce earlier:
k_wf_hits_load is not launched at bounce 2.

What could go wrong: lights added in another order or with other operands than k_og_shadow_vis's, a record added in part, a
stale bit or a stale record after an edit, a path ended by the escape masks before its lights were in its colour, an item
that reaches bounce 2 in one frame and not in the frame that stored the plane taken for a miss, the bounce-2 hits written
into the plane the launch is still reading, a frame plan counted in a frame that inlines and elides too short for one that
does not.  Every frame here is compared bit for bit - rgb8 and f32 accumulator - with the CPU oracle or with a render of the
same sequence with the two switches off, and every test reads the variant's own numbers (GpuScene.bounce1_fused_stats)."""
import numpy as np
import pytest

import scene_builder as sb
import test_bounce1_hit_cache as h1
import test_bounce1_shadow_visibility_cache as v1
import test_bounce2_hit_cache as h2
from test_bounce1_hit_cache import BOUNCES, H, SPP, W, open_case, open_want, shared
from test_bounce1_hits_fused import fused as fused0
from test_kernel_resources import find, kernel_table
from test_prestaged_misses import CAMERA, assert_same, open_scene, oracle_frame

gpu = pytest.mark.gpu

NAMES = ("launches", "inlined", "deferred", "next_written", "next_elided", "next_unknown")
ZERO = dict.fromkeys(NAMES, 0)
SWITCHES = ("PT_VIS1_FUSED", "PT_HIT2_FUSED")


@pytest.fixture(autouse=True)
def both_steps(monkeypatch):
    """Step A ships on and step B off (profiles/r16_experiments.txt item 3): the tests here run both unless they say otherwise."""
    for k in SWITCHES:
        monkeypatch.setenv(k, "1")


def fused(g):
    return dict(zip(NAMES, g.bounce1_fused_stats()))


def delta(after, before):
    return {k: after[k] - before[k] for k in NAMES}


def frames(g, prof, want, what, n, opts=None):
    """n frames, each `want`: what each added to the variant's numbers."""
    out = []
    for frame in range(n):
        before = fused(g)
        assert_same(g.render(prof, opts) if opts else g.render(prof), want, (what, frame))
        out.append(delta(fused(g), before))
    return out


def steady(g, prof, want, what, n=5, lit=True):
    """The frames of a fresh scene (one chunk each): plain; then the one that keys the planes - the variant runs, finds every
    bit unknown and defers every record, and stores the bounce-2 hits of all of them; then the ones that add the lights
    themselves and read the bounce-2 plane - the same numbers every frame.  Returns one such frame's.  lit=False: no bounce-1
    hit of the scene has a live light, so there is no shadow record either way."""
    got = frames(g, prof, want, what, n)
    assert got[0] == ZERO, (what, got[0])
    assert got[1]["launches"] == 1 and got[1]["inlined"] == 0 and (got[1]["deferred"] > 0) == lit, (what, got[1])
    assert got[1]["next_written"] == got[1]["next_unknown"] == 0, (what, got[1])
    for d in got[2:]:
        assert d == got[2] and d["launches"] == 1 and (d["inlined"] > 0) == lit and d["next_unknown"] == 0, (what, got)
        assert d["inlined"] + d["deferred"] == got[1]["deferred"], (what, got)   # (the same shadow records, one way or the other)
    assert v1.stats(g)["launches"] == n - 1 and v1.stats(g)["resets"] == 1, (what, v1.stats(g))   # (k_og_shadow_vis still runs)
    return got[2]


@gpu
@pytest.mark.parametrize("name", ["spheres", "cube", "reflection", "open"])
def test_consecutive_frames(pta, oracle, scene_cache, name):
    """From the frame after keying on, one launch of the variant per frame.  spheres: four point lights, all bit pairs.  open:
    the floor's normals are too long for the light grids - their bytes never fill, their records are deferred in every frame;
    cube has none.  The caches count as their own tests expect."""
    if name == "open":
        assert v1.v0.long_normals(pta) > 0
        _, scene, prof = open_case()
        want = open_want(oracle, scene, prof)
    else:
        scene = scene_cache(name)
        prof = pta.Profile.make(W, H, SPP, 3)
        want = shared(("steady", name), lambda: oracle_frame(oracle, scene, prof))
    g = pta.GpuScene(scene)
    d = steady(g, prof, want, name, lit=name != "cube")   # (the cube's bounce-1 hits see no light)
    print(name, d)
    if name == "open":
        assert d["deferred"] > 0 and d["next_elided"] > 0 and d["next_written"] > 0, d
    if name == "cube":
        assert d["deferred"] == 0, d
    s1, s2 = h2.stats(g)   # (no path of the cube has a bounce-2 ray: that plane is keyed and never stored, as in its own test)
    assert h2.counts(s1) == (1, 1, 3) and h2.counts(s2) == ((1, 1, 3) if name != "cube" else (1, 0, 0)) and s2["unknown"] == 0, (s1, s2)
    assert fused0(g)["launches"] == 3, fused0(g)
    g.close()


@gpu
def test_edits_under_a_live_scene(pta, oracle):
    """A light recoloured, brightened, made black (not moot: its term is not zero): the plane is kept, the variant goes on
    adding the lights, the image is the oracle's for the new colour.  A moved light: a frame without a plane (k_wf_shade),
    one that defers everything, then the lights are added again.  A material edit and a camera move re-key the hits too.
    Back at the first state a stale bit or a stale record would show as another image."""
    case, scene, prof = open_case()
    P = pta.PT_LIGHT_POINT
    cam1 = sb.make_camera(pta, **CAMERA)
    cam2 = sb.make_camera(pta, eye=(-0.9, 2.1, 2.9), target=(0.3, 0.3, -0.4), fov=0.8)
    lights1 = sb.make_lights(pta, "point")
    pos = tuple(lights1[0].vec)
    recoloured, brighter, black = ([sb._light(pta, P, pos, c)] for c in ((20.0, 170.0, 90.0), (60.0, 510.0, 270.0), (0.0, 0.0, 0.0)))
    moved = [sb._light(pta, P, (-0.8, 2.9, 0.4), (60.0, 510.0, 270.0))]
    table1 = sb.case_materials(case, pta)
    rough = sb.case_materials(case, pta)
    for m in rough:
        m.roughness = min(1.0, 0.37 + 0.5 * m.roughness)
    first = open_want(oracle, scene, prof)
    g = pta.GpuScene(scene)
    per_frame = steady(g, prof, first, "start", n=4)

    def check(what, state, kept):
        want = oracle_frame(oracle, sb.build(case, pta=pta, **state), prof, walk=True)
        got = frames(g, prof, want, what, 2 if kept else 4)
        if kept:   # the plane and the records stay: the numbers of a steady frame
            assert got == [per_frame] * 2, (what, got, per_frame)
        else:
            assert got[0] == ZERO, (what, got)
            assert got[1]["launches"] == 1 and got[1]["inlined"] == 0 and got[1]["deferred"] > 0, (what, got)
            assert got[2] == got[3] and got[2]["inlined"] > 0 and got[2]["inlined"] + got[2]["deferred"] == got[1]["deferred"], (what, got)
        return want

    g.set_lights(recoloured)
    a = check("colour", dict(camera=cam1, lights=recoloured), True)
    g.set_lights(brighter)
    b = check("intensity", dict(camera=cam1, lights=brighter), True)
    g.set_lights(black)
    c = check("black", dict(camera=cam1, lights=black), True)
    assert not np.array_equal(a[1], b[1]) and not np.array_equal(b[1], c[1]) and not np.array_equal(a[1], first[1])
    g.set_lights(moved)
    check("moved", dict(camera=cam1, lights=moved), False)
    g.set_materials(rough)
    check("materials", dict(camera=cam1, lights=moved, materials=rough), False)
    g.set_camera(cam2)
    check("camera", dict(camera=cam2, lights=moved, materials=rough), False)
    g.set_camera(cam1)
    g.set_materials(table1)
    g.set_lights(lights1)
    back = check("first state", dict(camera=cam1, lights=lights1), False)
    assert np.array_equal(back[1], first[1])
    g.close()


@gpu
def test_scenes_that_take_k_wf_shade(pta, oracle):
    """Five lights: no visibility plane.  A directional light: the orthographic branch is not built into the variant - such a
    scene keeps k_wf_shade, k_og_shadow_vis<true> and k_wf_hits_load.  A translucent table: no cache serves it.  The
    variant's numbers stand still, the frames are the oracle's."""
    case, scene, prof = open_case()
    cam = sb.make_camera(pta, **CAMERA)
    g = pta.GpuScene(scene)
    steady(g, prof, open_want(oracle, scene, prof), "start", n=3)
    before = fused(g)
    for name in ("five", "point_dir"):
        lights = sb.make_lights(pta, name)
        g.set_lights(lights)
        want = oracle_frame(oracle, sb.build(case, pta=pta, camera=cam, lights=lights), prof, walk=True)
        assert frames(g, prof, want, name, 4) == [ZERO] * 4
    assert v1.stats(g)["launches"] == 2 + 3, v1.stats(g)   # (the directional light's frames did use the plane)
    lights1 = sb.make_lights(pta, "point")
    g.set_lights(lights1)
    alpha = sb.case_materials(case._replace(factor_set="alpha"), pta)
    g.set_materials(alpha)
    want = oracle_frame(oracle, sb.build(case, pta=pta, camera=cam, materials=alpha), prof, walk=True)
    assert frames(g, prof, want, "translucent", 3) == [ZERO] * 3
    assert fused(g) == before
    g.close()


@gpu
def test_holes(pta, oracle, monkeypatch):
    """PT_HIT2_CACHE_HOLES=3: every third item has no bounce-2 record - its survivor keeps its queue record, is listed for the
    exact walker and counted, by the variant and by the cache alike; the frame is the oracle's, and its records are those of
    a frame without holes."""
    _, scene, prof = open_case()
    want = open_want(oracle, scene, prof)
    g = pta.GpuScene(scene)
    whole = steady(g, prof, want, "whole", n=3)
    g.close()
    monkeypatch.setenv("PT_HIT2_CACHE_HOLES", "3")
    g = pta.GpuScene(scene)
    got = frames(g, prof, want, "holes", 4)
    d = got[3]
    assert got[2] == d and d["next_unknown"] > 0 and d["launches"] == 1, got
    assert d["next_written"] + d["next_elided"] + d["next_unknown"] == whole["next_written"] + whole["next_elided"], (d, whole)
    assert d["next_elided"] < whole["next_elided"] and d["inlined"] == whole["inlined"], (d, whole)
    assert h2.stats(g)[1]["unknown"] == fused(g)["next_unknown"], (h2.stats(g), fused(g))
    g.close()


@gpu
def test_records_stored_by_a_frame_that_inlined_serve_a_frame_that_defers(pta, monkeypatch):
    """The generated scene (100 000 triangles, opaque, point lights) under a sky that is not black: its escape masks end paths at
    bounce 1 once their lights are in their colour - behind a shadow record they may not, the background comes after the lights.  PT_HIT2_CACHE switched on under a full visibility plane: the storing
    frame adds the lights itself, so the paths the masks end there leave no bounce-2 record.  Then a light moves: the frame
    that defers everything brings those paths to bounce 2 again - items without a record, cast exactly and counted.  Every
    frame is, bit for bit, the frame of the same sequence with the two switches off."""
    scene = pta.HostScene.generate_ps5(100000, 0, 8)
    for k, v in enumerate((0.3, 0.5, 0.9)):
        scene.desc.contents.background[k] = v
    prof = pta.Profile.make(W, H, SPP, BOUNCES)
    moved = scene.lights
    moved[0].vec[0] += 0.25

    def sequence(on):
        for k in SWITCHES:
            monkeypatch.setenv(k, "1" if on else "0")
        monkeypatch.setenv("PT_HIT2_CACHE", "0")
        g = pta.GpuScene(scene)
        images, numbers = [], []

        def run(n):
            for _ in range(n):
                before = fused(g)
                images.append(g.render(prof))
                numbers.append(delta(fused(g), before))

        run(4)
        monkeypatch.delenv("PT_HIT2_CACHE")
        run(3)   # (the frame before had this key: keyed and stored at once, then loaded)
        g.set_lights(moved)
        run(4)
        unknown = h2.stats(g)[1]["unknown"]
        g.close()
        return images, numbers, unknown

    want, off, _ = sequence(False)
    assert off == [ZERO] * 11, off
    got, n, unknown = sequence(True)
    print(n)
    for frame, (a, b) in enumerate(zip(got, want)):
        assert_same(a, b, frame)
    assert not np.array_equal(want[6][1], want[10][1])   # (the move changed the image)
    assert n[3]["inlined"] > 0 and n[3]["next_written"] == 0 and n[3]["next_elided"] > 0, n   # (ended by the masks)
    assert n[4]["next_written"] == 0 and n[6]["next_written"] > 0 and n[6]["next_unknown"] == 0, n
    assert n[7] == ZERO and n[8]["inlined"] == 0 and n[8]["next_unknown"] > 0 and unknown >= n[8]["next_unknown"], (n, unknown)
    assert n[10]["inlined"] > 0 and n[10]["next_unknown"] == 0, n


@gpu
def test_each_switch_toggled_between_frames(pta, oracle, monkeypatch):
    """PT_VIS1_FUSED=0: k_wf_shade again, the numbers stand still (and PT_HIT2_FUSED alone does nothing).  PT_HIT2_FUSED=0: the
    lights are still added here, bounce 2 loads through k_wf_hits_load.  On again the variant resumes at once: nothing was
    re-keyed.  The caches' loads go on throughout."""
    _, scene, prof = open_case()
    want = open_want(oracle, scene, prof)
    g = pta.GpuScene(scene)
    per_frame = steady(g, prof, want, "on", n=4)
    loads = h2.stats(g)[1]["loads"]
    monkeypatch.setenv("PT_VIS1_FUSED", "0")
    assert frames(g, prof, want, "first off", 2) == [ZERO] * 2
    monkeypatch.setenv("PT_VIS1_FUSED", "1")
    monkeypatch.setenv("PT_HIT2_FUSED", "0")
    got = frames(g, prof, want, "second off", 2)
    for d in got:   # (the paths the masks end here are counted as elided either way)
        assert d["launches"] == 1 and d["inlined"] == per_frame["inlined"] and d["deferred"] == per_frame["deferred"], (got, per_frame)
        assert d["next_written"] == d["next_unknown"] == 0 and d["next_elided"] < per_frame["next_elided"], (got, per_frame)
    monkeypatch.setenv("PT_HIT2_FUSED", "1")
    assert frames(g, prof, want, "on again", 2) == [per_frame] * 2
    for k in SWITCHES:   # the defaults: the first step on, the second off
        monkeypatch.delenv(k)
    for d in frames(g, prof, want, "defaults", 2):
        assert d["launches"] == 1 and d["inlined"] == per_frame["inlined"] and d["next_written"] == 0, (d, per_frame)
    assert h2.stats(g)[1]["loads"] == loads + 8 and h2.stats(g)[1]["unknown"] == 0, h2.stats(g)
    g.close()


@gpu
def test_chunks_sample_batches_and_a_partial_budget(pta, monkeypatch):
    """Small queues: two chunks of one pass, and - sample batches of two - four passes of one chunk each: every chunk takes the
    variant.  With room for about half of the items in the visibility plane the batches above its stride take k_wf_shade.
    Same bits as a frame with the switches off."""
    case, scene = open_scene("point", BOUNCES)
    w, h, spp = 640, 360, 8
    items = 640 * 384 * spp
    prof = sb.profile(case, w, h, spp)
    for k in SWITCHES:
        monkeypatch.setenv(k, "0")
    g = pta.GpuScene(scene)
    one_pass = [g.render(prof) for _ in range(3)][-1]
    assert fused(g) == ZERO
    g.close()
    for k in SWITCHES:
        monkeypatch.setenv(k, "1")
    monkeypatch.setenv("PT_QUEUE_GIB", "0.01")
    monkeypatch.setenv("PT_QUEUE_STEADY_GIB", "0.02")
    monkeypatch.setenv("PT_QUEUE_ONE_PASS_GIB", "0.02")
    whole = None
    for budget, batch in ((None, 0), (None, 2), ("0.00095", 2)):
        if budget:
            monkeypatch.setenv("PT_VIS1_CACHE_GIB", budget)   # room for 1 020 032 items: two of the four batches
        g = pta.GpuScene(scene)
        opts = pta.Opts.make(sample_batch=batch)
        for frame in range(4):
            c0 = v1.chunks(g)
            d = frames(g, prof, one_pass, (budget, batch, frame), 1, opts)[0]
            assert g.info().as_dict()["queue_chunk_items"] < items
            dc = v1.chunks(g) - c0
            if frame == 0:
                assert d == ZERO, d
            elif budget is None:
                assert d["launches"] == dc >= 2, (batch, frame, d, dc)
            else:
                assert 0 < d["launches"] < dc, (frame, d, dc)
            if frame >= 2 and budget is None:
                whole = whole or d["inlined"]
                assert d["inlined"] == whole > 0 and d["next_unknown"] == 0, (batch, frame, d, whole)
            elif frame >= 2:
                assert 0.3 * whole < d["inlined"] < 0.7 * whole, (frame, d, whole)
        g.close()


@gpu
def test_a_plan_counted_in_a_fused_frame_equals_one_counted_with_the_switches_off(pta, oracle, monkeypatch):
    """A colour edit drops the frame plan and keeps every plane: the next plan is counted in a frame that adds the lights
    itself and elides.  It reads shadow records written + inlined and queue records written + elided, so its queues, its
    inline rule and its last bounces are those of a frame that does neither: the switches off, and then the caches off, render
    the oracle's frame with it and no queue runs full (the call after would fail); a second scene that runs the sequence
    with the switches off throughout has the same queue bytes and plan."""
    case, scene = open_scene("point", BOUNCES)
    prof = sb.profile(case, 160, 96, SPP)
    pos = tuple(sb.make_lights(pta, "point")[0].vec)
    recoloured = [sb._light(pta, pta.PT_LIGHT_POINT, pos, (20.0, 170.0, 90.0))]
    first = shared(("children", "open"), lambda: oracle_frame(oracle, scene, prof))
    want = oracle_frame(oracle, sb.build(case, pta=pta, camera=sb.make_camera(pta, **CAMERA), lights=recoloured), prof, walk=True)

    def sequence(switches_off):
        for k in SWITCHES:
            monkeypatch.setenv(k, "0" if switches_off else "1")
        g = pta.GpuScene(scene)
        seen = []

        def run(what, w, n):
            for frame in range(n):
                assert_same(g.render(prof), w, (switches_off, what, frame))
                i = g.info().as_dict()
                seen.append((what, frame, i["queue_bytes"], i["frame_planned"]))

        run("start", first, 4)
        g.set_lights(recoloured)
        before = fused(g)
        run("recoloured", want, 4)   # counted in the first, planned from the second on
        assert seen[-1][3] == 1, seen
        d = delta(fused(g), before)
        assert (d["launches"] == 4 and d["inlined"] > 0 and d["next_elided"] > 0) != switches_off, (switches_off, d)
        for k in SWITCHES:
            monkeypatch.setenv(k, "0")
        st = fused(g)
        run("switches off", want, 3)
        assert fused(g) == st
        monkeypatch.setenv("PT_VIS1_CACHE", "0")
        monkeypatch.setenv("PT_HIT2_CACHE", "0")
        run("caches off", want, 3)
        assert seen[-1][3] == 1, seen
        g.close()
        for k in ("PT_VIS1_CACHE", "PT_HIT2_CACHE"):
            monkeypatch.delenv(k)
        return seen

    assert sequence(False) == sequence(True)


def test_the_variants_keep_the_budget_of_the_kernel_they_replace(tmp_path):
    """From the built library: at most 128 vector registers, scratch and LDS not above those of k_wf_shade<false, false, false, 0>
    in the same build - the workgroups per CU stay what they are."""
    t = kernel_table(tmp_path)
    base = find(t, "k_wf_shadeILb0ELb0ELb0ELi0EE")
    for gridx in (256, 256 | 512):
        k = find(t, f"k_wf_shade_fusedILi{gridx}EE")
        print(gridx, k, base)
        assert k["vgpr_count"] <= 128, (gridx, k)
        assert k["private_segment_fixed_size"] <= base["private_segment_fixed_size"], (gridx, k, base)
        assert k["group_segment_fixed_size"] <= base["group_segment_fixed_size"], (gridx, k, base)
