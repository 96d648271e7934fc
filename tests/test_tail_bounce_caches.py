"""The frame caches of the bounces behind bounce 2 (csrc/pt_gpu.hip pt_scene::tail_hits, tail_vis): the closest hits of the
rays of bounces 3, 4 and 5 and the shadow visibility of bounces 2, 3 and 4, each a plane of its own, driven by the table by
bounce that already serves bounces 1 and 2; and the shade pass of bounces 2-4 that adds the lights of known visibility itself
(k_wf_shade_fused<256> with that bounce's plane and counters).  No light enters a later bounce's ray and the roulette of
bounces 4+ draws from the item's words, so all of it has the keys of bounces 1 and 2.

What could go wrong beyond the lists of tests/test_bounce2_hit_cache.py and tests/test_bounce1_shade_fused.py: two bounces'
planes, events or counter blocks mixed up (the visibility byte of every bounce is found by the same out_slot), a count of a
later bounce leaking into the getters of bounces 1 and 2, a plane behind one that is switched off or over budget still in
use, the shade pass before a loaded bounce listing rays for the exact walker, bounce 6 cast from a bounce-5 queue whose hits
were loaded, a plan counted in a loading frame too short for a frame that casts.

Every frame is compared bit for bit - f32 accumulator and rgb8 - with the CPU oracle or with the same sequence rendered
with the three new switches off, and every test asserts loads > 0 (hits) or inlined > 0 (visibility) for each bounce it
claims to cover.  The scenes were picked on the CPU from the oracle's counts at this size (64 x 48 x 4; rays per bounce =
segments at depth b - segments at depth b - 1): `open` has 371 and 69 rays at bounces 3 and 4 and none at bounce 5, and its
shadow records go through k_og_shadow at every bounce - it covers the hit planes of bounces 3-4 and the visibility planes and
fused passes of bounces 2-4; `spheres` (tests/golden) has 419, 314, 50, 42 and 35 rays at bounces 3-7 - it covers the hit
planes of bounces 3-5 and the cast bounces behind them, while its frame plan puts the shadow casts of bounces 2-5 inside the
shade kernel (more than 60 % of their rays reach a lit surface), so its visibility planes are keyed and not read - except in the last test, which
renders it in a child process with PT_OG_INLINE_AUTO=0: the one case with a loaded bounce 5 and read visibility planes
together, and, spheres having no long normals, with nothing deferred once the planes are full.  The generator's closed room
(2 000 triangles) was tried and is not used: it has no ray at bounce 5 at this size and inlines every bounce."""
import numpy as np
import pytest

import scene_builder as sb
import test_bounce1_hit_cache as h1
import test_bounce1_shade_fused as f1
import test_bounce1_shadow_visibility_cache as v1
from test_bounce2_hit_cache import BOUNCES, H, SPP, W, open_case, open_want, shared
from test_prestaged_misses import CAMERA, assert_same, open_scene, oracle_frame

gpu = pytest.mark.gpu

TAIL = ("PT_TAIL_HIT_CACHE", "PT_TAIL_VIS_CACHE", "PT_TAIL_VIS_FUSED")
HITS, VIS = (3, 4, 5), (2, 3, 4)
ZERO = f1.ZERO


@pytest.fixture(autouse=True)
def tail_on(monkeypatch):
    """The tests here run all three steps, whatever ships on."""
    switch(monkeypatch, True)


def switch(monkeypatch, on):
    for k in TAIL:
        monkeypatch.setenv(k, "1" if on else "0")


def hits(g, b):
    return dict(zip(h1.NAMES, g.bounce_hits_cache_stats(b)))


def vis(g, b):
    return dict(zip(v1.NAMES, g.bounce_vis_cache_stats(b)))


def fused(g, b):
    return dict(zip(f1.NAMES, g.bounce_fused_stats(b)))


def counts(st):
    return st["resets"], st["stores"], st["loads"]


def old(g):
    """What the getters of bounces 1 and 2 say."""
    return (g.hit1_cache_stats(), g.hit1_fused_stats(), g.hit2_cache_stats(), g.vis1_cache_stats(), g.bounce1_fused_stats())


def frame(g, prof, want, what, opts=None):
    """One frame, `want`: what it added to the fused passes' numbers, by bounce."""
    before = {b: fused(g, b) for b in VIS}
    assert_same(g.render(prof, opts) if opts else g.render(prof), want, what)
    return {b: f1.delta(fused(g, b), before[b]) for b in VIS}


def spheres_case(pta, oracle, scene_cache, bounces):
    scene = scene_cache("spheres")
    prof = pta.Profile.make(W, H, SPP, bounces)
    return scene, prof, shared(("tail", "spheres", bounces), lambda: oracle_frame(oracle, scene, prof))


def test_the_library_has_the_getters_by_bounce(pta):
    """No GPU: the three symbols are there with the bounce argument."""
    lib = pta.gpu_lib()
    for name in ("pt_get_bounce_hits_cache_stats", "pt_get_bounce_vis_cache_stats", "pt_get_bounce_fused_stats"):
        assert name in pta.GPU_SYMBOLS and getattr(lib, name).argtypes[1].__name__ == "c_uint"


def by_bounce_equals_old(g):
    """Bounces 1 and 2 answer through the getters by bounce with the numbers of their own getters."""
    assert g.bounce_hits_cache_stats(1) == g.hit1_cache_stats() and g.bounce_hits_cache_stats(2) == g.hit2_cache_stats()
    assert g.bounce_vis_cache_stats(1) == g.vis1_cache_stats() and g.bounce_fused_stats(1) == g.bounce1_fused_stats()


@gpu
def test_the_getters_by_bounce_answer_for_bounces_1_and_2_and_refuse_the_rest(pta, oracle):
    """On a scene with live planes (open, four frames) and on a fresh one: bounces 1 and 2 give their own getters' numbers;
    bounce 0 and bounce 6 (hits), 0 and 5 (visibility, fused passes) are PT_ERR_INVALID."""
    _, scene, prof = open_case()
    want = open_want(oracle, scene, prof)
    g = pta.GpuScene(scene)
    for n in range(5):
        by_bounce_equals_old(g)
        for getter, bad in ((g.bounce_hits_cache_stats, (0, 6, 7)), (g.bounce_vis_cache_stats, (0, 5, 6)), (g.bounce_fused_stats, (0, 5, 6))):
            for b in bad:
                with pytest.raises(pta.PtError) as err:
                    getter(b)
                assert err.value.code == pta.PT_ERR_INVALID, (getter, b, err.value)
        if n < 4:
            frame(g, prof, want, ("getters", n))
    assert g.hit2_cache_stats()[5] > 0 and g.bounce1_fused_stats()[1] > 0   # (the numbers compared were not all zero)
    g.close()


@gpu
@pytest.mark.parametrize("name", ["open", "spheres"])
def test_consecutive_frames(pta, oracle, scene_cache, name):
    """Six frames of 5 bounces.  Frame 0 allocates nothing.  Frame 1 keys, zeroes and stores every hit plane - and, the
    visibility planes being keyed with the hits as bounce 1's is, fills them: its fused passes defer every record.  From frame
    2 on one load per plane and frame, the fused passes add the lights (inlined > 0) and what they still defer - the floor's
    long normals, which never get a byte - is the same every frame: k_og_shadow_vis casts nothing new.  open: hits 3-4,
    visibility 2-4.  spheres: hits 3-5."""
    if name == "open":
        _, scene, prof = open_case()
        want = open_want(oracle, scene, prof)
    else:
        scene, prof, want = spheres_case(pta, oracle, scene_cache, BOUNCES)
    reached = (3, 4) if name == "open" else HITS
    g = pta.GpuScene(scene)
    first = steady = None
    for n in range(6):
        d = frame(g, prof, want, (name, n))
        if n == 0:
            assert all(hits(g, b) == h1.NONE for b in HITS) and all(vis(g, b) == v1.NONE for b in VIS), n
            assert all(d[b] == ZERO for b in VIS), d
            continue
        items = g.hit_cache_stats()[1]
        for b in HITS:
            st = hits(g, b)
            assert st["bytes"] == 16 * items > 0 and st["items"] == st["cached"] == items and st["unknown"] == 0, (name, n, b, st)
            if b in reached:
                assert counts(st) == (1, 1, n - 1), (name, n, b, st)
            else:   # (no ray: keyed and marked full without a storing launch)
                assert st["resets"] == 1 and st["stores"] == 0, (name, n, b, st)
        for b in VIS:
            st = vis(g, b)
            assert st["bytes"] == st["items"] == items and st["resets"] == 1, (name, n, b, st)
            assert d[b]["next_written"] == d[b]["next_unknown"] == 0, (name, n, b, d)   # (bounce 1's alone)
        if name != "open":
            continue
        for b in VIS:
            assert vis(g, b)["launches"] == n and d[b]["launches"] == 1, (n, b, vis(g, b), d)
        if n == 1:
            first = d
            assert all(d[b]["inlined"] == 0 and d[b]["deferred"] > 0 for b in VIS), d
        else:
            steady = steady or d
            assert d == steady, (n, d, steady)
            assert all(d[b]["inlined"] > 0 and d[b]["inlined"] + d[b]["deferred"] == first[b]["deferred"] for b in VIS), (d, first)
    print(name, first, steady)
    assert all(hits(g, b)["loads"] > 0 for b in reached)
    g.close()


@gpu
def test_edits_under_a_live_scene(pta, oracle):
    """open, hits 3-4 and visibility 2-4.  A recoloured light: nothing re-keys.  A moved light: the visibility planes re-key -
    a frame without them, one that defers everything, then the lights are added again - while the hit planes go on loading.
    A material edit and a camera move: everything re-keys on the second frame after.  Five lights: no visibility plane is
    read, the hit planes go on (or re-key, where the count changed the camera grid's resolution, which is in their key).
    Every frame equals the oracle for the edited scene."""
    case, scene, prof = open_case()
    P = pta.PT_LIGHT_POINT
    cam1 = sb.make_camera(pta, **CAMERA)
    cam2 = sb.make_camera(pta, eye=(-0.9, 2.1, 2.9), target=(0.3, 0.3, -0.4), fov=0.8)
    lights1 = sb.make_lights(pta, "point")
    recoloured = [sb._light(pta, P, tuple(lights1[0].vec), (20.0, 170.0, 90.0))]
    moved = [sb._light(pta, P, (-0.8, 2.9, 0.4), (20.0, 170.0, 90.0))]
    rough = sb.case_materials(case, pta)
    for m in rough:
        m.roughness = min(1.0, 0.37 + 0.5 * m.roughness)
    g = pta.GpuScene(scene)
    first = open_want(oracle, scene, prof)
    for n in range(4):
        per_frame = frame(g, prof, first, ("start", n))
    assert all(per_frame[b]["inlined"] > 0 for b in VIS), per_frame

    def run(what, state, n):
        want = oracle_frame(oracle, sb.build(case, pta=pta, **state), prof, walk=True)
        out = []
        for k in range(n):
            d = frame(g, prof, want, (what, k))
            out.append((d, {b: counts(hits(g, b)) for b in (3, 4)}, {b: vis(g, b)["resets"] for b in VIS}))
        return out

    h0, v0 = {b: counts(hits(g, b)) for b in (3, 4)}, {b: vis(g, b)["resets"] for b in VIS}
    g.set_lights(recoloured)
    for k, (d, h, v) in enumerate(run("colour", dict(camera=cam1, lights=recoloured), 2)):
        assert d == per_frame and v == v0, (k, d, v)
        assert all(h[b] == (h0[b][0], h0[b][1], h0[b][2] + k + 1) for b in (3, 4)), (k, h, h0)
    h0 = {b: counts(hits(g, b)) for b in (3, 4)}
    g.set_lights(moved)
    got = run("moved", dict(camera=cam1, lights=moved), 4)
    for k, (d, h, v) in enumerate(got):   # (unknown casts are allowed: the escape masks end other paths under other lights)
        assert all(h[b] == (h0[b][0], h0[b][1], h0[b][2] + k + 1) for b in (3, 4)), (k, h, h0)
        assert all(v[b] == v0[b] + (k >= 1) for b in VIS), (k, v, v0)
    assert all(got[0][0][b] == ZERO for b in VIS), got[0]
    assert all(got[1][0][b]["inlined"] == 0 and got[1][0][b]["deferred"] > 0 for b in VIS), got[1]
    assert got[2][0] == got[3][0] and all(got[2][0][b]["inlined"] > 0 for b in VIS), got[2:]
    state = dict(camera=cam1, lights=moved)
    for what, edit, change in (("materials", lambda: g.set_materials(rough), dict(materials=rough)),
                               ("camera", lambda: g.set_camera(cam2), dict(camera=cam2))):
        h0, v0 = {b: counts(hits(g, b)) for b in (3, 4)}, {b: vis(g, b)["resets"] for b in VIS}
        edit()
        state.update(change)
        got = run(what, state, 4)
        for k, (d, h, v) in enumerate(got):   # nothing; zeroed and stored; loaded; loaded
            assert all(h[b] == (h0[b][0] + (k >= 1), h0[b][1] + (k >= 1), h0[b][2] + max(0, k - 1)) for b in (3, 4)), (what, k, h, h0)
            assert all(v[b] == v0[b] + (k >= 1) for b in VIS), (what, k, v, v0)
        assert all(got[0][0][b] == ZERO for b in VIS), (what, got[0])
        assert all(got[1][0][b]["inlined"] == 0 and got[1][0][b]["deferred"] > 0 for b in VIS), (what, got[1])
        assert got[2][0] == got[3][0] and all(got[2][0][b]["inlined"] > 0 for b in VIS), (what, got[2:])
    five = moved + [sb._light(pta, P, p, c) for p, c in (((-1.0, 3.0, 0.2), (60.0, 20.0, 90.0)), ((1.2, 2.5, 1.0), (30.0, 30.0, 30.0)),
                                                         ((0.0, 3.5, -0.5), (10.0, 40.0, 20.0)), ((-0.5, 2.8, 1.5), (25.0, 5.0, 45.0)))]
    h0, v0 = {b: counts(hits(g, b)) for b in (3, 4)}, {b: vis(g, b) for b in VIS}
    res = g.info().as_dict().get("cam_grid_res")
    g.set_lights(five)
    rekeyed = g.info().as_dict().get("cam_grid_res") != res
    state.update(lights=five)
    for k, (d, h, v) in enumerate(run("five", state, 4)):
        assert all(d[b] == ZERO for b in VIS) and all(vis(g, b) == v0[b] for b in VIS), (k, d)
        if rekeyed:
            assert all(h[b] == (h0[b][0] + (k >= 1), h0[b][1] + (k >= 1), h0[b][2] + max(0, k - 1)) for b in (3, 4)), (k, h, h0)
        else:
            assert all(h[b] == (h0[b][0], h0[b][1], h0[b][2] + k + 1) for b in (3, 4)), (k, h, h0)
    assert all(hits(g, b)["loads"] > h0[b][2] for b in (3, 4))
    g.close()


@gpu
def test_holes(pta, oracle, monkeypatch):
    """PT_TAIL_HIT_CACHE_HOLES=3 on open: the storing launches of bounces 3-5 leave out every third item, the loading launches
    of bounces 3 and 4 list those for the exact walker and count them, the image is the oracle's, and the exact list is long
    enough: a list that ran full would fail the call after."""
    _, scene, prof = open_case()
    want = open_want(oracle, scene, prof)
    monkeypatch.setenv("PT_TAIL_HIT_CACHE_HOLES", "3")
    g = pta.GpuScene(scene)
    for n in range(6):
        frame(g, prof, want, ("holes", n))
        for b in (3, 4):
            st = hits(g, b)
            assert (st["unknown"] > 0) == (n >= 2) and (n == 0 or counts(st) == (1, 1, n - 1)), (n, b, st)
        assert hits(g, 1)["unknown"] == hits(g, 2)["unknown"] == 0
    assert g.info().as_dict()["frame_planned"] == 1
    for b in (3, 4):
        per_frame = hits(g, b)["unknown"] // 4
        assert hits(g, b)["unknown"] == 4 * per_frame and per_frame > 0, (b, hits(g, b))
    g.close()


@gpu
def test_transition_to_cast_bounces(pta, oracle, scene_cache, monkeypatch):
    """spheres, 7 bounces: bounces 6 and 7 are cast behind a loaded bounce 5 - the shade pass of bounce 5 lists rays for the
    exact walker again - and the roulette of bounces 4+ draws on loaded records.  Same bits as the oracle and as the frame
    with the three switches off.  The premise, from the oracle's counts: rays exist at bounces 6 and 7."""
    scene, prof, want = spheres_case(pta, oracle, scene_cache, 7)
    seg = [shared(("tail", "spheres", b), lambda b=b: oracle_frame(oracle, scene, pta.Profile.make(W, H, SPP, b)))[2]["segments"] for b in (5, 6, 7)]
    assert seg[0] < seg[1] < seg[2], seg
    g = pta.GpuScene(scene)
    for n in range(5):
        frame(g, prof, want, ("seven", n))
    for b in HITS:
        assert counts(hits(g, b)) == (1, 1, 3) and hits(g, b)["unknown"] == 0, (b, hits(g, b))
    g.close()
    switch(monkeypatch, False)
    g = pta.GpuScene(scene)
    for n in range(3):
        assert_same(g.render(prof), want, ("seven, switches off", n))
    assert all(hits(g, b) == h1.NONE for b in HITS)
    g.close()


@gpu
def test_switches_and_budgets(pta, oracle, monkeypatch):
    """open.  PT_TAIL_HIT_CACHE=0 in the middle of a sequence: the planes of bounces 3-5 are released, the visibility planes
    of bounces 3 and 4 stand still, bounce 2's goes on (its hits are hit2_cache's); on again they are keyed at once.
    PT_TAIL_VIS_CACHE=0: no fused pass at bounces 2-4, the hits go on loading.  PT_TAIL_HIT_CACHE_GIB too small for a plane:
    bounces 3+ cast, the visibility planes of bounces 3 and 4 stay unused.  The image is the oracle's throughout, and the
    getters of bounces 1 and 2 say, frame by frame, what they say in a run with the three switches off."""
    _, scene, prof = open_case()
    want = open_want(oracle, scene, prof)
    steps = [(4, {}), (2, {"PT_TAIL_HIT_CACHE": "0"}), (3, {}), (2, {"PT_TAIL_VIS_CACHE": "0"}), (3, {}),
             (2, {"PT_TAIL_HIT_CACHE_GIB": "0.0000001"}), (3, {})]

    def sequence(on):
        g = pta.GpuScene(scene)
        seen, olds = [], []
        for n, env in steps:
            switch(monkeypatch, on)
            monkeypatch.delenv("PT_TAIL_HIT_CACHE_GIB", raising=False)
            for k, v in env.items():
                if on:
                    monkeypatch.setenv(k, v)
            for k in range(n):
                d = frame(g, prof, want, (on, env, k))
                olds.append(old(g))
                seen.append((d, {b: hits(g, b) for b in HITS}, {b: vis(g, b) for b in VIS}))
        g.close()
        return seen, olds

    off, olds_off = sequence(False)
    assert all(d[b] == ZERO for d, _, _ in off for b in VIS) and all(h[b] == h1.NONE for _, h, _ in off for b in HITS)
    on, olds_on = sequence(True)
    assert olds_on == olds_off
    at = np.cumsum([0] + [n for n, _ in steps])
    d, h, v = on[at[1] - 1]   # steady
    assert all(d[b]["inlined"] > 0 for b in VIS) and all(counts(h[b]) == (1, 1, 2) for b in (3, 4)), (d, h)
    for k in range(at[1], at[2]):   # the hit planes off
        d, h, v = on[k]
        assert all(h[b]["bytes"] == h[b]["items"] == h[b]["cached"] == 0 and counts(h[b])[:2] == (1, 1 if b < 5 else 0) for b in HITS), (k, h)
        assert d[2]["launches"] == 1 and d[2]["inlined"] > 0 and d[3] == d[4] == ZERO, (k, d)
    for k in range(at[2], at[3]):   # on again: keyed at once, stored, loaded
        d, h, v = on[k]
        assert all(counts(h[b]) == (2, 2, 2 + k - at[2]) and h[b]["cached"] == h[b]["items"] > 0 for b in (3, 4)), (k, h)
    assert all(on[at[3] - 1][0][b]["inlined"] > 0 for b in VIS), on[at[3] - 1][0]
    for k in range(at[3], at[4]):   # the visibility planes off
        d, h, v = on[k]
        assert all(d[b] == ZERO and v[b]["bytes"] == 0 for b in VIS), (k, d, v)
        assert all(h[b]["loads"] == on[k - 1][1][b]["loads"] + 1 for b in (3, 4)), (k, h)
    assert all(on[at[5] - 1][0][b]["inlined"] > 0 for b in VIS), on[at[5] - 1][0]
    for k in range(at[5], at[6]):   # no room for a hit plane
        d, h, v = on[k]
        assert all(counts(h[b]) == counts(on[at[5] - 1][1][b]) for b in HITS), (k, h)
        assert d[2]["launches"] == 1 and d[2]["inlined"] > 0 and d[3] == d[4] == ZERO, (k, d)
        assert all(v[b]["launches"] == on[at[5] - 1][2][b]["launches"] for b in (3, 4)), (k, v)
    d, h, v = on[-1]
    assert all(d[b]["inlined"] > 0 for b in VIS) and all(h[b]["loads"] > on[at[6] - 1][1][b]["loads"] for b in (3, 4)), (d, h)


@gpu
def test_a_plan_counted_in_a_loading_and_inlining_frame_equals_one_counted_with_the_switches_off(pta, oracle, monkeypatch):
    """A colour edit drops the frame plan and keeps every plane: the next plan is counted in a frame that loads bounces 1-4
    and adds the lights of bounces 1-4 itself.  It reads queue records written + elided and shadow records written + inlined,
    so the three switches off, and then every cache off, render the oracle's frame with it and no queue or list runs full
    (the call after would fail); a second scene that runs the sequence with the three switches off throughout has the same
    queue bytes and plan in every frame."""
    case, scene = open_scene("point", BOUNCES)
    prof = sb.profile(case, 160, 96, SPP)
    pos = tuple(sb.make_lights(pta, "point")[0].vec)
    recoloured = [sb._light(pta, pta.PT_LIGHT_POINT, pos, (20.0, 170.0, 90.0))]
    first = shared(("children", "open"), lambda: oracle_frame(oracle, scene, prof))
    want = oracle_frame(oracle, sb.build(case, pta=pta, camera=sb.make_camera(pta, **CAMERA), lights=recoloured), prof, walk=True)

    def sequence(on):
        switch(monkeypatch, on)
        g = pta.GpuScene(scene)
        seen = []

        def run(what, w, n):
            total = {b: dict(ZERO) for b in VIS}
            for k in range(n):
                d = frame(g, prof, w, (on, what, k))
                total = {b: {key: total[b][key] + d[b][key] for key in ZERO} for b in VIS}
                i = g.info().as_dict()
                # (a frame that casts what the plan's frame loaded makes its exact lists as long as its queues, as
                # tests/test_bounce2_hit_cache.py has it: from the switch on, the bytes differ by those lists)
                seen.append((what, k, i["queue_bytes"] if what in ("start", "recoloured") else None, i["frame_planned"]))
            return total

        run("start", first, 4)
        g.set_lights(recoloured)
        loads = {b: hits(g, b)["loads"] for b in (3, 4)}
        d = run("recoloured", want, 4)   # counted in the first, planned from the second on
        assert seen[-1][3] == 1, seen
        for b in VIS:
            assert (d[b]["launches"] == 4 and d[b]["inlined"] > 0) == on and (d[b] == ZERO) != on, (on, b, d)
        assert all((hits(g, b)["loads"] == loads[b] + 4) == on for b in (3, 4)), (on, loads)
        switch(monkeypatch, False)
        assert run("switches off", want, 3) == {b: ZERO for b in VIS}
        for k in ("PT_VIS1_CACHE", "PT_HIT1_CACHE"):
            monkeypatch.setenv(k, "0")
        run("caches off", want, 3)
        assert seen[-1][3] == 1, seen
        g.close()
        for k in ("PT_VIS1_CACHE", "PT_HIT1_CACHE"):
            monkeypatch.delenv(k)
        return seen

    assert sequence(True) == sequence(False)


@gpu
def test_chunks_and_sample_batches(pta, monkeypatch):
    """Small queues (the budget of tests/test_bounce2_hit_cache.py): two chunks of one pass over all eight samples, and -
    sample batches of two - four passes of one chunk each.  The visibility byte of a record is found in its batch's part
    of each bounce's plane; the hit planes grow as prefixes over the chunks.  Per bounce, loads and fused launches per frame
    equal the chunks.  Same bits as a frame with the three switches off, in one pass."""
    case, scene = open_scene("point", BOUNCES)
    w, h, spp = 640, 360, 8
    items = 640 * 384 * spp
    prof = sb.profile(case, w, h, spp)
    switch(monkeypatch, False)
    g = pta.GpuScene(scene)
    one_pass = [g.render(prof) for _ in range(3)][-1]
    assert all(hits(g, b) == h1.NONE for b in HITS)
    g.close()
    switch(monkeypatch, True)
    monkeypatch.setenv("PT_QUEUE_GIB", "0.01")
    monkeypatch.setenv("PT_QUEUE_STEADY_GIB", "0.02")
    monkeypatch.setenv("PT_QUEUE_ONE_PASS_GIB", "0.02")
    whole = None
    for batch in (0, 2):
        g = pta.GpuScene(scene)
        opts = pta.Opts.make(sample_batch=batch)
        for n in range(4):
            c0, l0 = v1.chunks(g), {b: hits(g, b)["loads"] for b in (3, 4)}
            d = frame(g, prof, one_pass, (batch, n), opts)
            assert g.info().as_dict()["queue_chunk_items"] < items
            dc = v1.chunks(g) - c0
            if n == 0:
                assert all(d[b] == ZERO for b in VIS), d
                continue
            assert dc >= 2 and all(d[b]["launches"] == dc for b in VIS), (batch, n, d, dc)
            for b in (3, 4):
                st = hits(g, b)
                assert st["items"] == st["cached"] == items and st["resets"] == 1 and st["unknown"] == 0, (batch, n, b, st)
                assert st["loads"] - l0[b] == (dc if n >= 2 else 0), (batch, n, b, st, l0, dc)
            if n >= 2:
                inl = {b: d[b]["inlined"] for b in VIS}
                whole = whole or inl
                assert inl == whole and all(v > 0 for v in inl.values()), (batch, n, inl, whole)
        g.close()


@gpu
def test_scenes_that_keep_k_wf_shade(pta, oracle):
    """A point and a directional light on open: the orthographic branch is not built into the fused pass, so every bounce
    keeps k_wf_shade - no fused launch is counted at any bounce - while the hit planes of bounces 3-4 load and the visibility
    planes of bounces 2-4 are read and filled by k_og_shadow_vis<true>.  Every frame is the oracle's."""
    case, _, prof = open_case()
    lights = sb.make_lights(pta, "point_dir")
    scene = sb.build(case, pta=pta, camera=sb.make_camera(pta, **CAMERA), lights=lights)
    want = oracle_frame(oracle, scene, prof, walk=True)
    g = pta.GpuScene(scene)
    for n in range(5):
        d = frame(g, prof, want, ("point_dir", n))
        assert all(d[b] == ZERO for b in VIS) and fused(g, 1) == ZERO, (n, d)
    for b in (3, 4):
        assert counts(hits(g, b)) == (1, 1, 3) and hits(g, b)["unknown"] == 0, (b, hits(g, b))
    for b in VIS:
        assert vis(g, b)["resets"] == 1 and vis(g, b)["launches"] > 0, (b, vis(g, b))
    g.close()


SORT_CHILD = r"""
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
shas = []
for frame in range(5):
    rgb, acc = g.render(prof)
    shas.append(hashlib.sha1(np.ascontiguousarray(rgb, np.uint8).tobytes() + np.ascontiguousarray(acc, np.float32).tobytes()).hexdigest())
print("RESULT", json.dumps({"shas": shas, "hits": [list(map(int, g.bounce_hits_cache_stats(b))) for b in (3, 4)],
                            "vis": [list(map(int, g.bounce_vis_cache_stats(b))) for b in (2, 3, 4)],
                            "fused": [list(map(int, g.bounce_fused_stats(b))) for b in (1, 2, 3, 4)]}))
"""


@gpu
def test_a_sorting_frame_keeps_k_wf_shade(oracle):
    """PT_WF_SORT=1 (read once per process: a child): the fused pass keeps its counts in the LDS row that option writes, so no
    bounce takes it; the planes are used as before."""
    import hashlib
    import json
    import os
    import subprocess
    import sys
    from pathlib import Path
    root = Path(__file__).resolve().parent.parent
    _, scene, prof = open_case()
    want = open_want(oracle, scene, prof)
    want_sha = hashlib.sha1(np.ascontiguousarray(want[0], np.uint8).tobytes() + np.ascontiguousarray(want[1], np.float32).tobytes()).hexdigest()
    env = {k: v for k, v in os.environ.items() if not k.startswith(("PT_WF_", "PT_TAIL_"))}
    env.update(PT_WF_SORT="1", **dict.fromkeys(TAIL, "1"))
    run = subprocess.run([sys.executable, "-c", SORT_CHILD % {"root": str(root)}], env=env, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    res = json.loads([ln for ln in run.stdout.splitlines() if ln.startswith("RESULT ")][0][7:])
    print(res)
    assert res["shas"] == [want_sha] * 5, res
    assert all(tuple(h[3:6]) == (1, 1, 3) for h in res["hits"]) and all(v[2] == 1 and v[3] > 0 for v in res["vis"]), res
    assert all(f == [0] * 6 for f in res["fused"]), res


NO_INLINE_CHILD = r"""
import hashlib, json, sys
import numpy as np
sys.path.insert(0, %(root)r)
import __graft_entry__ as e
pta = e.load_package()
scene = pta.HostScene.load_isf(e.ROOT / "tests" / "golden" / "scenes" / "spheres" / "scene.isf")
prof = pta.Profile.make(64, 48, 4, 5)
g = pta.GpuScene(scene)
out = []
for frame in range(6):
    rgb, acc = g.render(prof)
    sha = hashlib.sha1(np.ascontiguousarray(rgb, np.uint8).tobytes() + np.ascontiguousarray(acc, np.float32).tobytes()).hexdigest()
    out.append({"sha": sha, "hits": [list(map(int, g.bounce_hits_cache_stats(b))) for b in (3, 4, 5)],
                "vis": [list(map(int, g.bounce_vis_cache_stats(b))) for b in (2, 3, 4)],
                "fused": [list(map(int, g.bounce_fused_stats(b))) for b in (2, 3, 4)]})
print("RESULT", json.dumps(out))
"""


@gpu
def test_loaded_bounce_5_and_read_visibility_planes_in_one_scene_without_long_normals(pta, oracle, scene_cache):
    """spheres, 5 bounces, with PT_OG_INLINE_AUTO=0 (read once per process: a child), so that its shadow records of bounces
    2-4 go through k_og_shadow_vis instead of the shade kernel: the one scene here that loads the hit planes of bounces 3, 4
    AND 5 and reads the visibility planes of bounces 2-4 in the same frames.  No surface of it has a normal too long for the
    light grids, so once the planes are filled NOTHING is deferred: from frame 2 on every shadow record of bounces 2-4 is
    inlined (deferred stands still, inlined grows by what frame 1 deferred) - a k_og_shadow_vis that left part of a
    bounce's bytes unwritten would show as deferred records.  Every frame is the oracle's."""
    import hashlib
    import json
    import os
    import subprocess
    import sys
    from pathlib import Path
    root = Path(__file__).resolve().parent.parent
    _, _, want = spheres_case(pta, oracle, scene_cache, BOUNCES)
    want_sha = hashlib.sha1(np.ascontiguousarray(want[0], np.uint8).tobytes() + np.ascontiguousarray(want[1], np.float32).tobytes()).hexdigest()
    env = {k: v for k, v in os.environ.items() if not k.startswith(("PT_WF_", "PT_TAIL_", "PT_OG_"))}
    env.update(PT_OG_INLINE_AUTO="0", **dict.fromkeys(TAIL, "1"))
    run = subprocess.run([sys.executable, "-c", NO_INLINE_CHILD % {"root": str(root)}], env=env, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    res = json.loads([ln for ln in run.stdout.splitlines() if ln.startswith("RESULT ")][0][7:])
    print(res)
    assert [r["sha"] for r in res] == [want_sha] * 6, res
    first = res[1]["fused"]   # the keying frame: launches 1, inlined 0, every record deferred
    assert all(f[0] == 1 and f[1] == 0 and f[2] > 0 for f in first), first
    for n in range(2, 6):
        for k in range(3):
            h, v, f = res[n]["hits"][k], res[n]["vis"][k], res[n]["fused"][k]
            assert tuple(h[3:7]) == (1, 1, n - 1, 0), (n, k, h)           # resets, stores, loads, unknown: bounces 3, 4, 5
            assert v[2] == 1 and v[3] == n, (n, k, v)                      # one reset, one k_og_shadow_vis launch per frame
            assert f[0] == n and f[2] == first[k][2] and f[1] == (n - 1) * first[k][2], (n, k, f, first)   # nothing deferred again
