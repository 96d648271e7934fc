"""Escape masks (csrc/pt_escape.h) and frame caches (csrc/pt_gpu.hip frame_caches) together, in the states a user gets: masks
that really end paths, arriving on the shipped schedule (PT_ESCAPE_AFTER unset: with a scene's third default-pipeline frame)
under caches that were keyed and stored without them, going away under a camera move while the caches serve, and coming back.

The geometry is scene_builder's `terrace`: a tessellated ground, a floating convex box, a floating slab and the panel of
`open` under a sky that is not black - three of four secondary rays leave the scene (the oracle's counts) and the masks end a
third of those without a cast (test_the_masks_of_terrace_end_paths prints the share; DESIGN 4b has it).  Every frame is
compared bit for bit - rgb8 and the f32 accumulator - with the brute-force CPU oracle, which knows neither masks nor caches
nor plans, and every test reads the numbers that make it mean something: masked_casts / bounce0_masked of an instrumented
frame, escape_prims and frame_planned, the caches' own counters.

What the caches do when the masks arrive or go - the expected tuples below follow from these rules, not from a run:
  * no cache key holds the masks (frame_caches: the enumeration, camera_generation, cam_res, material_generation, the light
    words), so arrival and loss re-key nothing, zero nothing and store nothing again: records stored without masks are
    loaded under them, the loads go on, one per frame and plane;
  * the shadow-visibility plane of bounce b (1-4) counts one launch of k_og_shadow_vis per chunk in which the plane exists,
    the bounce is launched (the plan leaves out the bounces behind the chunk's last ray) and its shadow casts are not inline
    (render_chunk: `vis_plane_of(b) && grid_mode == 0`; inline: where the plan counted shadow records for 60 % of the bounce's
    rays, make_plan) - on terrace one per frame and plane from the keying frame on (test_terrace_is_fit_for_a_gpu has the premise);
  * the masks only ever END paths, and only paths without a shadow record (pt_wf_shade_body.h: `zero || !to_shadow`), so
    under unchanged lights a loading frame keeps no path alive that the storing frame ended: no item without a record;
    under OTHER lights it may - the natural hole of test_a_light_edit_revives_paths_the_masks_ended_while_the_planes_were_filled;
  * escape_masks_build invalidates every frame plan: the arrival frame counts again (frame_planned 0), the next is planned;
  * pt_scene_set_camera to a camera with a larger delta_in drops the masks and restarts the schedule; the camera move - not
    the loss - re-keys the hit caches (nothing, then zeroed and stored, then loaded)."""
import numpy as np
import pytest

import film_model as fm
import scene_builder as sb
from test_prestaged_misses import CAMERA, assert_same, oracle_frame

gpu = pytest.mark.gpu

W, H, SPP, BOUNCES = 64, 48, 4, 5
HIT_NAMES = ("bytes", "items", "cached", "resets", "stores", "loads", "unknown")
SCHEDULES = {"default": None, "after-0": "0", "after-1": "1", "after-4": "4", "no-masks": None}
# The bounces of terrace at this size that have a ray, by the oracle's counts (rays_per_bounce; test_terrace_is_fit_for_a_gpu
# asserts them, at 5 and at 8 bounces): at each of bounces 1-4 some ray HITS - a ray that hits is never ended by a mask, so those
# queues are never empty, their hit planes get a storing launch and the plan launches those bounces; no ray at bounce 5 or
# later: that plane is keyed and marked full, and no test of this file stores or loads a record in it
# (tests/test_tail_bounce_caches.py does, on `spheres`).
REACHED, UNREACHED = (1, 2, 3, 4), (5,)

_frames = {}


def shared(key, make):
    """A reference frame, made once, shared and left unchanged."""
    if key not in _frames:
        out = make()
        for a in out[:2]:
            a.setflags(write=False)
        _frames[key] = out
    return _frames[key]


def terrace(pta, light_set="point", factor_set="opaque", bounces=BOUNCES, camera=None, size=(W, H), spp=SPP):
    case = sb.Case(f"terrace-{light_set}-{factor_set}", "terrace", "none", light_set, factor_set, bounces, "FILMIC", 0, False)
    scene = sb.build(case, pta=pta, camera=camera or sb.make_camera(pta, **CAMERA))
    return case, scene, sb.profile(case, size[0], size[1], spp)


def want_of(oracle, scene, prof, *key, **kw):
    """The oracle's frame, every ray of it checked finite first."""
    return shared(key + (prof.width, prof.height, prof.samples, prof.bounces, tuple(sorted(kw.items()))),
                  lambda: oracle_frame(oracle, scene, prof, walk=True, **kw))


def schedule(monkeypatch, name):
    """The environment of a schedule, set before the scene is made (scene_upload reads it once per scene).  Returns the frame
    index (0-based) at which the masks arrive, None: never."""
    monkeypatch.delenv("PT_ESCAPE_AFTER", raising=False)
    monkeypatch.delenv("PT_ESCAPE", raising=False)
    for k in ("PT_HIT1_CACHE_HOLES", "PT_HIT2_CACHE_HOLES", "PT_TAIL_HIT_CACHE_HOLES"):
        monkeypatch.delenv(k, raising=False)
    if name == "no-masks":
        monkeypatch.setenv("PT_ESCAPE", "0")
        return None
    if SCHEDULES[name] is not None:
        monkeypatch.setenv("PT_ESCAPE_AFTER", SCHEDULES[name])
        return int(SCHEDULES[name])
    return 2


def hits(g, b):
    return dict(zip(HIT_NAMES, g.bounce_hits_cache_stats(b)))


def cache_stats(g):
    d = {"rng": g.rng_cache_stats(), "hit": g.hit_cache_stats(), "vis": g.vis_cache_stats(), "hit1": g.hit1_cache_stats(),
         "cont": g.cont_cache_stats(), "hit2": g.hit2_cache_stats(), "vis1": g.vis1_cache_stats()}
    assert d["hit1"] == g.bounce_hits_cache_stats(1) and d["hit2"] == g.bounce_hits_cache_stats(2) and d["vis1"] == g.bounce_vis_cache_stats(1)
    for b in (3, 4, 5):
        d[f"hits{b}"] = g.bounce_hits_cache_stats(b)
    for b in (2, 3, 4):
        d[f"vis{b}"] = g.bounce_vis_cache_stats(b)
    return d


def rays_per_bounce(pta, oracle, bounces, **kw):
    """[(rays, hits)] by bounce 0 .. bounces of the opaque terrace under the point light, from the oracle's counts: segments
    and shaded hits at depth b minus those at depth b - 1."""
    out, prev = [], (0, 0)
    for b in range(bounces + 1):
        case, scene, prof = terrace(pta, "point", bounces=b, **kw)
        st = oracle_frame(oracle, scene, prof)[2]
        out.append((st["segments"] - prev[0], st["shaded_hits"] - prev[1]))
        prev = (st["segments"], st["shaded_hits"])
    return out


def masked(pta, g, prof, want, what, **shard):
    """(masked_casts, bounce0_masked) of an instrumented frame of the scene as it stands - and that frame is the oracle's too.
    shard: the keywords of Opts.make of a sharded frame (`want` is that rank's pixels then, its counts the whole frame's)."""
    assert_same(g.render(prof, pta.Opts.make(flags=pta.PT_FLAG_COUNTERS, **shard)), want, (what, "instrumented"))
    c = g.counters().as_dict()
    assert c["segments"] == want[2]["segments"] or shard, (what, c["segments"], want[2]["segments"])
    return c["masked_casts"], c["bounce0_masked"]


def expect_caches(k, lights):
    """What the caches' counters say after frame k (0-based) of a fresh opaque terrace scene of one chunk per frame, whatever
    the masks do meanwhile: {cache: {field index: value}}.  Frame 0 keys nothing; frame 1 keys, zeroes and stores (fills) every
    cache; every later frame loads once.  lights: 1-4 lights (the visibility planes exist)."""
    if k == 0:
        return None
    e = {"rng": {3: 1}, "hit": {3: 1, 4: k - 1}}
    for b in REACHED:
        e["hit1" if b == 1 else "hit2" if b == 2 else f"hits{b}"] = {3: 1, 4: 1, 5: k - 1, 6: 0}
    for b in UNREACHED:   # (whether an empty queue gets a storing launch is the plan's business: a planned frame leaves it out)
        e[f"hits{b}"] = {3: 1, 6: 0}
    e["cont"] = {3: 1, 4: 1, 6: 0}
    if lights:   # (zeroed once and never again; bounce 0's variant runs in every chunk that loads its camera hits)
        e["vis"] = {2: 1, 3: k - 1}
        for b in REACHED:   # (one launch of k_og_shadow_vis per frame from the keying frame on: launched, never inline)
            e[f"vis{b}"] = {2: 1, 3: k}
    return e


def check_caches(g, k, lights, what):
    st = cache_stats(g)
    print(what, "frame", k, st)
    e = expect_caches(k, lights)
    if e is None:
        assert all(not any(v) for v in st.values()), (what, k, st)
        return st
    items = st["rng"][1]
    assert items == (W // 32) * ((H + 31) // 32) * 32 * 32 * SPP and st["rng"][2] == items, (what, k, st["rng"])
    for name, fields in e.items():
        assert st[name][1] == items, (what, k, name, st[name])
        for idx, value in fields.items():
            assert st[name][idx] == value, (what, k, name, idx, st[name], value)
    if not lights:
        assert all(not any(st[n]) for n in ("vis", "vis1", "vis2", "vis3", "vis4")), (what, k, st)
    return st


# -------------------------------------------------------------------------------------------------------------------------
# the geometry, on the CPU
# -------------------------------------------------------------------------------------------------------------------------
def test_terrace_is_fit_for_a_gpu(pta, oracle):
    """No GPU: every ray of every profile the GPU tests below render is finite and the oracle reports no numeric error
    (oracle_frame asserts both; the paths of 5 bounces are prefixes of those of 8, so the 8-bounce profiles are the ones
    walked), most secondary rays leave the scene, the geometry stays out of the shading matrix - and what the expected cache
    counters rest on: which bounces have a ray, and that no bounce's shadow casts can go inline."""
    from test_prestaged_misses import secondary_miss_share
    assert "terrace" in sb.MASKED_GEOMETRIES and "terrace" not in sb.GEOMETRIES
    assert all(c.geometry in sb.GEOMETRIES for c in sb.cases())
    for light_set in ("none", "point", "five", "point_dir", "dir_short"):
        for factor_set in ("opaque", "alpha"):
            for bounces in (BOUNCES, 8):
                case, scene, prof = terrace(pta, light_set, factor_set, bounces)
                assert scene.n_triangles <= 300 and scene.translucent == (factor_set == "alpha")
                want = oracle_frame(oracle, scene, prof, walk=bounces == 8)
                assert want[2]["numeric_errors"] == 0
    # the other views, sizes and sample counts: the far camera, the sharded frame, the films' passes and windows
    for kw in (dict(camera=far_camera(pta)), dict(size=(70, 33)), dict(spp=2), dict(spp=8), dict(spp=16)):
        case, scene, prof = terrace(pta, "point", bounces=8, **kw)
        assert oracle_frame(oracle, scene, prof, walk=True)[2]["numeric_errors"] == 0
    case, scene, prof = terrace(pta, "point")
    share = secondary_miss_share(oracle, scene, case, W, H, SPP, BOUNCES)
    print(f"terrace: {share:.3f} of the casts of bounces >= 1 leave the scene")
    assert share >= 0.4, share
    # REACHED / UNREACHED, and the far view of the camera test: at bounces 1-4 some ray hits, behind them there is none
    for kw in ({}, dict(camera=far_camera(pta))):
        counts = rays_per_bounce(pta, oracle, 8, **kw)
        print("rays, hits by bounce", kw and "far", counts)
        assert all(counts[b][1] > 0 for b in REACHED), counts
        if not kw:
            assert all(counts[b] == (0, 0) for b in range(UNREACHED[0], 9)), counts
            # make_plan puts a bounce's shadow casts inline where it counted shadow records for 60 % of the bounce's rays.  A
            # record needs a hit: h of r rays in the oracle, at most 49 %.  The masks shift that share only a little: under a
            # live light they end a ray only where it leaves a surface with no record pending - one the light does not reach,
            # or one whose lights the shade pass added itself, and then the frame counts hardly any record at all.  (If a
            # plan did go inline the expected launches would be missed, loudly: the premise cannot make a test pass.)
            assert all(10 * counts[b][1] < 6 * counts[b][0] for b in REACHED), counts


# -------------------------------------------------------------------------------------------------------------------------
# a. the geometry is not vacuous
# -------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("factor_set", ["opaque", "alpha"])
@pytest.mark.parametrize("light_set", ["none", "point", "five", "point_dir"])
def test_the_masks_of_terrace_end_paths(pta, oracle, monkeypatch, light_set, factor_set):
    """Masks live: masked_casts > 0 and bounce0_masked > 0.  PT_ESCAPE=0: both 0, the same bits.  Printed: the share of the
    oracle's secondary misses that the masks answered (recorded in DESIGN.md; a property of the geometry, no threshold)."""
    case, scene, prof = terrace(pta, light_set, factor_set)
    want = want_of(oracle, scene, prof, light_set, factor_set)
    flat = want_of(oracle, scene, sb.profile(case, W, H, SPP, bounces=0), light_set, factor_set)
    schedule(monkeypatch, "after-0")
    g = pta.GpuScene(scene)
    with_masks = g.render(prof)
    assert_same(with_masks, want, (light_set, factor_set, "masks"))
    info = g.info().as_dict()
    m, m0 = masked(pta, g, prof, want, (light_set, factor_set))
    g.close()
    if factor_set == "opaque":   # (one shaded hit per cast that hits)
        misses = (want[2]["segments"] - flat[2]["segments"]) - (want[2]["shaded_hits"] - flat[2]["shaded_hits"])
        print(f"terrace {light_set}: masks on {info['escape_prims']} of {info['n_prims']} primitives, masked_casts {m} (bounce 0: {m0}) "
              f"of {misses} secondary misses: {m / misses:.3f}")
    else:
        print(f"terrace {light_set} alpha: masks on {info['escape_prims']} of {info['n_prims']} primitives, masked_casts {m} (bounce 0: {m0})")
    assert info["escape_prims"] > 0 and m > 0 and m0 > 0 and m >= m0, (info, m, m0)
    schedule(monkeypatch, "no-masks")
    g = pta.GpuScene(scene)
    without = g.render(prof)
    assert_same(without, want, (light_set, factor_set, "no masks"))
    assert_same(without, with_masks, (light_set, factor_set, "masks vs none"))
    assert masked(pta, g, prof, want, (light_set, factor_set, "no masks")) == (0, 0) and g.info().escape_prims == 0
    g.close()


# -------------------------------------------------------------------------------------------------------------------------
# b. arrival schedules
# -------------------------------------------------------------------------------------------------------------------------
def arrival_sequence(pta, g, prof, want, arrival, what, lights, opaque, opts=None, frames=7):
    """`frames` frames of a fresh scene: each the oracle's; escape_prims > 0 from the arrival frame on; the plan counted in
    frame 0 and again in the arrival frame; the caches as expect_caches says (opaque scenes; a translucent one has none but
    the words)."""
    seen = []
    for k in range(frames):
        got = g.render(prof, opts) if opts is not None else g.render(prof)
        assert_same(got, want, (what, k))
        info = g.info().as_dict()
        seen.append((info["escape_prims"] > 0, info["frame_planned"]))
        if opts is not None:
            continue
        if opaque:
            check_caches(g, k, lights, what)
        else:
            st = cache_stats(g)
            print(what, "frame", k, st)
            assert all(not any(v) for name, v in st.items() if name != "rng"), (what, k, st)
    print(what, seen)
    assert [s[0] for s in seen] == [arrival is not None and k >= arrival for k in range(frames)], (what, seen)
    assert [s[1] for s in seen] == [0 if k in (0, arrival) else 1 for k in range(frames)], (what, seen)


@gpu
@pytest.mark.parametrize("name", ["opaque-point", "opaque-none", "alpha-point"])
@pytest.mark.parametrize("sched", list(SCHEDULES))
def test_masks_arrive_under_caches_that_were_stored_without_them(pta, oracle, monkeypatch, sched, name):
    """Seven frames of a fresh scene per schedule.  default and after-4: frame 1 keys and stores every cache WITHOUT masks,
    the arrival frame (2 / 4) and those behind it load under them; after-0 / after-1: stored with them; no-masks: never.  The
    counters are the same in all five (no key holds the masks), and no load ever meets an item without a record."""
    factor_set, light_set = name.split("-")
    case, scene, prof = terrace(pta, light_set, factor_set)
    want = want_of(oracle, scene, prof, light_set, factor_set)
    arrival = schedule(monkeypatch, sched)
    g = pta.GpuScene(scene)
    arrival_sequence(pta, g, prof, want, arrival, (sched, name), light_set != "none", factor_set == "opaque")
    if factor_set == "opaque":   # (said again where the issue asks for it: stored before arrival, loaded after it)
        st = cache_stats(g)
        loads = {n: st[n][5] for n in ("hit1", "hit2", "hits3", "hits4")}
        loads["hit"] = st["hit"][4]
        assert all(v == 5 for v in loads.values()), loads
        assert light_set == "none" or (st["cont"][5] > 0 and st["vis"][3] == 5), st
        # the shadow-visibility planes of bounces 1-4: in use since the keying frame (1 launch by then: before any arrival but
        # after-0's and after-1's), and in every frame since - 6 by the last, the arrival frame and those behind it included
        assert light_set == "none" or all(st[f"vis{b}"][2:] == (1, 6) for b in REACHED), st
    m, m0 = masked(pta, g, prof, want, (sched, name))
    print(sched, name, "masked_casts", m, "bounce0_masked", m0)
    assert (m > 0 and m0 > 0) if arrival is not None else (m, m0) == (0, 0), (sched, name, m, m0)
    g.close()


# -------------------------------------------------------------------------------------------------------------------------
# c. the natural hole
# -------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("first,second", [("none", "point"), ("dir_short", "point"), ("point", "none")])
def test_a_light_edit_revives_paths_the_masks_ended_while_the_planes_were_filled(pta, oracle, monkeypatch, first, second):
    """Masks from frame 0, 8 bounces.  Under `none` (no light) and `dir_short` (one light, moot on every surface that faces
    up) no path of the ground, the slab or the box's top carries a shadow record, so the masks end it at shade time and the
    planes of bounces 1-3 are filled without a record for it.  set_lights to `point`: the long normals of the slab and the
    panel go through the shadow queue at bounce 0, every lit surface does at the later bounces until its visibility is known -
    those paths are alive, have no record and are cast: unknown > 0 in the planes of bounces 1, 2 and 3, no study switch set.
    Then the edit back.  point -> none -> point is the reverse: the planes are filled with every record, fewer are read.
    (What such an item can show: its ray was PROVEN a miss when the plane was filled, so the cast it gets finds nothing - a
    loader that read "no record" as a miss would render the same frames; one that read a hit there - a stale record, another
    item's - would not.)"""
    schedule(monkeypatch, "after-0")
    state = {}
    for ls in (first, second):
        case, scene, prof = terrace(pta, ls, bounces=8)
        state[ls] = (scene, want_of(oracle, scene, prof, ls, "opaque"))
    assert not np.array_equal(state[first][1][1], state[second][1][1])
    g = pta.GpuScene(state[first][0])
    res = g.info().as_dict()["cam_grid_res"]
    for k in range(4):
        assert_same(g.render(prof), state[first][1], (first, k))
    filled = {b: hits(g, b) for b in (1, 2, 3)}
    assert all(st["stores"] == 1 and st["loads"] == 2 and st["unknown"] == 0 for st in filled.values()), filled
    m, m0 = masked(pta, g, prof, state[first][1], (first, "filled"))
    assert g.info().escape_prims > 0 and m0 > 0 and (m > m0 or first == "point"), (m, m0)
    for ls in (second, first):
        g.set_lights(sb.make_lights(pta, ls))
        assert g.info().as_dict()["cam_grid_res"] == res   # (the premise: the edit re-keys no hit plane)
        for k in range(3):
            assert_same(g.render(prof), state[ls][1], (first, "->", ls, k))
        now = {b: hits(g, b) for b in (1, 2, 3)}
        print(first, "->", ls, "masked while filled", (m, m0), now)
        for b in (1, 2, 3):
            assert (now[b]["resets"], now[b]["stores"]) == (1, 1) and now[b]["loads"] > filled[b]["loads"], (ls, b, now[b])
            if first == "point":
                assert now[b]["unknown"] == 0, (ls, b, now[b])
            else:
                assert now[b]["unknown"] > 0, (ls, b, now[b])
        filled = now
    g.close()


# -------------------------------------------------------------------------------------------------------------------------
# d. masks lost and rebuilt under serving caches
# -------------------------------------------------------------------------------------------------------------------------
def far_camera(pta, factor=2.0):
    """The camera of test_camera_update.cameras' "far" recipe: the same orientation, the eye moved away from the middle of
    the scene (delta_in grows with the scene's reach from the eye)."""
    eye, target, pivot = np.array(CAMERA["eye"]), np.array(CAMERA["target"]), np.array([0.0, 0.5, -0.2])
    far = pivot + factor * (eye - pivot)
    return sb.make_camera(pta, eye=tuple(far), target=tuple(far + (target - eye)), fov=CAMERA["fov"])


@gpu
@pytest.mark.parametrize("sched", ["default", "after-0"])
def test_masks_lost_and_rebuilt_under_serving_caches(pta, oracle, monkeypatch, sched):
    """Four frames at A (masks live, caches loading), set_camera to a camera twice as far out: the masks go at once, the
    schedule starts again (default: they return with that view's third frame, a loading frame), the move re-keys the hit
    caches; four frames there; back to A - the masks of the larger delta_in stay - three frames.  Every frame is the oracle's
    for its camera."""
    arrival = schedule(monkeypatch, sched)
    cams = {"A": sb.make_camera(pta, **CAMERA), "far": far_camera(pta)}
    state = {}
    for label, cam in cams.items():
        case, scene, prof = terrace(pta, "point", camera=cam)
        state[label] = (scene, want_of(oracle, scene, prof, "point", "opaque", label))
    assert not np.array_equal(state["A"][1][1], state["far"][1][1])
    g = pta.GpuScene(state["A"][0])
    arrival_sequence(pta, g, prof, state["A"][1], arrival, (sched, "A"), True, True, frames=4)
    before, vis1 = hits(g, 1), g.vis1_cache_stats()
    assert before["loads"] == 2 and g.info().escape_prims > 0 and vis1[2:] == (1, 3)
    for label, frames, live in (("far", 4, [k >= arrival for k in range(4)]), ("A", 3, [True] * 3)):
        g.set_camera(cams[label])
        assert (g.info().escape_prims > 0) == (label == "A"), label   # (dropped by the move out, kept by the move in)
        seen = []
        for k, (dr, ds, dl) in zip(range(frames), [(0, 0, 0), (1, 1, 0), (0, 0, 1), (0, 0, 1)]):
            assert_same(g.render(prof), state[label][1], (sched, label, k))
            info = g.info().as_dict()
            seen.append((info["escape_prims"] > 0, info["frame_planned"]))
            for b in REACHED:
                st = hits(g, b)
                want_counts = (before["resets"] + dr, before["stores"] + ds, before["loads"] + dl)
                assert (st["resets"], st["stores"], st["loads"], st["unknown"]) == want_counts + (0,), (sched, label, k, b, st)
            before = hits(g, 1)
            # bounce 1's visibility plane, re-keyed with the hits (a quarter of that bounce's rays hit in either view: never
            # inline): zeroed in the view's second frame and launched on from there, through the frame the masks return in
            now = g.vis1_cache_stats()
            assert now[2:] == (vis1[2] + dr, vis1[3] + (k >= 1)), (sched, label, k, now, vis1)
            vis1 = now
        print(sched, label, seen, cache_stats(g))
        assert [s[0] for s in seen] == live, (sched, label, seen)
        # the plan: dropped by the move, counted in the view's first frame and again in the frame the masks are built in
        built = arrival if label == "far" else None
        assert [s[1] for s in seen] == [0 if k in (0, built) else 1 for k in range(frames)], (sched, label, seen)
    m, m0 = masked(pta, g, prof, state["A"][1], (sched, "back at A"))
    assert m > 0 and m0 > 0 and hits(g, 1)["loads"] == 2 + 2 + 1
    g.close()


# -------------------------------------------------------------------------------------------------------------------------
# e. what advances the schedule
# -------------------------------------------------------------------------------------------------------------------------
@gpu
def test_only_whole_default_pipeline_frames_advance_the_schedule(pta, oracle, monkeypatch):
    """PT_ESCAPE_AFTER unset.  KD-only frames, megakernel frames, tile-list frames and sample windows between the default
    frames (render, render_moments, render_device): the masks are there exactly from the third counted frame on, and every
    frame of every kind is the oracle's - tile lists by their pixel map, windows as chained sums that end as the 4-sample
    accumulator (the boundary at 2 samples is the oracle's 2-sample prefix)."""
    import torch
    schedule(monkeypatch, "default")
    case, scene, prof = terrace(pta, "point")
    want = want_of(oracle, scene, prof, "point", "opaque")
    half = want_of(oracle, scene, prof, "point", "opaque", sample_count=2)
    g = pta.GpuScene(scene)
    n = W * H

    def default(k):
        assert_same(g.render(prof), want, ("render", k))

    def moments(k):
        assert_same(g.render_moments(prof)[:2], want, ("render_moments", k))

    def device(k):
        rgb = torch.empty(n * 3, dtype=torch.uint8, device="cuda")
        acc = torch.empty(n * 3, dtype=torch.float32, device="cuda")
        g.render_device(prof, pta.Opts.make(), rgb.data_ptr(), acc.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert_same((rgb.cpu().numpy().reshape(-1, 3), acc.cpu().numpy().reshape(-1, 3)), want, ("render_device", k))

    def kd(k):
        assert_same(g.render(prof, pta.Opts.make(flags=pta.PT_FLAG_NO_GRIDS)), want, ("kd", k))

    def mega(k):
        assert_same(g.render(prof, pta.Opts.make(flags=pta.PT_FLAG_MEGAKERNEL)), want, ("megakernel", k))

    def tiles(k):
        t = [0, 3] if k % 2 else [1, 2]
        rgb, acc, _ = g.render_tiles(prof, t)
        m = pta.tiles_pixel_map(prof, t)
        assert len(m) > 0
        assert_same((rgb, acc), (want[0][m], want[1][m]), ("tiles", k))

    def window(k):
        rgb, acc, mom = g.render_window(prof, 0, 2)
        assert_same((rgb, acc), (oracle.post_process(sb.profile(case, W, H, 2), half[1]), half[1]), ("window [0, 2)", k))
        rgb, acc, mom = g.render_window(prof, 2, 4, acc, mom)
        assert_same((rgb, acc), want, ("window [2, 4)", k))

    counted = 0
    order = [kd, default, mega, tiles, window, moments, kd, tiles, window, device, mega, kd, tiles, window, default, default]
    for k, kind in enumerate(order):
        kind(k)
        counted += kind in (default, moments, device)
        live = g.info().escape_prims > 0
        print(k, kind.__name__, "counted", counted, "masks", live)
        assert live == (counted >= 3), (k, kind.__name__, counted, live)
    assert counted == 5
    st = cache_stats(g)
    print(st)
    assert st["hit"][4] > 0 and st["hit1"][5] > 0 and st["hit1"][6] == 0, st
    m, m0 = masked(pta, g, prof, want, "interleaved")
    assert m > 0 and m0 > 0
    g.close()


# -------------------------------------------------------------------------------------------------------------------------
# f. shards
# -------------------------------------------------------------------------------------------------------------------------
@gpu
def test_the_default_schedule_on_three_shards(pta, oracle, monkeypatch):
    """The default-schedule sequence with shard_count = 3, 16 x 16 tiles and a 70 x 33 frame: every rank a scene of its own
    with masks and caches of its own, every frame of every rank the oracle's pixels of that rank."""
    arrival = schedule(monkeypatch, "default")
    case, scene, prof = terrace(pta, "point", size=(70, 33))
    want = want_of(oracle, scene, prof, "point", "opaque")
    total = [0, 0]
    covered = np.zeros(70 * 33, bool)
    for rank in range(3):
        shard = dict(shard_rank=rank, shard_count=3, tile_w=16, tile_h=16)
        o = pta.Opts.make(**shard)
        m = pta.local_pixel_map(prof, o)
        assert len(m) > 0 and not covered[m].any()
        covered[m] = True
        local = (want[0][m], want[1][m], want[2])
        g = pta.GpuScene(scene)
        arrival_sequence(pta, g, prof, local, arrival, ("rank", rank), True, True, opts=o)
        st = cache_stats(g)
        print("rank", rank, st)
        assert st["rng"][3] == 1 and st["hit"][3:] == (1, 5) and st["hit1"][3:] == (1, 1, 5, 0) and st["hit2"][3:] == (1, 1, 5, 0), st
        assert st["vis"][2:] == (1, 5) and st["vis1"][2] == 1 and st["vis1"][3] > 0, st
        mm = masked(pta, g, prof, local, ("rank", rank), **shard)
        print("rank", rank, "masked_casts, bounce0_masked", mm)
        total = [total[0] + mm[0], total[1] + mm[1]]
        g.close()
    assert covered.all() and total[0] > 0 and total[1] > 0, total


# -------------------------------------------------------------------------------------------------------------------------
# g. films across arrival
# -------------------------------------------------------------------------------------------------------------------------
@gpu
def test_a_uniform_film_whose_third_pass_is_the_arrival_frame(pta, oracle, monkeypatch):
    """Passes of 2, 4 and 8 samples under the unset schedule - each a whole default-pipeline frame, the third built with the
    masks: the film's accum is the f32 sum of the oracle's three accumulators in pass order (film_model.merge)."""
    schedule(monkeypatch, "default")
    case, scene, prof = terrace(pta, "point")
    frames = {n: want_of(oracle, scene, sb.profile(case, W, H, n), "point", "opaque") for n in (2, 4, 8)}
    g = pta.GpuScene(scene)
    film = pta.Film(prof)
    want = np.zeros((W * H, 3), np.float32)
    live = []
    for n in (2, 4, 8):
        film.add_pass(g, n)
        live.append(g.info().escape_prims > 0)
        want = fm.merge(want, frames[n][1])
        got = film.read()[0]
        assert_same((np.zeros(0), got), (np.zeros(0), want), ("film after the pass of", n))
    assert live == [False, False, True], live
    assert (film.info.samples, film.info.passes) == (14, 3)
    m, m0 = masked(pta, g, sb.profile(case, W, H, 8), frames[8], "film")
    assert m > 0 and m0 > 0
    film.close()
    g.close()


@gpu
def test_a_windowed_film_across_arrival(pta, oracle, monkeypatch):
    """A windowed film (W = 4 of N = 16) under the unset schedule.  Its windows are detached frames and advance nothing, so
    three whole frames between them bring the masks: the last window is rendered with them, the first three without, and the
    film ends as the oracle's 16-sample frame, bit for bit."""
    schedule(monkeypatch, "default")
    case, scene, prof4 = terrace(pta, "point")
    prof16 = sb.profile(case, W, H, 16)
    want4, want16 = want_of(oracle, scene, prof4, "point", "opaque"), want_of(oracle, scene, prof16, "point", "opaque")
    g = pta.GpuScene(scene)
    film = pta.Film.windowed(prof16)
    live = []
    for k in range(4):
        film.add_window(g, 4)
        live.append(g.info().escape_prims > 0)
        prefix = want_of(oracle, scene, prof16, "point", "opaque", sample_count=4 * (k + 1))
        assert_same((np.zeros(0), film.read()[0]), (np.zeros(0), prefix[1]), ("windows", k + 1))
        if k < 3:
            assert_same(g.render(prof4), want4, ("frame between the windows", k))
    assert live == [False, False, False, True], live
    assert (film.info.samples, film.window_info.windows) == (16, 4)
    assert_same((film.resolve(), film.read()[0]), want16, "the film")
    m, m0 = masked(pta, g, prof16, want16, "windowed film")
    assert m > 0 and m0 > 0
    g.close()
    film.close()
