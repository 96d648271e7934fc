"""The lean variant of the loading bounce-0 launch (csrc/pt_wf_shade_body.h LEAN, k_wf_shade_hits<2283 | 4096>; csrc/pt_gpu.hip
lean_frame, frame_plan, render_chunk).  A steady frame - every cache loaded, every light's visibility known, every record with
its escape answer - makes no shadow cast, runs no escape test and writes no shadow record, so a configuration whose last
counted frame was such a frame launches a variant of the kernel without that code: 96 registers and 12 KiB of LDS, five waves
per SIMD.  A lane that needs the missing code all the same writes nothing and flags the frame.

What could go wrong: a frame that goes lean too early (unknown visibility, records without answers, surfaces that take the
shadow queue), one that stays lean across an edit, a re-keyed cache or new masks, the late records read from another thread's
LDS slot or a stale step's, a partial last step, a guard that writes.  Every frame of every sequence is compared bit for bit -
rgb8 and the f32 accumulator - with the same sequence under PT_B0_LEAN=0, and every test reads the launch counts that make
it mean something (GpuScene.b0_lean_stats).

The scene: the floor of `terrace` as 14 x 14 quads, its box and the ball (404 triangles and a sphere, every normal of length
one: no surface takes the shadow queue) under three point lights, 70 x 38 pixels (partial pixel blocks, a partial last step),
4 spp, 3 bounces."""
import numpy as np
import pytest

import scene_builder as sb
from test_masked_sequences import schedule
from test_prestaged_misses import CAMERA, assert_same, oracle_frame

gpu = pytest.mark.gpu

W, H, SPP, BOUNCES = 70, 38, 4, 3
NAMES = ("lean", "general", "guard")


def lean_lights(pta, third=(0.0, 0.0, 0.0), first_at=(0.4, 3.3, 0.9)):
    P = pta.PT_LIGHT_POINT
    return [sb._light(pta, P, first_at, (160.0, 150.0, 140.0)), sb._light(pta, P, (-1.0, 3.0, 0.2), (60.0, 70.0, 80.0)),
            sb._light(pta, P, (1.5, 2.5, -1.0), third)]


def lean_scene(pta, lights=None, materials=None, camera=None, factor_set="opaque", wall=False):
    """floor (14 x 14 quads), box, ball; wall: terrace's slab with vertex normals of length 4 and 0.5 as well."""
    case = sb.Case("lean", "terrace", "none", "point", factor_set, BOUNCES, "FILMIC", 0, False)
    mats = materials if materials is not None else sb.case_materials(case, pta)   # (fills sb._TEX)
    tex, texels, _ = sb._TEX["t"]
    groups = {"floor": [], "box": sb._terrace()["box"]}
    if wall:
        groups["wall"] = sb._terrace()["wall"]
    n, dx, dz = 14, 4.0 / 14, 3.6 / 14
    normal = lambda x, z: sb._unit([0.035 * np.sin(1.7 * x + 0.3), 1.0, 0.035 * np.cos(2.1 * z)])
    for i in range(n):
        for j in range(n):
            x, z = -2.0 + i * dx, 1.6 - j * dz
            ns = [normal(x, z), normal(x + dx, z), normal(x + dx, z - dz), normal(x, z - dz)]
            uv0 = (-2.5 + 1.3 * (x + 2.0) + 0.23 * (1.6 - z), -2.5 + 0.2 * (x + 2.0) + 1.45 * (1.6 - z))
            groups["floor"] += sb._quad((x, 0.0, z), (dx, 0, 0), (0, 0, -dz), ns, uv0, (1.3 * dx, 0.2 * dx), (0.23 * dz, 1.45 * dz))
    tris, models = [], []
    import ctypes as C
    for k, name in enumerate(sb.MATERIALS):
        if name == "ball":
            models.append(pta.Model(pta.PT_MODEL_SPHERE, k, 0, 0, (C.c_float * 3)(0.7, 0.55, -0.3), 0.5))
        elif name in groups:
            models.append(pta.Model(pta.PT_MODEL_MESH, k, len(tris), len(groups[name]), (C.c_float * 3)(0, 0, 0), 0.0))
            tris += groups[name]
    tris = np.array(tris, np.float32).reshape(-1, 24)
    scene = sb.BuiltScene(pta, tris, models, mats, tex, texels, lights if lights is not None else lean_lights(pta),
                          camera or sb.make_camera(pta, **CAMERA), (0.25, 0.3, 0.45))
    return case, scene, pta.Profile.make(W, H, SPP, BOUNCES, "FILMIC")


def stats(g):
    return dict(zip(NAMES, g.b0_lean_stats()))


def sequence(pta, monkeypatch, scene, prof, frames, lean, edits=None, opts=None):
    """`frames` frames of a fresh GpuScene with PT_B0_LEAN=lean; edits: {frame: function(g)} applied before that frame.
    Returns per frame (rgb8, accum) and (lean launches, general launches, planned) of that frame alone."""
    monkeypatch.setenv("PT_B0_LEAN", lean)
    g = pta.GpuScene(scene)
    out, seen, before = [], [], stats(g)
    for k in range(frames):
        if edits and k in edits:
            edits[k](g)
        out.append(g.render(prof, opts) if opts is not None else g.render(prof))
        now = stats(g)
        assert now["guard"] == 0, (k, now)
        seen.append((now["lean"] - before["lean"], now["general"] - before["general"], int(g.info().frame_planned)))
        before = now
    g.close()
    return out, seen


def both(pta, monkeypatch, scene, prof, frames, what, edits=None, opts=None):
    """The sequence with the switch off and on: the same frames bit for bit; returns the per-frame launches of the second."""
    ref, seen_off = sequence(pta, monkeypatch, scene, prof, frames, "0", edits, opts)
    got, seen = sequence(pta, monkeypatch, scene, prof, frames, "1", edits, opts)
    print(what, "off:", seen_off)
    print(what, "on: ", seen)
    assert all(s[0] == 0 for s in seen_off), (what, seen_off)
    assert [s[0] + s[1] for s in seen] == [s[1] for s in seen_off] and [s[2] for s in seen] == [s[2] for s in seen_off], (what, seen, seen_off)
    for k in range(frames):
        assert_same(got[k], ref[k], (what, k))
    for k, s in enumerate(seen):   # a frame is lean or general as a whole, and a lean one follows a planned, loading one
        assert s[0] == 0 or s[1] == 0, (what, k, s)
        if s[0]:
            assert s[2] == 1 and k > 0 and seen[k - 1][2] == 1 and seen[k - 1][0] + seen[k - 1][1] > 0, (what, k, seen)
    return seen, got


def first_lean(seen, start=0):
    return next((k for k in range(start, len(seen)) if seen[k][0]), None)


def test_the_library_has_the_getter(pta):
    """No GPU: the symbol is there."""
    assert "pt_get_b0_lean_stats" in pta.GPU_SYMBOLS and len(pta.gpu_lib().pt_get_b0_lean_stats.argtypes) == 4


def test_the_lean_variant_fits_five_waves(tmp_path):
    """From the built library: at most 96 registers (512 / 5, in the allocation's granules of 8), no scratch, at most 32 KiB of
    LDS a workgroup (160 KiB / 5); the general variants stay as they were."""
    from test_kernel_resources import find, kernel_table
    t = kernel_table(tmp_path)
    lean = find(t, "k_wf_shade_hitsILi6379EE")
    print(lean)
    assert lean["vgpr_count"] <= 96 and lean["private_segment_fixed_size"] == 0 and lean["group_segment_fixed_size"] <= 32 * 1024, lean
    general = find(t, "k_wf_shade_hitsILi2283EE")
    assert general["vgpr_count"] <= 128 and general["private_segment_fixed_size"] == 0 and general["group_segment_fixed_size"] <= 40 * 1024, general


@gpu
def test_a_fresh_scene_goes_lean_behind_its_first_clean_frame(pta, oracle, monkeypatch):
    """Default schedule, eight frames.  Frame 0 counts, 1 stores, the masks arrive before 2, which counts again and fills the
    visibility (its lanes cast: not clean); frame 3 is planned, loads everything and casts nothing - the first clean frame;
    frames 4-7 are lean.  All eight are the oracle's frame as well."""
    case, scene, prof = lean_scene(pta)
    assert scene.n_triangles == 404 and not scene.translucent
    want = oracle_frame(oracle, scene, prof, walk=True)
    schedule(monkeypatch, "default")
    seen, got = both(pta, monkeypatch, scene, prof, 8, "fresh")
    assert [s[2] for s in seen] == [0, 1, 0, 1, 1, 1, 1, 1], seen
    assert [s[0] > 0 for s in seen] == [False] * 4 + [True] * 4 and seen[3][1] > 0, seen
    for k in range(8):
        assert_same(got[k], want, ("oracle", k))


@gpu
@pytest.mark.parametrize("edit", ["light-move", "light-on", "material", "camera"])
def test_an_edit_ends_it_and_a_clean_frame_brings_it_back(pta, monkeypatch, edit):
    """Six frames (lean from frame 4 on), then the edit, then seven more: the frame behind the edit is general, the launches
    stay general until a planned frame has been counted clean, then they are lean again - and every frame is the frame of the
    sequence with the switch off."""
    case, scene, prof = lean_scene(pta)
    schedule(monkeypatch, "default")

    def apply(g):
        if edit == "light-move":
            g.set_lights(lean_lights(pta, first_at=(-0.8, 2.9, 0.4)))
        elif edit == "light-on":   # the third light was black: nothing it could add
            g.set_lights(lean_lights(pta, third=(90.0, 20.0, 40.0)))
        elif edit == "material":
            other = sb.case_materials(case, pta)
            for m in other:
                m.roughness = min(1.0, 0.37 + 0.5 * m.roughness)
            g.set_materials(other)
        else:
            g.set_camera(sb.make_camera(pta, eye=(-0.9, 2.1, 2.9), target=(0.3, 0.3, -0.4), fov=0.8))

    seen, got = both(pta, monkeypatch, scene, prof, 13, edit, edits={6: apply})
    assert seen[4][0] and seen[5][0], seen
    assert seen[6][0] == 0 and seen[6][2] == 0, seen   # (the counts are dropped with the edit: a first frame, and general)
    back = first_lean(seen, 6)
    assert back is not None and back >= 8 and all(s[0] for s in seen[back:]), (edit, back, seen)
    assert not np.array_equal(got[5][1], got[12][1]), edit   # (the edit changed the image)


@gpu
@pytest.mark.parametrize("after", ["0", "1", "2"])
def test_masks_that_arrive_late(pta, monkeypatch, after):
    """PT_ESCAPE_AFTER = 0, 1, 2: whenever the masks arrive, the launches go lean behind a planned frame that loaded records
    with answers, and stay lean."""
    case, scene, prof = lean_scene(pta)
    monkeypatch.delenv("PT_ESCAPE", raising=False)
    monkeypatch.setenv("PT_ESCAPE_AFTER", after)
    seen, _ = both(pta, monkeypatch, scene, prof, 8, ("after", after))
    k = first_lean(seen)
    assert k is not None and 3 <= k <= 5 and all(s[0] for s in seen[k:]), (after, seen)


@gpu
def test_surfaces_that_take_the_shadow_queue_never_go_lean(pta, monkeypatch):
    """With terrace's slab - vertex normals of length 4 and 0.5, longer than the light grids' margin - bounce 0 writes shadow
    records in every frame: no frame is clean."""
    case, scene, prof = lean_scene(pta, wall=True)
    t = np.asarray(scene._tris).reshape(-1, 3, 8)
    assert int(((t[:, :, 3:6] ** 2).sum(axis=2) > 2.25).sum()) > 0
    schedule(monkeypatch, "default")
    seen, _ = both(pta, monkeypatch, scene, prof, 8, "wall")
    assert first_lean(seen) is None and sum(s[1] for s in seen) >= 5, seen


@gpu
@pytest.mark.parametrize("kind", ["orthographic", "translucent"])
def test_scenes_that_never_go_lean(pta, monkeypatch, kind):
    """A directional light compiles the orthographic branch in (variant 2287 stays), a translucent table keys no cache."""
    if kind == "orthographic":
        lights = lean_lights(pta)[:2] + [sb._light(pta, pta.PT_LIGHT_DIRECTIONAL, 10.0 * sb._unit([-0.3, -0.9, -0.25]), (0.5, 0.6, 0.7))]
        case, scene, prof = lean_scene(pta, lights=lights)
    else:
        case, scene, prof = lean_scene(pta, factor_set="alpha")
        assert scene.translucent
    schedule(monkeypatch, "default")
    seen, _ = both(pta, monkeypatch, scene, prof, 7, kind)
    assert first_lean(seen) is None, seen
    assert (sum(s[1] for s in seen) > 0) == (kind == "orthographic"), seen


@gpu
def test_a_frame_in_several_chunks(pta, monkeypatch):
    """1056 x 768 x 4 items (3.1 Mi), two bounces, queue budgets that leave the planned frame in chunks of 1 Mi items: several
    lean launches a frame, the last one on a partial chunk."""
    case, scene, _ = lean_scene(pta)
    prof = pta.Profile.make(1056, 768, SPP, 2, "FILMIC")
    schedule(monkeypatch, "after-0")
    monkeypatch.setenv("PT_QUEUE_GIB", "0.01")
    monkeypatch.setenv("PT_QUEUE_STEADY_GIB", "0.02")
    monkeypatch.setenv("PT_QUEUE_ONE_PASS_GIB", "0.02")
    seen, _ = both(pta, monkeypatch, scene, prof, 6, "chunks")
    k = first_lean(seen)
    assert k is not None and seen[k][0] >= 3 and all(s[0] == seen[k][0] for s in seen[k:]), seen


@gpu
def test_two_shards(pta, monkeypatch):
    """shard_count = 2, 16 x 16 tiles: every rank a scene, a plan and an eligibility of its own."""
    case, scene, prof = lean_scene(pta)
    schedule(monkeypatch, "default")
    for rank in range(2):
        o = pta.Opts.make(shard_rank=rank, shard_count=2, tile_w=16, tile_h=16)
        seen, _ = both(pta, monkeypatch, scene, prof, 7, ("rank", rank), opts=o)
        assert first_lean(seen) == 4 and all(s[0] for s in seen[4:]), (rank, seen)


@gpu
def test_the_guard_flags_a_lean_launch_on_a_frame_that_is_not_clean(pta, monkeypatch):
    """What cannot happen made to happen: PT_B0_LEAN_TEST_FORCE puts the lean variant on frame 2 of a fresh scene, whose visibility
    plane is all unknown.  The launch must write nothing for those lanes (the image is not checked) and nothing it does not
    own; the NEXT call of the configuration must fail loudly, the frames after it are the right ones, and the launches go lean
    again by the rule."""
    case, scene, prof = lean_scene(pta)
    schedule(monkeypatch, "after-0")
    ref, _ = sequence(pta, monkeypatch, scene, prof, 3, "0")
    monkeypatch.setenv("PT_B0_LEAN", "1")
    g = pta.GpuScene(scene)
    for k in range(2):
        assert_same(g.render(prof), ref[k], ("before", k))
    assert stats(g) == {"lean": 0, "general": 0, "guard": 0}, stats(g)
    monkeypatch.setenv("PT_B0_LEAN_TEST_FORCE", "1")
    g.render(prof)
    monkeypatch.delenv("PT_B0_LEAN_TEST_FORCE")
    assert stats(g) == {"lean": 1, "general": 0, "guard": 0}, stats(g)
    with pytest.raises(pta.PtError, match="lean bounce-0 launch"):
        g.render(prof)
    assert stats(g)["guard"] == 1
    for k in range(5):
        assert_same(g.render(prof), ref[2], ("after", k))
    s = stats(g)
    assert s["guard"] == 1 and s["lean"] >= 2 and s["general"] >= 2, s
    g.close()
