"""The feature matrix of tests/scene_builder.py on the GPU: every case, and live walks through the matrix's materials and
lights, bit for bit against the CPU oracle on the three pipelines.  What the shade and shadow kernels do in feature
COMBINATIONS (one texture kind alone, an opacity texture on an otherwise opaque scene, spheres under a directional light only,
lights the kernels treat specially, a live edit that moves a scene between the opaque and the ALPHA kernel variants) is
rendered here and nowhere else.

Every frame that goes to the GPU is first walked on the CPU: every ray of every path finite (OracleScene.path_rays) and no
numeric error in the oracle.  Light COLOURS may be non-finite - they never reach a ray."""
import numpy as np
import pytest

import scene_builder as sb
import shading_model as sm

pytestmark = pytest.mark.gpu

CASES = sb.cases()
FLAG_SETS = (0, 4, 8)   # default, PT_FLAG_NO_GRIDS, PT_FLAG_MEGAKERNEL
FRAMES = ((96, 64, 3), (33, 17, 1))
COUNTERS = ("samples", "segments", "shadow_rays", "shaded_hits", "rng_draws")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_same(got, want, what):
    """rgb8 and the accumulator's bits (NaN == NaN: the kernels restate glibc bit for bit, payloads aside)."""
    assert np.array_equal(got[0], want[0]), (what, "rgb8", int((got[0] != want[0]).any(axis=1).sum()))
    g, w = np.asarray(got[1], np.float32), np.asarray(want[1], np.float32)
    same = (bits(g) == bits(w)) | (np.isnan(g) & np.isnan(w))
    assert same.all(), (what, "accum", int((~same).any(axis=1).sum()), "first", np.argwhere(~same)[0].tolist())


def cpu_walk(oracle, scene, prof, what):
    """The oracle's frame, after the checks that let the frame onto a GPU."""
    o = oracle.OracleScene(scene.desc, oracle.PTO_BRUTE_FORCE)
    assert sm.rays_finite(o, prof), (what, "a non-finite ray: stays on the CPU")
    rgb, acc, stats = o.render(prof)
    assert stats["numeric_errors"] == 0, what
    return rgb, acc, stats


def skipped(pta, g, prof, flags):
    g.render(prof, pta.Opts.make(flags=flags | pta.PT_FLAG_COUNTERS))
    return g.counters().as_dict()["shadow_skipped"]


@pytest.mark.parametrize("name", [c.name for c in CASES])
def test_case_equals_the_oracle(pta, oracle, name):
    case = sb.case_by_name(name)
    scene = sb.build(case)
    g = pta.GpuScene(scene)
    assert bool(g.info().has_translucent) == scene.translucent
    for w, h, spp in FRAMES:
        prof = sb.profile(case, w, h, spp)
        want = cpu_walk(oracle, scene, prof, (name, w, h))
        for flags in FLAG_SETS:
            assert_same(g.render(prof, pta.Opts.make(flags=flags)), want, (name, w, h, flags))
            got = g.render(prof, pta.Opts.make(flags=flags | pta.PT_FLAG_COUNTERS))
            assert_same(got, want, (name, w, h, flags, "counters"))
            c = g.counters().as_dict()
            assert {k: c[k] for k in COUNTERS} == {k: want[2][k] for k in COUNTERS}, (name, w, h, flags)
            assert c["shadow_skipped"] <= c["shadow_rays"]
            if case.moot and flags != pta.PT_FLAG_MEGAKERNEL:   # (the megakernel casts every shadow ray: nothing to skip)
                assert c["shadow_skipped"] > 0, (name, w, h, flags, "a light whose BRDF term is exactly 0 was cast")
    g.close()


@pytest.mark.parametrize("tex_kind", ["none", "roughness", "opacity"])
def test_wild_light_colours_are_never_skipped(pta, oracle, tex_kind):
    """A light with a colour component >= 1e30 or non-finite is not `tame`: its shadow ray is cast even where its BRDF term
    is exactly 0 (0 * inf is NaN, and the oracle says so).  Without those lights the frame skips exactly as many casts.  The
    light of colour 9e29 is on the tame side: without it the frame skips fewer.  (Default and KD-tree pipelines: the
    megakernel has no such skip - it casts every shadow ray - so its shadow_skipped says nothing.)"""
    case = sb.case_by_name(f"{tex_kind}-huge")
    scene = sb.build(case)
    tame = sb.build(case, lights=sb.tame_subset(pta, scene.lights))
    small = sb.build(case, lights=[l for l in tame.lights if max(l.color) < 1e29])
    assert 0 < small.n_lights < tame.n_lights < scene.n_lights
    prof = sb.profile(case, 96, 64, 2)
    for sc in (scene, tame, small):
        cpu_walk(oracle, sc, prof, case.name)
    g, gt, gs = pta.GpuScene(scene), pta.GpuScene(tame), pta.GpuScene(small)
    for flags in (0, pta.PT_FLAG_NO_GRIDS):
        a, b, c = (skipped(pta, x, prof, flags) for x in (g, gt, gs))
        print(f"{case.name} flags {flags}: skipped {a} (all lights), {b} (tame ones), {c} (without the 9e29 one)")
        assert a == b and b > c > 0, (tex_kind, flags, a, b, c)
    g.close(), gt.close(), gs.close()


def far_hits(oracle, scene, prof, light):
    """(shaded hits farther than 1e-3 from the light, those nearer, the smallest margin to 1e-3) of a bounces-0 frame, from
    the f32 camera rays and their first hits."""
    o = oracle.OracleScene(scene.desc, oracle.PTO_BRUTE_FORCE)
    rays = np.array([o.path_rays(prof, p, s)[0] for s in range(1, prof.samples + 1) for p in range(prof.width * prof.height)])
    recs, counts = o.trace_all(rays, 2)
    assert (counts >= 1).all()
    pos = rays[:, :3].astype(np.float64) + rays[:, 3:].astype(np.float64) * recs[:, 0]["dist"].astype(np.float64)[:, None]
    d = np.linalg.norm(pos - np.array(list(light.vec), np.float64), axis=1)
    guard = float(np.float32(1e-3))
    return int((d > guard).sum()), int((d <= guard).sum()), float(np.abs(d - guard).min())


@pytest.mark.parametrize("with_other", [False, True])
def test_a_point_light_within_1e_3_is_never_skipped(pta, oracle, with_other):
    """The other side of the skip: a point light nearer than 1e-3 to the shaded point is cast even where its BRDF term is
    exactly 0.  The light sits 5e-4 under an opaque, non-emissive floor a 2.8 mrad camera looks at: the term is 0 at every hit
    (n.l < 0) and the hits lie on both sides of 1e-3.  The casts the light adds to shadow_skipped are exactly the hits
    farther than 1e-3 - alone (the shade kernel filters a single light) and next to a second light (the shadow kernels do).
    Default and KD-tree pipelines; the megakernel casts every shadow ray."""
    case, scene = sb.guard_scene(pta, True, with_other)
    _, plain = sb.guard_scene(pta, False, with_other)
    prof = sb.profile(case, 96, 64, 2)
    want = cpu_walk(oracle, scene, prof, case.name)
    cpu_walk(oracle, plain, prof, case.name)
    far, near, margin = far_hits(oracle, scene, prof, scene.lights[-1])
    print(f"near-guard: {far} hits beyond 1e-3, {near} within, closest to it {margin:.2e}")
    assert near >= 50 and far > 10 * near and margin > 1e-7   # (f32 places a hit to 5e-8 here)
    g, gp = pta.GpuScene(scene), pta.GpuScene(plain)
    for flags in (0, pta.PT_FLAG_NO_GRIDS):
        assert_same(g.render(prof, pta.Opts.make(flags=flags)), want, (case.name, flags))
        a, b = skipped(pta, g, prof, flags), skipped(pta, gp, prof, flags)
        assert a - b == far, (with_other, flags, a, b, far, near)
    g.close(), gp.close()


# ---------------------------------------------------------------------------------------------------------------------
# live transitions
# ---------------------------------------------------------------------------------------------------------------------
# (texture kind, factor set, light set, the sheet's opacity or None for the factor set's own): opaque and translucent tables
# alternate (eight crossings), the light count goes 0 -> 5 -> 1 -> 0 -> 5 -> 4 -> 1 -> 2 -> 1 -> 0
WALK = (("none", "opaque", "none", 1.0), ("opacity", "opaque", "five", 1.0), ("none", "mirror", "point", 1.0),
        ("none", "alpha", "none", None), ("normal", "glow", "huge", 1.0), ("all", "edges", "near", None),
        ("albedo", "black", "dir_short", 1.0), ("emissive", "alpha", "point_dir", None),
        ("metalness", "opaque", "dir_long", 1.0), ("roughness", "edges", "none", 0.5))
THREE_FRAMES_AT = 4


def walk_step(pta, case, step, k):
    tex_kind, factor_set, light_set, sheet = step
    mats = sb.case_materials(case._replace(tex_kind=tex_kind, factor_set=factor_set, size_shift=k))
    if sheet is not None:
        mats[sb.MATERIALS.index("sheet")].opacity = sheet
    return mats, sb.make_lights(pta, light_set)


@pytest.mark.parametrize("geometry,from_prep", [(g, False) for g in sb.GEOMETRIES] + [("full", True)])
def test_live_walk_through_the_matrix(pta, oracle, geometry, from_prep):
    case = sb.Case("walk", geometry, "none", "none", "opaque", 3, "ACES", 0, False)
    prof = sb.profile(case, 48, 32, 2)
    mats, lights = walk_step(pta, case, WALK[-1], 0)
    first = sb.build(case, lights=lights, materials=mats)
    prep = pta.Prep(first) if from_prep else None
    g = pta.GpuScene(first, prep=prep)
    if prep is not None:
        prep.close()   # (an edited scene must not need it)
    crossings, was = 0, first.translucent
    for k, step in enumerate(WALK):
        mats, lights = walk_step(pta, case, step, k)
        edited = sb.build(case, lights=lights, materials=mats)
        want = cpu_walk(oracle, edited, prof, (geometry, k))
        g.set_materials(mats)
        g.set_lights(lights)
        crossings += edited.translucent != was
        was = edited.translucent
        fresh = pta.GpuScene(edited)
        gi, fi = g.info(), fresh.info()
        assert bool(gi.has_translucent) == bool(fi.has_translucent) == edited.translucent, (geometry, k)
        assert gi.light_grids == fi.light_grids, (geometry, k)
        for flags in FLAG_SETS:
            got = g.render(prof, pta.Opts.make(flags=flags))
            assert_same(got, fresh.render(prof, pta.Opts.make(flags=flags)), (geometry, k, flags, "fresh scene"))
            assert_same(got, want, (geometry, k, flags, "oracle"))
        if k == THREE_FRAMES_AT:   # a frame plan and the escape masks are live when the next edit arrives
            for _ in range(3):
                assert_same(g.render(prof), want, (geometry, k, "repeated frame"))
            assert g.info().frame_planned == 1
        fresh.close()
    assert crossings >= 4
    g.close()
