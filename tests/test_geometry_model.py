"""Ray casts held to an independent f32 model of the geometry code (tests/geometry_model.py: Triangle::intersect, the sphere
arm of Model::intersect and ray_cast restated in numpy from the Rust source, every operation one IEEE f32 operation).

(a) The model against itself, CPU: its f32 layer against the same formulas in float64 on the well-conditioned pairs (the
    largest deviation is recorded in tests/golden/geometry_model_deviation.json, the ceiling is twice that), and against the
    reference's own 6 024 Moeller-Trumbore vectors.
(b) The model against the oracle, CPU: 400 000 adversarial ray / triangle pairs and 216 pairs that sit on, one ulp below and
    one ulp above every threshold, then the sorted hit lists of 20 000 rays in each of two scenes of 1 000 - 1 200 primitives
    (brute force and the oracle's own candidate filter) - bit for bit.
(c) The model against the device, `-m gpu`, bit for bit.  The device cast paths the model anchors:
      * isect_triangle alone                 pt_intersect_triangles on every pair;
      * the scalar walker kd_traverse        GpuScene.trace_all (whole lists and counts) and GpuScene.trace;
      * k_wf_trace                           trace_wavefront mode 0 (the near-axis rays among them: k_wf_trace_exact);
      * k_wf_trace_wide                      trace_wavefront mode 2 (every cast handed over);
      * k_wf_trace_exact                     the rays of either mode with a direction component below the walker's slack;
      * entry lists                          trace_wavefront modes 1 and 3 on the rays that leave a primitive;
      * grids via renders                    a small frame of each scene variant on the default path (camera grid, a cube-map
                                             light grid, an orthographic light grid, escape masks), asserted built;
      * the KD-tree pipeline, the megakernel the same frames with PT_FLAG_NO_GRIDS and PT_FLAG_MEGAKERNEL.
    The frames are compared with the oracle, which (b) holds to the model on the very same scenes.

Set-aside cases (a non-finite f32 intermediate, a NaN key: the Rust program panics) are counted, not compared, and capped at
0.1 % of every generated set.
"""
import ctypes as C
import json
from pathlib import Path

import numpy as np
import pytest

import geometry_model as gm
import scene_builder as sb
from conftest import GOLDEN

FIXTURE = json.loads((GOLDEN / "geometry_model_deviation.json").read_text())
SCENES = {"mixed": gm.scene_mixed, "balls": gm.scene_balls}
VARIANTS = (("mixed", False), ("mixed", True), ("balls", False))
MAX_HITS = 16
FIELDS = ("prim", "flags", "dist", "u", "v")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_records(got, ref, keep, what):
    """Every field of pt_hit records equal, the floats bit for bit, on the rows `keep`."""
    for f in FIELDS:
        g, r = got[f][keep], ref[f][keep]
        same = (g == r) if f in ("prim", "flags") else (bits(g) == bits(r))
        assert same.all(), (what, f, "first differing rows", np.argwhere(~same)[:3].tolist(), g[~same][:3], r[~same][:3])


# ---------------------------------------------------------------------------------------------------------------------
# shared inputs and the model's answers, computed once
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pairs():
    """The generated pairs with the threshold triplets appended, and the model's records for them."""
    rays, tris = gm.gen_pairs()
    t_rays, t_tris, what = gm.gen_threshold_pairs()
    rays, tris = np.concatenate([rays, t_rays]), np.concatenate([tris, t_tris])
    res = gm.triangle(rays, tris)
    return dict(rays=rays, tris=tris, res=res, records=gm.triangle_records(res), keep=~res["set_aside"], n_thresholds=len(what))


@pytest.fixture(scope="module")
def casts():
    cache = {}

    def get(name):
        if name not in cache:
            scene = SCENES[name]()
            rays, starts, classes = gm.gen_rays(scene)
            hits, counts, aside = gm.ray_cast(rays, scene["models"], MAX_HITS)
            cache[name] = dict(scene=scene, rays=rays, starts=starts, classes=classes, hits=hits, counts=counts, keep=~aside)
        return cache[name]
    return get


def built(pta, scene, translucent):
    """The pt_scene_desc of a model scene: model k has material k; flat normals; one point light and one directional light
    whose direction has length 3."""
    tris, models, mats = [], [], []
    for k, m in enumerate(scene["models"]):
        opacity = 0.5 if translucent and k in scene["translucent"] else 1.0
        albedo = (0.35 + 0.6 * ((k * 7) % 10) / 10.0, 0.35 + 0.6 * ((k * 3) % 10) / 10.0, 0.35 + 0.6 * ((k * 9) % 10) / 10.0)
        mats.append(pta.Material((C.c_float * 3)(*albedo), (C.c_float * 3)(0, 0, 0), opacity, 1.0 if k % 4 == 1 else 0.0,
                                 0.15 if k % 4 == 1 else 0.6, 1.5, -1, -1, -1, -1, -1, -1))
        if m[0] == "mesh":
            t = np.asarray(m[1], np.float64)
            n = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
            n /= np.linalg.norm(n, axis=1, keepdims=True)
            rec = np.zeros((len(t), 3, 8))
            rec[:, :, :3], rec[:, :, 3:6] = t, n[:, None, :]
            rec[:, 1, 6], rec[:, 2, 7] = 1.0, 1.0
            models.append(pta.Model(pta.PT_MODEL_MESH, k, len(tris), len(t), (C.c_float * 3)(0, 0, 0), 0.0))
            tris += list(rec.reshape(-1, 24))
        else:
            models.append(pta.Model(pta.PT_MODEL_SPHERE, k, 0, 0, (C.c_float * 3)(*[float(v) for v in m[1]]), float(m[2])))
    lights = [sb._light(pta, pta.PT_LIGHT_POINT, (1.5, 3.5, 2.0), (90.0, 85.0, 80.0)),
              sb._light(pta, pta.PT_LIGHT_DIRECTIONAL, 3.0 * sb._unit([-0.3, -0.9, -0.25]), (0.9, 1.0, 1.1))]
    eye, target = ((0.3, 2.4, 4.6), (0.0, 0.2, 0.0)) if scene["name"] == "mixed" else ((0.2, 0.6, 7.5), (0.0, 0.0, 0.0))
    return sb.BuiltScene(pta, np.array(tris, np.float32).reshape(-1, 24), models, mats, [], np.zeros(0, np.uint8), lights,
                         sb.make_camera(pta, eye, target, 0.9), (0.25, 0.3, 0.45))


# ---------------------------------------------------------------------------------------------------------------------
# (a) the model against itself
# ---------------------------------------------------------------------------------------------------------------------
def test_recorded_deviation_names_its_set_and_is_under_its_ceiling():
    """The f32 layer against float64 on the well-conditioned pairs of gen_pairs(): the same verdicts, and dist, u, v within
    twice the recorded largest deviation (the factor covers another seed's worst case and nothing else).  Conditions on the
    record itself: it names the seed and the set, and a deviation above 1e-3 - the margin that defines the set - would mean
    that the f32 layer does not compute what the float64 layer computes."""
    assert FIXTURE["seed"] == gm.PAIR_SEED and FIXTURE["pairs_generated"] == gm.PAIR_COUNT and FIXTURE["margin"] == gm.MARGIN
    assert "gen_pairs" in FIXTURE["set"]
    assert all(0 < v <= gm.MARGIN for v in FIXTURE["deviation"].values())
    for n, seed in ((gm.PAIR_COUNT, gm.PAIR_SEED), (gm.PAIR_COUNT // 4, gm.PAIR_SEED + 1)):   # the recorded set, another seed
        g = gm.guard(*gm.gen_pairs(n, seed))
        print(seed, g)
        assert g["pairs"] >= 0.1 * n and g["hits"] >= 0.075 * n      # a tenth of the pairs qualify
        assert g["verdict_mismatches"] == 0
        for k, v in g["deviation"].items():
            assert v <= 2.0 * FIXTURE["deviation"][k], (seed, k, v, FIXTURE["deviation"][k])


def test_model_passes_the_reference_vectors():
    """tests/golden/moller_trumbore.npz through the f32 layer: the 3 012 hit vectors within the reference's own 1e-5 of their
    expected dist, u, v (triangle.rs:213-216 compares tex_coords), the 3 012 miss vectors all missed."""
    mt = np.load(GOLDEN / "moller_trumbore.npz")
    hit = gm.triangle(mt["hit_rays"].astype(np.float32), mt["hit_tris"].astype(np.float32).reshape(-1, 3, 3))
    assert len(mt["hit_rays"]) == 3012 and hit["accepted"].all() and not hit["set_aside"].any()
    for k, col in (("dist", 0), ("tex_u", 1), ("tex_v", 2)):
        assert np.abs(hit[k].astype(np.float64) - mt["hit_expect"][:, col]).max() < 1e-5, k
    miss = gm.triangle(mt["miss_rays"].astype(np.float32), mt["miss_tris"].astype(np.float32).reshape(-1, 3, 3))
    assert len(mt["miss_rays"]) == 3012 and not miss["accepted"].any() and not miss["set_aside"].any()


def test_generated_sets_reach_what_they_aim_at(pairs, casts):
    """The generators' own conditions: the set-aside share under its cap, every origin strictly inside the corner box, and the
    decisions really exercised - pairs rejected at each of the four tests, hits on both sides, exact zeros, tangent rays on both
    sides of the discriminant, one-hit and two-hit spheres, tie groups in the sorted lists, lists longer than the hook's."""
    res = pairs["res"]
    assert (~pairs["keep"]).mean() <= gm.SET_ASIDE_CAP
    n = len(res["accepted"])
    stages = [(~res["r1"]).sum(), (res["r1"] & ~res["r2"]).sum(), (res["r2"] & ~res["r3"]).sum(), (res["r3"] & ~res["accepted"]).sum()]
    print("pairs", n, "accepted", int(res["accepted"].sum()), "rejected at det / u / v, u+v / dist", [int(s) for s in stages])
    assert all(s > 0.01 * n for s in stages) and res["accepted"].sum() > 0.3 * n
    assert (res["accepted"] & res["backface"]).sum() > 0.1 * n and (res["accepted"] & ~res["backface"]).sum() > 0.1 * n
    assert (res["accepted"] & (res["u"] == 0)).sum() > 100 and (res["accepted"] & (res["v"] == 0)).sum() > 100
    assert (np.abs(res["det"]) < 1e-5).sum() > 0.05 * n      # around the det threshold
    thr = slice(n - pairs["n_thresholds"], n)
    acc = res["accepted"][thr].reshape(-1, 3)                 # (below, on, above) of each triplet
    assert pairs["n_thresholds"] >= 72 and (acc[:, 1]).all() and (acc[:, 0] != acc[:, 2]).all()
    for name in SCENES:
        c = casts(name)
        assert (~c["keep"]).mean() <= gm.SET_ASIDE_CAP, name
        assert gm.origins_inside_box(c["rays"]), name
        n_prims = gm.flatten(c["scene"]["models"])[5]
        assert 1000 <= n_prims <= 2000, (name, n_prims)
        h, cnt = c["hits"], c["counts"]
        ties = (h["prim"][:, 1:] >= 0) & (bits(h["dist"][:, 1:]) == bits(h["dist"][:, :-1]))
        exits_only = (h["flags"][:, 0] & gm.FLAG_EXIT) != 0
        print(name, "prims", n_prims, "rays", len(cnt), "hits per ray", float(cnt.mean()), "rays with a tie", int(ties.any(axis=1).sum()),
              "lists over", MAX_HITS, int((cnt > MAX_HITS).sum()), "misses", int((cnt == 0).sum()))
        assert ties.any(axis=1).sum() > 50, name              # the twin spheres / shared edges / tangent rays
        assert exits_only.sum() > 1000 and (cnt > MAX_HITS).sum() > 0 and len(cnt) >= 20_000, name
        tangent = c["classes"] == 1
        first_is_sphere = (h["flags"][tangent, 0] & gm.FLAG_SPHERE) != 0
        assert 0.1 < first_is_sphere.mean() < 0.98, (name, float(first_is_sphere.mean()))   # both sides of the discriminant
    mixed = casts("mixed")["hits"]
    assert ((mixed["flags"] & gm.FLAG_SPHERE) == 0)[mixed["prim"] >= 0].sum() > 5000 and (mixed["flags"] & gm.FLAG_BACKFACE).any()


# ---------------------------------------------------------------------------------------------------------------------
# (b) the model against the oracle
# ---------------------------------------------------------------------------------------------------------------------
def test_oracle_triangles_match_the_model(oracle, pairs):
    same_records(oracle.intersect_triangles(pairs["rays"], pairs["tris"]), pairs["records"], pairs["keep"], "oracle pairs")


@pytest.mark.parametrize("mode", ["PTO_BRUTE_FORCE", "PTO_BVH"])
@pytest.mark.parametrize("name", sorted(SCENES))
def test_oracle_casts_match_the_model(pta, oracle, casts, name, mode):
    c = casts(name)
    scene = built(pta, c["scene"], False)
    hits, counts = oracle.OracleScene(scene.desc, getattr(oracle, mode)).trace_all(c["rays"], MAX_HITS)
    assert np.array_equal(counts[c["keep"]], c["counts"][c["keep"]])
    same_records(hits, c["hits"], c["keep"], (name, mode))


# ---------------------------------------------------------------------------------------------------------------------
# (c) the model against the device
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_device_triangles_match_the_model(pta, pairs):
    rays, tris = np.ascontiguousarray(pairs["rays"]), np.ascontiguousarray(pairs["tris"])
    out = np.zeros(len(rays), dtype=pta.HIT_DTYPE)
    pta.check_gpu(pta.gpu_lib().pt_intersect_triangles(0, rays.ctypes.data, tris.ctypes.data, len(rays), out.ctypes.data))
    same_records(out, pairs["records"], pairs["keep"], "device pairs")


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SCENES))
def test_device_casts_match_the_model(pta, casts, name):
    c = casts(name)
    keep, ref = c["keep"], c["hits"]
    g = pta.GpuScene(built(pta, c["scene"], False))
    assert g.info().n_kd_leaves > 16           # a real tree: the walkers' early exit runs
    hits, counts = g.trace_all(c["rays"], MAX_HITS)                      # the scalar walker, whole lists
    assert np.array_equal(counts[keep], c["counts"][keep])
    same_records(hits, ref, keep, (name, "trace_all"))
    same_records(g.trace(c["rays"]), ref[:, 0], keep, (name, "trace"))
    for mode in (0, 2):                                                  # k_wf_trace, k_wf_trace_wide, k_wf_trace_exact
        same_records(g.trace_wavefront(c["rays"], None, mode), ref[:, 0], keep, (name, "wavefront", mode))
    leaving = c["starts"] >= 0                                           # entry lists: from the primitive the ray leaves
    assert leaving.sum() >= 2 * gm.RAYS_PER_CLASS
    for mode in (1, 3):
        w = g.trace_wavefront(c["rays"][leaving], c["starts"][leaving].astype(np.uint32), mode)
        same_records(w, ref[leaving, 0], keep[leaving], (name, "wavefront", mode))
    g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name,translucent", VARIANTS)
def test_device_frames_match_the_oracle(pta, oracle, casts, name, translucent):
    """64 x 48, 4 spp, 4 bounces on the default path, the KD-tree pipeline and the megakernel: accumulation buffer and image
    equal to the oracle's bit for bit.  The camera grid, both light grids and the escape masks are built - otherwise the frame
    would test the KD path three times."""
    scene = built(pta, casts(name)["scene"], translucent)
    prof = pta.Profile.make(64, 48, 4, 4)
    o_rgb, o_acc, stats = oracle.OracleScene(scene.desc, oracle.PTO_BVH).render(prof)
    assert stats["numeric_errors"] == 0 and stats["segments"] > 1.5 * stats["samples"]
    g = pta.GpuScene(scene)
    for flags in (0, pta.PT_FLAG_NO_GRIDS, pta.PT_FLAG_MEGAKERNEL):
        rgb, acc = g.render(prof, pta.Opts.make(flags=flags))
        assert np.array_equal(bits(acc), bits(o_acc)) and np.array_equal(rgb, o_rgb), (name, translucent, flags)
    info = g.info().as_dict()
    print(name, translucent, {k: info[k] for k in ("cam_grid_res", "light_grids", "grid_refs", "escape_prims", "has_translucent")})
    assert info["cam_grid_res"] > 0 and info["light_grids"] == 2 and info["grid_refs"] > 0 and info["escape_prims"] > 0
    assert info["has_translucent"] == int(translucent)
    g.close()
