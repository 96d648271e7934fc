"""Escape masks against brute force on hostile geometry (tests/escape_scenes.py: terraces, hinges, resting objects, a skyline,
a dome, awkward normals, the reach limit, scaled and translated placements - each flat and tilted).

One statement, no case set aside:

    for every query (P, o, d) whose foot lies within delta of P:  GpuScene.escape_query says proven  =>  the brute-force
    oracle's trace_all(o, d) is empty, and so is the device's GpuScene.trace_all.

delta = 8e-6 x the diagonal of the scene's box (the lower bound of escape_delta_in, csrc/pt_gpu.hip, computed here from the
description).  escape_query runs escape_proves_miss itself - the function k_wf_shade calls - so which cell the device reads
for a direction on a border is asked, not restated; a query whose height check fails there comes back "not proven" and is
never counted as a proof.  Origins and directions are float32 before they go anywhere.

Ray sets, per masked floor primitive with clear cells: (a) interior - the generator of tests/test_escape_masks.py; (b) borders
- cube-map coordinates on k x 0.25 and 1, 2, 4 float32 steps to either side, face seams and cube corners, normalised in
float32 and not; (c) grazing - the corner of every clear cell nearest the plane from the extremes of the origin set; (d)
aimed - from those extremes at the primitives that rise above P's plane; (e) a - d under PT_ESCAPE_ALPHA 0.2 and 0.01; (f)
origins the pipeline makes: hit point + interpolated normal x 1e-5 in float32 (the foot condition replaced by that).
Every test prints its figures as `ESC-RECORD ...` lines before it asserts (profiles/r11_escape_adversarial.txt keeps them).

(f) forms the origin as k_wf_shade does (pt_wf_shade_body.h: pos + normal * 1e-5f with make_surface's interpolated normal, which
is NOT flipped on a back face - shading_normal's flip goes to the BRDF only) and, as a second variant, with the normal
flipped on a back face."""
import time

import numpy as np
import pytest

import escape_scenes as es
from test_escape_masks import H_HI, H_LO, bits, rays_through_clear_cells

pytestmark = pytest.mark.gpu

# Families in which the builder declines (nearly) every floor primitive, with the reason: set (a) need not reach 5 000 proofs there.
# At most two entries.
DECLINED = {}
F32 = np.float32
BORDER_CAP = 300000   # rows of set b per instance (the brute-force pass of a family is to stay under ~10 s)
EXTREMES = 28   # 7 feet (vertices, edge midpoints, centroid) x (as is, pushed outward by delta) x (just inside H_LO, H_HI)


def record(**kw):
    print("ESC-RECORD " + " ".join(f"{k}={v}" for k, v in kw.items()))


# ---------------------------------------------------------------------------------------------------------------------
# one instance of a family with everything the tests need, made once
# ---------------------------------------------------------------------------------------------------------------------
class Instance:
    def __init__(self, pta, oracle, family, instance):
        self.family, self.instance, self.pta = family, instance, pta
        self.scene, self.floors = es.make(pta, family, instance)
        self.P = es.primitives(self.scene)
        self.tri = self.P["tri"].astype(np.float64)
        self.n_prims = len(self.tri)
        tri_rows, sph_rows = ~self.P["is_sphere"], self.P["is_sphere"]
        lo = np.concatenate([self.P["tri"][tri_rows].reshape(-1, 3), (self.P["centre"] - self.P["radius"][:, None])[sph_rows]]).min(axis=0)
        hi = np.concatenate([self.P["tri"][tri_rows].reshape(-1, 3), (self.P["centre"] + self.P["radius"][:, None])[sph_rows]]).max(axis=0)
        self.delta = 8e-6 * float(np.linalg.norm(hi.astype(np.float64) - lo.astype(np.float64)))
        self.rounding = 2.0 * 2.0 ** -24 * float(max(np.abs(lo).max(), np.abs(hi).max()))   # of an origin's three float32 coordinates
        self.g = pta.GpuScene(self.scene)
        self.masks = self.g.escape_masks()
        self.normals, self.v0, self.blocked = self.masks
        self.has = np.abs(self.normals).sum(axis=1) > 0
        self.clear_count = (~self.blocked).reshape(self.n_prims, -1).sum(axis=1) * self.has
        self.floor = np.concatenate(list(self.floors.values()))
        self.targets = self.floor[self.clear_count[self.floor] > 0]    # masked floor primitives that have clear cells
        self.oracle = oracle.OracleScene(self.scene.desc, oracle.PTO_BRUTE_FORCE)
        self.bf_seconds = 0.0

    def with_alpha(self, alpha):
        """The same scene, its masks built under another PT_ESCAPE_ALPHA (set by the caller through monkeypatch)."""
        other = object.__new__(Instance)
        other.__dict__.update(self.__dict__)
        other.g = self.pta.GpuScene(self.scene)
        other.masks = other.g.escape_masks()
        other.normals, other.v0, other.blocked = other.masks
        other.has = np.abs(other.normals).sum(axis=1) > 0
        other.clear_count = (~other.blocked).reshape(other.n_prims, -1).sum(axis=1) * other.has
        other.targets = other.floor[other.clear_count[other.floor] > 0]
        other.bf_seconds = 0.0
        return other


_INSTANCES = {}


@pytest.fixture(scope="module")
def family_instances(pta, oracle):
    def get(family):
        if family not in _INSTANCES:
            _INSTANCES[family] = [Instance(pta, oracle, family, i) for i in es.instances(family)]
        return _INSTANCES[family]
    yield get
    _INSTANCES.clear()


# ---------------------------------------------------------------------------------------------------------------------
# geometry helpers (float64)
# ---------------------------------------------------------------------------------------------------------------------
def unit(v):
    n = np.linalg.norm(v, axis=-1, keepdims=True)
    return v / np.where(n > 0, n, 1.0)


def foot_distance(tri, n, o):
    """Distance of the foot of o (on the plane through tri[:, 0] with unit normal n) from the triangle, in the plane."""
    h = ((o - tri[:, 0]) * n).sum(axis=1)
    f = o - n * h[:, None]
    side, dist = [], []
    for k in range(3):
        a, b = tri[:, k], tri[:, (k + 1) % 3]
        ab = b - a
        side.append((np.cross(ab, f - a) * n).sum(axis=1))
        t = np.clip(((f - a) * ab).sum(axis=1) / np.maximum((ab * ab).sum(axis=1), 1e-300), 0.0, 1.0)
        dist.append(np.linalg.norm(f - (a + t[:, None] * ab), axis=1))
    side = np.stack(side)
    inside = (side >= 0).all(axis=0) | (side <= 0).all(axis=0)
    return np.where(inside, 0.0, np.min(dist, axis=0))


def cube_dirs(face, u, v):
    """Directions (un-normalised: the face's axis is +-1) of cube-map coordinates (u, v) on `face` - esc_cell's convention:
    face = 2 axis + negative, u along the next axis, v along the one after."""
    d = np.zeros((len(face), 3), np.float64)
    i, axis = np.arange(len(face)), face // 2
    d[i, axis] = np.where(face % 2 == 1, -1.0, 1.0)
    d[i, (axis + 1) % 3] = u
    d[i, (axis + 2) % 3] = v
    return d


def normalise_f32(d):
    d = d.astype(F32)
    m = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    return d / m[:, None]


def esc_cell(w):
    """esc_cell (csrc/pt_escape.h) in float32: (face, column, row) of directions w [n, 3]."""
    w = w.astype(F32)
    ax, ay, az = np.abs(w[:, 0]), np.abs(w[:, 1]), np.abs(w[:, 2])
    fx = (ax >= ay) & (ax >= az)
    fy = ~fx & (ay >= az)
    wa = np.where(fx, w[:, 0], np.where(fy, w[:, 1], w[:, 2]))
    wb = np.where(fx, w[:, 1], np.where(fy, w[:, 2], w[:, 0]))
    wc = np.where(fx, w[:, 2], np.where(fy, w[:, 0], w[:, 1]))
    inv = F32(1.0) / np.abs(wa)
    fu, fv = (wb * inv + F32(1.0)) * F32(4.0), (wc * inv + F32(1.0)) * F32(4.0)
    cu = np.where(fu >= 0, np.minimum(np.floor(fu), F32(7.0)), F32(0.0)).astype(np.int64)
    cv = np.where(fv >= 0, np.minimum(np.floor(fv), F32(7.0)), F32(0.0)).astype(np.int64)
    face = np.where(fx, 0, np.where(fy, 2, 4)) + (wa < 0)
    return face, cu, cv


def height_f32(I, prims, o):
    """The height escape_proves_miss computes: dot3(n, o - v0), every operation one float32 operation."""
    n, rel = I.normals[prims].astype(F32), o.astype(F32) - I.v0[prims].astype(F32)
    return (n[:, 0] * rel[:, 0] + n[:, 1] * rel[:, 1]) + n[:, 2] * rel[:, 2]


def extreme_origins(I, prims, which):
    """Origin number `which` (0 .. EXTREMES - 1) of the extremes of the origin set of each primitive: the three vertices, the edge
    midpoints and the centroid, as they are or pushed outward by delta in the plane, just inside H_LO or just inside H_HI."""
    t, n = I.tri[prims], I.normals[prims].astype(np.float64)
    cen = t.mean(axis=1)
    spot, pushed, high = which % 7, (which // 7) % 2, which // 14
    rows = np.arange(len(prims))
    vert = t[rows, spot % 3]
    a, b = t[rows, spot % 3], t[rows, (spot + 1) % 3]
    mid = 0.5 * (a + b)
    out_n = unit(np.cross(b - a, n))
    out_n *= np.where(((mid - cen) * out_n).sum(axis=1) < 0, -1.0, 1.0)[:, None]
    foot = np.where((spot < 3)[:, None], vert, np.where((spot < 6)[:, None], mid, cen))
    push = np.where((spot < 3)[:, None], unit(vert - cen), np.where((spot < 6)[:, None], out_n, unit(t[:, 0] - cen)))
    h = np.where(high == 1, H_HI - 3e-7, H_LO + 3e-7)
    return foot + push * (I.delta * pushed)[:, None] + n * h[:, None]


def check(I, what, prims, rays, foot_rule=True):
    """The statement on one set of queries.  Returns (queries, proofs examined, violations)."""
    rays = np.ascontiguousarray(rays, F32)
    prims = np.ascontiguousarray(prims, np.uint32)
    assert np.isfinite(rays).all() and (np.abs(rays[:, 3:]).max(axis=1) > 0).all(), what
    proven = I.g.escape_query(prims, rays)
    if foot_rule:
        # (an origin pushed outward by exactly delta and then rounded to float32 lies up to sqrt(3) / 2 ulp of the largest
        # coordinate farther out: the foot rule allows that rounding, as escape_delta_in does with its 4 eps amax)
        within = foot_distance(I.tri[prims], I.normals[prims].astype(np.float64), rays[:, :3].astype(np.float64)) <= I.delta + I.rounding
    else:
        within = np.ones(len(rays), bool)
    assert not proven[~I.has[prims]].any(), "a primitive without a mask proved something"
    sel = proven & within
    sub = rays[sel]
    t0 = time.perf_counter()
    o_hits, o_counts = I.oracle.trace_all(sub, 2)
    bf = time.perf_counter() - t0
    I.bf_seconds += bf
    d_hits, d_counts = I.g.trace_all(sub, 2)
    bad_o, bad_d = int((o_counts > 0).sum()), int((d_counts > 0).sum())
    record(family=I.family, instance=I.instance, set=what, queries=len(rays), proven=int(proven.sum()), foot_outside_delta=int((~within).sum()),
           proofs=int(sel.sum()), violations_oracle=bad_o, violations_device=bad_d, brute_force_s=f"{bf:.2f}")
    if bad_o or bad_d:
        k = np.nonzero((o_counts > 0) | (d_counts > 0))[0][:5]
        print("violations:", what, "prims", prims[sel][k].tolist(), "rays", sub[k].tolist(), "oracle hits", o_hits[k, 0].tolist(),
              "device hits", d_hits[k, 0].tolist())
    return len(rays), int(sel.sum()), bad_o + bad_d


# ---------------------------------------------------------------------------------------------------------------------
# the ray sets
# ---------------------------------------------------------------------------------------------------------------------
def set_interior(I, n, seed):
    floor_only = (np.where(np.isin(np.arange(I.n_prims), I.floor)[:, None], I.normals, 0.0), I.v0, I.blocked)
    rays, prims = rays_through_clear_cells(I.scene, floor_only, n, seed)
    if rays is None:
        return np.zeros(0, np.uint32), np.zeros((0, 6), F32)
    return prims, rays


def steps_f32(x, k):
    """x (float32 values) moved k float32 steps (k < 0: down)."""
    x = x.astype(F32)
    for _ in range(abs(k)):
        x = np.nextafter(x, F32(np.inf if k > 0 else -np.inf))
    return x


def set_borders(I, seed):
    """Every side of a clear cell beyond which lies a blocked cell or the face's edge: directions on the border (and 1, 2, 4
    float32 steps to either side of it) at the side's two ends - cell corners, on the face's edge cube corners - and its middle;
    un-normalised (the face's axis exactly 1) and normalised in float32.  Origins: one of the extremes each."""
    rng = np.random.default_rng(seed)
    clear = np.zeros((I.n_prims, 6, 8, 8), bool)   # [prim, face, row (v), column (u)]
    clear[I.targets] = ~I.blocked[I.targets].reshape(-1, 6, 8, 8)
    prims, faces, us, vs = [], [], [], []
    for axis_uv, step in ((3, -1), (3, 1), (2, -1), (2, 1)):   # the side towards lower / higher u, lower / higher v
        nb = np.ones_like(clear)   # "the neighbour across this side is blocked, or there is none on this face"
        src = [slice(None)] * 4
        dst = [slice(None)] * 4
        src[axis_uv], dst[axis_uv] = (slice(0, 7), slice(1, 8)) if step < 0 else (slice(1, 8), slice(0, 7))
        nb[tuple(dst)] = ~clear[tuple(src)]
        p, f, cv, cu = np.nonzero(clear & nb)
        along, across = (cu, cv) if axis_uv == 3 else (cv, cu)
        border = (along + (1 if step > 0 else 0)) * 0.25 - 1.0
        for k in (0, -1, 1, -2, 2, -4, 4):
            b = steps_f32(border, k).astype(np.float64)
            for frac in (0.0, 0.5, 1.0):
                other = (across + frac) * 0.25 - 1.0
                prims.append(p)
                faces.append(f)
                us.append(b if axis_uv == 3 else other)
                vs.append(other if axis_uv == 3 else b)
    if not prims:
        return np.zeros(0, np.uint32), np.zeros((0, 6), F32)
    prims, faces, us, vs = (np.concatenate(x) for x in (prims, faces, us, vs))
    raw = cube_dirs(faces, us, vs).astype(F32)
    dirs = np.concatenate([raw, normalise_f32(raw)])
    prims = np.concatenate([prims, prims])
    if len(prims) > BORDER_CAP:   # every border has 42 rows: a random subset of the rows still holds (nearly) every border
        keep = rng.choice(len(prims), BORDER_CAP, replace=False)
        prims, dirs = prims[keep], dirs[keep]
    o = extreme_origins(I, prims, rng.integers(0, EXTREMES, len(prims)))
    return prims, np.concatenate([o, dirs], axis=1).astype(F32)


def set_grazing(I, seed, per_cell=2):
    """In every clear cell the corner with the smallest d . N - exactly, and 1e-4 inside the cell - from `per_cell` of the
    extremes of the origin set, drawn per query."""
    rng = np.random.default_rng(seed)
    clear = np.zeros((I.n_prims, 6, 8, 8), bool)
    clear[I.targets] = ~I.blocked[I.targets].reshape(-1, 6, 8, 8)
    p, f, cv, cu = np.nonzero(clear)
    if len(p) == 0:
        return np.zeros(0, np.uint32), np.zeros((0, 6), F32)
    n = I.normals[p].astype(np.float64)
    best, best_dot = None, None
    for du in (0, 1):
        for dv in (0, 1):
            inset = np.stack([(cu + du) * 0.25 - 1.0, (cv + dv) * 0.25 - 1.0, np.full(len(p), (0.5 - du) * 2e-4), np.full(len(p), (0.5 - dv) * 2e-4)], axis=1)
            dn = (unit(cube_dirs(f, inset[:, 0], inset[:, 1])) * n).sum(axis=1)
            take = np.ones(len(p), bool) if best is None else dn < best_dot
            best = inset if best is None else np.where(take[:, None], inset, best)
            best_dot = dn if best_dot is None else np.where(take, dn, best_dot)
    dirs = np.concatenate([unit(cube_dirs(f, best[:, 0], best[:, 1])), unit(cube_dirs(f, best[:, 0] + best[:, 2], best[:, 1] + best[:, 3]))])
    prims = np.concatenate([p, p])
    prims, dirs = np.tile(prims, per_cell), np.tile(dirs, (per_cell, 1))
    o = extreme_origins(I, prims, rng.integers(0, EXTREMES, len(prims)))
    return prims, np.concatenate([o, dirs], axis=1).astype(F32)


def set_aimed(I, seed, nearest=200, most=120):
    """From the extremes of the origin set of P at every primitive Q that rises above P's plane (the `nearest` nearest):
    a triangle's vertices, edge midpoints and centroid (and two points between), a sphere's centre and 8 points of its
    silhouette as P's centroid sees it.  At most `most` primitives P per instance, drawn at random: the whole product is
    millions of rays per family."""
    rng = np.random.default_rng(seed)
    P = I.targets if len(I.targets) <= most else np.sort(rng.choice(I.targets, most, replace=False))
    if len(P) == 0:
        return np.zeros(0, np.uint32), np.zeros((0, 6), F32)
    n, v0 = I.normals[P].astype(np.float64), I.tri[P][:, 0]
    sph = I.P["is_sphere"]
    qc = np.where(sph[:, None], I.P["centre"].astype(np.float64), I.tri.mean(axis=1))
    # the highest point of every Q above every P's plane
    sig = np.einsum("pk,pqvk->pqv", n, I.tri[None, :, :, :] - v0[:, None, None, :]).max(axis=2)
    sig_s = np.einsum("pk,pqk->pq", n, qc[None, :, :] - v0[:, None, :]) + I.P["radius"].astype(np.float64)[None, :]
    top = np.where(sph[None, :], sig_s, sig)
    cen = I.tri[P].mean(axis=1)
    dist = np.linalg.norm(qc[None, :, :] - cen[:, None, :], axis=2)
    rises = top > 0.0
    rises[np.arange(len(P)), P] = False
    dist = np.where(rises, dist, np.inf)
    k = min(nearest, I.n_prims)
    order = np.argsort(dist, axis=1)[:, :k]
    ok = np.take_along_axis(dist, order, axis=1) < np.inf
    pi, qi = np.nonzero(ok)
    q = order[pi, qi]
    if len(q) == 0:
        return np.zeros(0, np.uint32), np.zeros((0, 6), F32)
    t = I.tri[q]
    tri_t = np.stack([t[:, 0], t[:, 1], t[:, 2], 0.5 * (t[:, 0] + t[:, 1]), 0.5 * (t[:, 1] + t[:, 2]), 0.5 * (t[:, 2] + t[:, 0]),
                      t.mean(axis=1), (4 * t[:, 0] + t[:, 1] + t[:, 2]) / 6.0, (t[:, 0] + 4 * t[:, 1] + t[:, 2]) / 6.0], axis=1)
    see = unit(qc[q] - cen[pi])
    a = unit(np.cross(see, np.where(np.abs(see[:, :1]) < 0.9, [[1.0, 0, 0]], [[0, 1.0, 0]])))
    b = np.cross(see, a)
    ph = np.arange(8) * (np.pi / 4) + 0.1
    ring = qc[q][:, None, :] + I.P["radius"][q].astype(np.float64)[:, None, None] * (np.cos(ph)[None, :, None] * a[:, None, :] + np.sin(ph)[None, :, None] * b[:, None, :])
    sph_t = np.concatenate([qc[q][:, None, :], ring], axis=1)
    target = np.where(sph[q][:, None, None], sph_t, tri_t).reshape(-1, 3)
    prims = np.repeat(P[pi], 9)
    o = extreme_origins(I, prims, rng.integers(0, EXTREMES, len(prims)))
    o32 = o.astype(F32)
    d = unit(target - o32.astype(np.float64)).astype(F32)
    aims = np.abs(d).max(axis=1) > 0   # (in a large scene the rounded origin can BE the shared vertex it aims at: no ray)
    return prims[aims], np.concatenate([o32, d], axis=1)[aims]


def run_sets(I, sets, n_interior, tag=""):
    out = {}
    for s in sets:
        if s == "a":
            prims, rays = set_interior(I, n_interior, seed=11 + I.instance)
        elif s == "b":
            prims, rays = set_borders(I, seed=21 + I.instance)
        elif s == "c":
            prims, rays = set_grazing(I, seed=31 + I.instance)
        else:
            prims, rays = set_aimed(I, seed=41 + I.instance)
            if len(rays):
                hit = I.g.trace(rays)["prim"] >= 0
                record(family=I.family, instance=I.instance, set=tag + "d", aimed_rays_that_hit_on_the_device=int(hit.sum()), of=len(rays))
        out[s] = check(I, tag + s, prims, rays)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the tests
# ---------------------------------------------------------------------------------------------------------------------
def test_the_scenes_meet_their_form(pta):
    """Every instance: at most 3 000 primitives, the background, one point and one directional light, float32 triangles 0.05 -
    0.3 across in the unscaled floor patches (escape_scenes.make asserts the primitive count)."""
    for family in es.FAMILIES:
        for i in es.instances(family):
            scene, floors = es.make(pta, family, i)
            d = scene.desc.contents
            assert scene.n_prims <= es.MAX_PRIMS and [F32(d.background[k]) for k in range(3)] == [F32(v) for v in es.BACKGROUND]
            assert sorted(l.kind for l in scene.lights) == sorted([pta.PT_LIGHT_POINT, pta.PT_LIGHT_DIRECTIONAL])
            assert floors and all(len(v) for v in floors.values())


def test_most_families_have_masks(family_instances):
    """Conditions that keep the other tests from proving nothing: in at least six of the eight families at least 20 % of the
    floor primitives have a mask with clear cells."""
    good = 0
    for family in es.FAMILIES:
        floor = masked = escape_prims = 0
        for I in family_instances(family):
            info = I.g.info()
            assert info.escape_prims == int(I.has.sum())
            floor += len(I.floor)
            masked += len(I.targets)
            escape_prims += info.escape_prims
            clear = (~I.blocked[I.has]).mean() if I.has.any() else 0.0
            record(family=family, instance=I.instance, primitives=I.n_prims, escape_prims=info.escape_prims, floor_prims=len(I.floor),
                   floor_with_clear_cells=len(I.targets), clear_fraction=f"{clear:.4f}", delta=f"{I.delta:.3e}",
                   floors_without_a_clear_cell=",".join(k for k, v in I.floors.items() if not (I.clear_count[v] > 0).any()) or "-")
        share = masked / floor
        record(family=family, share_of_floor_with_clear_cells=f"{share:.3f}", escape_prims=escape_prims)
        good += share >= 0.2
    assert good >= 6
    assert len(DECLINED) <= 2


@pytest.mark.parametrize("which", ["a", "b", "c", "d"])
@pytest.mark.parametrize("family", es.FAMILIES)
def test_proofs_hold_on_hostile_geometry(family_instances, family, which):
    """One of the sets a - d on every instance of the family; set a yields at least 5 000 proofs unless the builder declines the
    family, sets b and c yield some."""
    t0 = time.perf_counter()
    instances = family_instances(family)
    bf0 = sum(I.bf_seconds for I in instances)
    queries = proofs = bad = 0
    for I in instances:
        r = run_sets(I, which, 20000 // len(instances))[which]
        queries, proofs, bad = queries + r[0], proofs + r[1], bad + r[2]
    record(family=family, set=which, total_queries=queries, total_proofs=proofs, violations=bad,
           brute_force_seconds=f"{sum(I.bf_seconds for I in instances) - bf0:.2f}", test_seconds=f"{time.perf_counter() - t0:.2f}")
    assert bad == 0
    if which == "a":
        assert proofs >= 5000 or family in DECLINED
    elif which in "bc" and family not in DECLINED:
        assert proofs > 0


@pytest.mark.parametrize("alpha", ["0.2", "0.01"])
@pytest.mark.parametrize("family", ["skyline", "resting"])
def test_proofs_hold_under_another_alpha_stop(family_instances, monkeypatch, family, alpha):
    """Set e: the masks rebuilt with PT_ESCAPE_ALPHA = 0.2 (nodes are taken whole much earlier) and 0.01 (the walk goes
    deeper), sets a and d again."""
    monkeypatch.setenv("PT_ESCAPE_ALPHA", alpha)
    total = {s: [0, 0, 0] for s in "ad"}
    for I0 in family_instances(family):
        I = I0.with_alpha(alpha)
        record(family=family, instance=I.instance, alpha=alpha, escape_prims=int(I.has.sum()), clear_fraction=f"{(~I.blocked[I.has]).mean():.4f}",
               bits_that_differ_from_the_default_alpha=int((I.blocked != I0.blocked).sum()))
        for s, r in run_sets(I, "ad", 10000, tag=f"e{alpha}:").items():
            total[s] = [x + y for x, y in zip(total[s], r)]
    record(family=family, alpha=alpha, a=total["a"], d=total["d"])
    assert all(bad == 0 for _, _, bad in total.values()), total
    assert total["a"][1] > 0


@pytest.mark.parametrize("family", es.FAMILIES)
def test_proofs_hold_from_pipeline_origins(family_instances, family):
    """Set f: 20 000 downward rays at the structure through GpuScene.trace; from every triangle hit the origin the shade kernel
    would use - (ray_o + ray_d * dist) + normal * 1e-5 in float32, the normal the barycentric blend of the vertex normals, once as
    the kernel takes it and once flipped on a back face - and 4 directions in the hemisphere of the geometric normal on the
    origin's side.  The push can exceed delta (long, tilted normals; hits accepted slightly outside): the foot condition is
    replaced by "the pipeline's own arithmetic"."""
    instances = family_instances(family)
    bad = proofs = 0
    for I in instances:
        rng = np.random.default_rng(51 + I.instance)
        n = 20000 // len(instances)
        ft = I.tri[I.floor]
        up = unit(np.cross(ft[:, 1] - ft[:, 0], ft[:, 2] - ft[:, 0]).sum(axis=0))
        ext = np.linalg.norm(ft.reshape(-1, 3).max(axis=0) - ft.reshape(-1, 3).min(axis=0))
        tris = np.nonzero(~I.P["is_sphere"])[0]
        t = I.tri[rng.choice(tris, n)]
        w = rng.dirichlet((1.0, 1.0, 1.0), n)
        aim = (t * w[:, :, None]).sum(axis=1)
        o = aim + ext * (up * rng.uniform(0.3, 1.5, (n, 1)) + rng.uniform(-0.5, 0.5, (n, 3)))
        d = unit(aim - o)
        keep = (d * up).sum(axis=1) < 0
        rays = np.concatenate([o, d], axis=1)[keep].astype(F32)
        hits = I.g.trace(rays)
        on_tri = (hits["prim"] >= 0) & ((hits["flags"] & 2) == 0)
        rays, hits = rays[on_tri], hits[on_tri]
        prim, u, v = hits["prim"].astype(np.int64), hits["u"].astype(F32), hits["v"].astype(F32)
        pos = rays[:, :3] + rays[:, 3:] * hits["dist"].astype(F32)[:, None]
        nn = I.P["nrm"][prim]
        normal = ((F32(1.0) - u - v)[:, None] * nn[:, 0] + u[:, None] * nn[:, 1]) + v[:, None] * nn[:, 2]
        back = (hits["flags"] & 1) != 0
        assert pos.dtype == F32 and normal.dtype == F32
        variants = [pos + normal * F32(0.00001), pos + np.where(back[:, None], -normal, normal) * F32(0.00001)]
        geo = np.cross(I.tri[prim][:, 1] - I.tri[prim][:, 0], I.tri[prim][:, 2] - I.tri[prim][:, 0])
        all_prims, all_rays = [], []
        for origin in variants:
            side = np.where((geo * (origin - pos).astype(np.float64)).sum(axis=1) < 0, -1.0, 1.0)
            for _ in range(4):
                dd = unit(rng.normal(size=(len(prim), 3)))
                dd *= np.where((dd * geo).sum(axis=1) * side < 0, -1.0, 1.0)[:, None]
                all_prims.append(prim)
                all_rays.append(np.concatenate([origin, dd.astype(F32)], axis=1))
        record(family=family, instance=I.instance, set="f", cast=len(keep), downward=int(keep.sum()), triangle_hits=len(prim), back_face_hits=int(back.sum()))
        q, p, b = check(I, "f", np.concatenate(all_prims), np.concatenate(all_rays), foot_rule=False)
        proofs += p
        bad += b
    record(family=family, set="f", total_proofs=proofs, violations=bad)
    assert bad == 0
    assert proofs > 0 or family in DECLINED


@pytest.mark.parametrize("family", es.FAMILIES)
def test_declined_primitives_prove_nothing(family_instances, family):
    """A primitive whose record has the normal 0 (declined, a sphere, degenerate): every query on it returns "not proven"."""
    for I in family_instances(family):
        none = np.nonzero(~I.has)[0]
        if len(none) == 0:
            continue
        rng = np.random.default_rng(61)
        prims = np.repeat(none, 24)
        where = np.where(I.P["is_sphere"][prims][:, None], I.P["centre"][prims].astype(np.float64), I.tri[prims].mean(axis=1))
        d = unit(rng.normal(size=(len(prims), 3)))
        o = where + d * rng.choice([0.0, 5e-6, 1e-5, 1e-4, 1e-3], (len(prims), 1))
        proven = I.g.escape_query(prims, np.concatenate([o, d], axis=1).astype(F32))
        record(family=family, instance=I.instance, declined_prims=len(none), queries=len(prims), proven=int(proven.sum()))
        assert not proven.any()


@pytest.mark.parametrize("family", es.FAMILIES)
def test_the_hook_reads_the_copied_masks(family_instances, family):
    """escape_query against esc_cell restated in numpy on the bits of GpuScene.escape_masks(), combined with the height test:
    50 000 random directions at least 1e-3 from every cell border in (u, v), heights on both sides of [H_LO, H_HI]."""
    I = family_instances(family)[0]
    rng = np.random.default_rng(71)
    n = 50000
    face = rng.integers(0, 6, n)
    cu, cv = rng.integers(0, 8, n), rng.integers(0, 8, n)
    u = (cu + rng.uniform(0.004, 0.996, n)) * 0.25 - 1.0
    v = (cv + rng.uniform(0.004, 0.996, n)) * 0.25 - 1.0
    d = cube_dirs(face, u, v) * rng.uniform(0.5, 2.0, (n, 1))
    d = np.where((rng.random(n) < 0.5)[:, None], unit(d), d).astype(F32)
    tri_prims = np.nonzero(~I.P["is_sphere"])[0]
    prims = np.where(rng.random(n) < 0.8, rng.choice(I.floor, n), rng.choice(tri_prims, n))
    w = rng.dirichlet((1.0, 1.0, 1.0), n)
    foot = (I.tri[prims] * w[:, :, None]).sum(axis=1)
    h = np.where(rng.random(n) < 0.6, rng.uniform(H_LO, H_HI, n), rng.uniform(-1e-4, 2e-3, n))
    geo = unit(np.cross(I.tri[prims][:, 1] - I.tri[prims][:, 0], I.tri[prims][:, 2] - I.tri[prims][:, 0]))
    nm = np.where(I.has[prims][:, None], I.normals[prims].astype(np.float64), geo)
    o = (foot + nm * h[:, None]).astype(F32)
    f2, cu2, cv2 = esc_cell(d)
    assert np.array_equal(f2, face) and np.array_equal(cu2, cu) and np.array_equal(cv2, cv)   # (away from the borders: no doubt)
    hf = height_f32(I, prims, o)
    expect = I.has[prims] & (hf >= F32(H_LO)) & (hf <= F32(H_HI)) & ~I.blocked[prims, f2, cv2 * 8 + cu2]
    got = I.g.escape_query(prims, np.concatenate([o, d], axis=1))
    record(family=family, set="hook-vs-masks", queries=n, expected_proofs=int(expect.sum()), got=int(got.sum()), differ=int((got != expect).sum()))
    assert np.array_equal(got, expect)


@pytest.mark.parametrize("family", es.FAMILIES)
def test_frames_are_the_same_bits(pta, oracle, family_instances, monkeypatch, family):
    """A 96 x 64 frame, 4 samples, 5 bounces on the default pipeline against the brute-force oracle, a scene made with
    PT_ESCAPE=0, the KD-tree pipeline and the megakernel, bit for bit; the masks did remove casts where there are clear cells."""
    prof = pta.Profile.make(96, 64, 4, 5, "FILMIC")
    masked_casts = with_clear_cells = 0
    for I in family_instances(family):
        g = pta.GpuScene(I.scene)
        rgb, acc = g.render(prof)
        g.render(prof, pta.Opts.make(flags=pta.PT_FLAG_COUNTERS))
        c = g.counters().as_dict()
        record(family=family, instance=I.instance, frame_segments=c["segments"], masked_casts=c["masked_casts"])
        t0 = time.perf_counter()
        o_rgb, o_acc, _ = I.oracle.render(prof)
        record(family=family, instance=I.instance, oracle_frame_s=f"{time.perf_counter() - t0:.2f}")
        assert np.array_equal(bits(acc), bits(o_acc)) and np.array_equal(rgb, o_rgb), "oracle"
        with monkeypatch.context() as m:
            m.setenv("PT_ESCAPE", "0")
            g0 = pta.GpuScene(I.scene)
        assert g0.info().escape_prims == 0
        rgb0, acc0 = g0.render(prof)
        assert np.array_equal(bits(acc), bits(acc0)) and np.array_equal(rgb, rgb0), "PT_ESCAPE=0"
        for f in (pta.PT_FLAG_NO_GRIDS, pta.PT_FLAG_MEGAKERNEL):
            rgb2, acc2 = g.render(prof, pta.Opts.make(flags=f))
            assert np.array_equal(bits(acc), bits(acc2)) and np.array_equal(rgb, rgb2), f
        masked_casts += c["masked_casts"]
        with_clear_cells += len(I.targets)
    if with_clear_cells:
        assert masked_casts > 0


def test_the_cell_radius_keeps_its_rounding_margin(pta):
    """The builder fattens every cell by 2e-5 rad beyond its circumscribed circle (rho + 2e-5: the rounding of esc_cell, of rho
    itself and of the cone arithmetic).  No ray can observe that margin through a hit: the spheres of far geometry are fattened by
    slop_far >= 8e-6 x the scene's reach, 8e-6 rad or more as an angle, forty times what esc_cell rounds by - so this test pins the
    margin on the bits themselves.  A lone triangle's mask is the grazing band alone: a cell is blocked iff cos(angle(centre, N) +
    rho + 2e-5) < sin_b = 2e-3.  Per face one cell and two triangles: one whose normal puts the cell's circle 1e-5 rad INSIDE the
    margin (blocked only thanks to it), one that puts it 1e-5 rad outside (clear)."""
    limit = np.arccos(2e-3)
    for face, (cu, cv) in enumerate(((2, 5), (6, 1), (0, 3), (7, 7), (4, 4), (3, 0))):
        f = np.array([face])
        centre = unit(cube_dirs(f, np.array([cu * 0.25 - 0.875]), np.array([cv * 0.25 - 0.875])))[0]
        corners = unit(cube_dirs(np.repeat(f, 4), cu * 0.25 - 1.0 + 0.25 * np.array([0, 1, 0, 1]), cv * 0.25 - 1.0 + 0.25 * np.array([0, 0, 1, 1])))
        rho = np.arccos(np.clip(corners @ centre, -1.0, 1.0)).max()
        t = unit(np.cross(centre, (0.3, -0.5, 0.8)))
        for inside, expect_blocked in ((1e-5, True), (-1e-5, False)):
            theta = limit - 2e-5 + inside - rho    # angle(centre, N) + rho + 2e-5 = limit + inside
            scene, floors = es.lone_triangle(pta, centre * np.cos(theta) + t * np.sin(theta))
            normals, v0, blocked = pta.GpuScene(scene).escape_masks()
            assert np.abs(normals[0]).sum() > 0
            n = unit(normals[0].astype(np.float64))
            got = np.arccos(np.clip(n @ centre, -1.0, 1.0)) + rho + 2e-5 - limit    # what the float32 normal really gives
            record(test="cell-radius-margin", face=face, cell=(cu, cv), wanted=inside, real=f"{got:.3e}", blocked=bool(blocked[0, face, cv * 8 + cu]))
            assert abs(got - inside) < 3e-6    # (the set-up holds: the float32 triangle has the normal it was given)
            assert bool(blocked[0, face, cv * 8 + cu]) == expect_blocked, (face, cu, cv, inside)


def test_hook_errors_are_statuses(pta, family_instances, monkeypatch):
    """A null argument, a primitive index out of range (checked on the host before anything is launched), a scene that cannot
    have masks: PT_ERR_INVALID each; n = 0: PT_OK and nothing written."""
    I = family_instances("skyline")[0]
    lib, h = I.g.lib, I.g.handle
    rays = np.zeros((4, 6), F32)
    rays[:, 4] = 1.0
    prims = np.zeros(4, np.uint32)
    out = np.full(4, 7, np.uint8)
    args = [h, prims.ctypes.data, rays.ctypes.data, 4, out.ctypes.data]
    assert lib.pt_escape_query(*args) == pta.PT_OK and (out <= 1).all()
    for k in (0, 1, 2, 4):
        bad = list(args)
        bad[k] = None
        assert lib.pt_escape_query(*bad) == pta.PT_ERR_INVALID, k
    out[:] = 7
    prims[2] = I.n_prims
    assert lib.pt_escape_query(*args) == pta.PT_ERR_INVALID and (out == 7).all()
    prims[2] = 0xFFFFFFFF
    assert lib.pt_escape_query(*args) == pta.PT_ERR_INVALID and (out == 7).all()
    with pytest.raises(Exception):
        I.g.escape_query(prims, rays)
    prims[2] = 0
    assert lib.pt_escape_query(h, prims.ctypes.data, rays.ctypes.data, 0, out.ctypes.data) == pta.PT_OK and (out == 7).all()
    assert len(I.g.escape_query(np.zeros(0, np.uint32), np.zeros((0, 6), F32))) == 0
    monkeypatch.setenv("PT_ESCAPE", "0")
    g0 = pta.GpuScene(I.scene)
    assert lib.pt_escape_query(g0.handle, prims.ctypes.data, rays.ctypes.data, 4, out.ctypes.data) == pta.PT_ERR_INVALID
