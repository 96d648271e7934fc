"""The geometry half of the reference renderer, restated in numpy from the Rust source alone
(src/scene/internal/triangle.rs:37-82, src/scene/internal/model.rs:26-64, src/renderer/utils.rs:11-21 and
src/renderer/hit.rs for get_dist / get_position of the two hit kinds) - a second reading, independent of
oracle/pt_oracle.cpp and of csrc/: this module imports nothing from either.

Two layers, ONE set of formulas.  Every function below takes a dtype:

  * np.float32, the VERDICT layer: every array is float32 and every numpy operation on float32 arrays is one IEEE f32
    operation, so every intermediate is rounded exactly where the f32 Rust program rounds it.  cgmath's operation order is
    spelled out once, in dot() / cross() / magnitude() below.  Oracle and kernels are held to this layer bit for bit.
  * np.float64, the GUARD layer: the same formulas on the same (f32) inputs in double precision.  It is used only to show
    that the f32 layer reads the source correctly: on well-conditioned pairs both must reach the same verdict and nearly the
    same numbers (tests/golden/geometry_model_deviation.json, tests/test_geometry_model.py).

Taken as given, not modelled:

  * The order of hits at EQUAL distance.  ray_cast sorts with a stable sort (sort_by(partial_cmp), utils.rs:19), so the
    order among equal distances is the order in which kdtree-ray's traversal yields the models and triangles; that crate is
    not available.  The project's convention is global primitive order - (model, triangle), a sphere's entry before its exit
     - and ray_cast() below concatenates in that order before it sorts.
  * kdtree-ray's slab test against the scene's bounding box (pinned by the golden white_furnace_direct).  Every ray
    set made here keeps its origins strictly inside the scene's box, where the test cannot fail; the scenes carry
    four tiny far-away triangles at corners of a box that holds every origin (BOX) and the tests assert the containment.

Set-aside cases: a pair or a ray of which some f32 intermediate THAT THE PROGRAM REACHES is non-finite, or whose hit list has
a NaN key - the Rust program panics there or its behaviour is undefined.  They are flagged (`set_aside`), counted by the tests
and not compared.  `assert!(t1 <= t2)` (model.rs:37) can only fail through a NaN; it is mapped to "no hits" and flagged.
"""
import numpy as np

F32 = np.float32
F64 = np.float64
EPSILON = F32(0.000001)     # triangle.rs:49,70 (f32 literals)
NORMAL_BIAS = F32(0.00001)  # renderer/mod.rs: a bounce ray starts at position + normal * 0.00001
BOX = 40.0                  # the corner triangles of the cast scenes: every origin lies strictly inside (-BOX, BOX)^3
HIT_DTYPE = np.dtype([("prim", "<i4"), ("flags", "<i4"), ("dist", "<f4"), ("u", "<f4"), ("v", "<f4")])
FLAG_BACKFACE, FLAG_SPHERE, FLAG_EXIT = 1, 2, 4
SET_ASIDE_CAP = 1e-3        # at most 0.1 % of any generated set (a condition on the generators, not a measurement)
MARGIN = 1e-3               # guard layer: a pair is well-conditioned when every decision it reaches is this far from its threshold
PAIR_SEED, PAIR_COUNT = 20261, 400_000
RAY_SEED, RAYS_PER_CLASS = 733, 4_000


# ---------------------------------------------------------------------------------------------------------------------
# cgmath, spelled out.  Vector3::dot is mul_element_wise().sum() = (x*x' + y*y') + z*z', left to right; Vector3::cross is
# (y z' - z y', z x' - x z', x y' - y x'); magnitude is sqrt(dot(v, v)); vector +, -, * scalar are per component.
# ---------------------------------------------------------------------------------------------------------------------
def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1],
                     a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def magnitude(a):
    return np.sqrt(dot(a, a))


def _fin3(a):
    return np.isfinite(a).all(axis=-1)


# ---------------------------------------------------------------------------------------------------------------------
# Triangle::intersect (triangle.rs:37-82)
# ---------------------------------------------------------------------------------------------------------------------
def _mt_head(o, d, v0, v1, v2):
    """triangle.rs:43-59: up to the test of u.  -> dict (r1: det passed, r2: u passed too, bad: a reached value non-finite)."""
    one = o.dtype.type(1)
    eps = o.dtype.type(EPSILON)
    v0v1 = v1 - v0
    v0v2 = v2 - v0
    pvec = cross(d, v0v2)
    det = dot(v0v1, pvec)
    r1 = ~(np.abs(det) < eps)                       # :49  if det.abs() < 0.000001 { return None }
    invdet = one / det                              # :53
    tvec = o - v0                                   # :55
    u = dot(tvec, pvec) * invdet                    # :56
    r2 = r1 & ((u >= 0) & (u <= one))               # :57  if !(0.0..=1.).contains(&u) { return None }
    bad = ~(_fin3(v0v1) & _fin3(v0v2) & _fin3(pvec) & np.isfinite(det))
    bad = bad | (r1 & ~(np.isfinite(invdet) & _fin3(tvec) & np.isfinite(u)))
    return dict(v0v1=v0v1, v0v2=v0v2, det=det, invdet=invdet, tvec=tvec, u=u, r1=r1, r2=r2, bad=bad)


def triangle(rays, tris, dtype=F32):
    """Triangle::intersect of rays [..., 6] (origin, direction) with tris [..., 3, 3], pair by pair (the leading shapes
    broadcast).  -> dict: accepted, dist, u, v (raw, as Hit::new_triangle receives them), backface (det < 0), tex_u / tex_v
    (the tex_coords of the unit-test triangle - tex_coords (0,0), (1,0), (0,1), triangle.rs:165-184 - which the
    pt_intersect_triangles hooks return: hit.rs:111-113), position (ray.origin + ray.direction * dist), det, set_aside."""
    rays, tris = np.asarray(rays, dtype), np.asarray(tris, dtype)
    zero, one, eps = dtype(0), dtype(1), dtype(EPSILON)
    o, d = rays[..., :3], rays[..., 3:]
    with np.errstate(all="ignore"):
        h = _mt_head(o, d, tris[..., 0, :], tris[..., 1, :], tris[..., 2, :])
        u, invdet, det = h["u"], h["invdet"], h["det"]
        qvec = cross(h["tvec"], h["v0v1"])              # :61
        v = dot(d, qvec) * invdet                       # :62
        upv = u + v
        r3 = h["r2"] & ~((v < zero) | (upv > one))      # :63  if v < 0. || u + v > 1. { return None }
        dist = dot(h["v0v2"], qvec) * invdet            # :67
        accepted = r3 & ~(dist < eps)                   # :70  if dist < 0.000001 { return None }   (a NaN passes)
        position = o + d * dist[..., None]              # :77
        # hit.rs:111-113 with tex_coords (0,0), (1,0), (0,1): t0 + u * (t1 - t0) + v * (t2 - t0), per component
        tex_u = (zero + u * (one - zero)) + v * (zero - zero)
        tex_v = (zero + u * (zero - zero)) + v * (one - zero)
        bad = h["bad"] | (h["r2"] & ~(_fin3(qvec) & np.isfinite(v) & np.isfinite(upv)))
        bad = bad | (r3 & ~np.isfinite(dist)) | (accepted & ~_fin3(position))
    return dict(accepted=accepted, dist=dist, u=u, v=v, upv=upv, backface=det < zero, tex_u=tex_u, tex_v=tex_v,
                position=position, det=det, r1=h["r1"], r2=h["r2"], r3=r3, set_aside=bad)


def triangle_records(res):
    """The pt_hit records the pt_intersect_triangles hooks return for triangle()'s result (miss: -1, 0, 0, 0, 0)."""
    out = np.zeros(res["accepted"].shape, HIT_DTYPE)
    a = res["accepted"]
    out["prim"] = np.where(a, 0, -1)
    out["flags"] = np.where(a & res["backface"], FLAG_BACKFACE, 0)
    for f, k in (("dist", "dist"), ("u", "tex_u"), ("v", "tex_v")):
        out[f] = np.where(a, res[k], F32(0))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# Model::intersect, the sphere arm (model.rs:26-64)
# ---------------------------------------------------------------------------------------------------------------------
def sphere(rays, center, radius, dtype=F32):
    """-> dict: count (0, 1 or 2 hits), t [..., 2] (ray parameter), dist [..., 2] (Hit::Sphere.dist = |hit_point - origin|),
    exit [..., 2] (the t2 hit: normal turned inwards), in the order of the returned Vec - the entry hit first;
    assert_failed (model.rs:37, mapped to no hits), set_aside."""
    rays, center, radius = np.asarray(rays, dtype), np.asarray(center, dtype), np.asarray(radius, dtype)
    zero, two, four = dtype(0), dtype(2), dtype(4)
    o, d = rays[..., :3], rays[..., 3:]
    with np.errstate(all="ignore"):
        ray_to_center = o - center                                      # :27
        a = dot(d, d)                                                   # :28
        b = two * dot(ray_to_center, d)                                 # :29
        c = dot(ray_to_center, ray_to_center) - radius * radius         # :30
        disc = b * b - four * a * c                                     # :31  (4.0 * a) * c
        reached = ~(disc < zero)                                        # :32
        root = np.sqrt(disc)
        t1 = (-b - root) / (two * a)                                    # :35
        t2 = (-b + root) / (two * a)                                    # :36
        assert_failed = reached & ~(t1 <= t2)                           # :37
        alive = reached & ~assert_failed & ~(t2 < zero)                 # :38
        p2 = o + d * t2[..., None]                                      # :43
        k2 = magnitude(p2 - o)                                          # :46
        both = alive & ~(t1 < zero)                                     # :50
        p1 = o + d * t1[..., None]                                      # :55
        k1 = magnitude(p1 - o)                                          # :58
        bad = ~(_fin3(ray_to_center) & np.isfinite(a) & np.isfinite(b) & np.isfinite(c) & np.isfinite(disc))
        bad = bad | (reached & ~(np.isfinite(t1) & np.isfinite(t2))) | (alive & ~np.isfinite(k2)) | (both & ~np.isfinite(k1))
    count = np.where(both, 2, np.where(alive, 1, 0))
    t = np.stack([np.where(both, t1, t2), t2], axis=-1)
    dist = np.stack([np.where(both, k1, k2), k2], axis=-1)
    exit_ = np.stack([~both, np.ones_like(both)], axis=-1)
    return dict(count=count, t=t, dist=dist, exit=exit_, assert_failed=assert_failed, set_aside=bad | assert_failed,
                disc=disc, t1=t1, t2=t2)


# ---------------------------------------------------------------------------------------------------------------------
# ray_cast (utils.rs:11-21)
# ---------------------------------------------------------------------------------------------------------------------
def flatten(models):
    """models: list of ("mesh", tris [m, 3, 3]) / ("sphere", center [3], radius), in scene order.  -> (tris [T, 3, 3],
    their global primitive ids, centers [S, 3], radii [S], their ids); a sphere counts as one primitive."""
    tris, tri_id, cen, rad, sph_id, prim = [], [], [], [], [], 0
    for m in models:
        if m[0] == "mesh":
            t = np.asarray(m[1], F32).reshape(-1, 3, 3)
            tris.append(t)
            tri_id.append(np.arange(prim, prim + len(t)))
            prim += len(t)
        else:
            cen.append(np.asarray(m[1], F32))
            rad.append(F32(m[2]))
            sph_id.append(prim)
            prim += 1
    tris = np.concatenate(tris) if tris else np.zeros((0, 3, 3), F32)
    tri_id = np.concatenate(tri_id) if tri_id else np.zeros(0, np.int64)
    return (tris, tri_id, np.array(cen, F32).reshape(-1, 3), np.array(rad, F32), np.array(sph_id, np.int64), prim)


def ray_cast(rays, models, max_hits=16, chunk=1024):
    """ray_cast of every ray: the hits of every model pushed in (model, triangle) order, a sphere's entry before its exit,
    then sorted by get_dist() with a STABLE sort (utils.rs:19).  -> (records [n, max_hits] of HIT_DTYPE in the layout of the
    trace_all hooks - u = v = 0 for spheres, unused slots -1, 0, 0, 0, 0 -, counts [n] (the whole list's length), set_aside [n])."""
    rays = np.ascontiguousarray(rays, F32).reshape(-1, 6)
    tris, tri_id, cen, rad, sph_id, _ = flatten(models)
    n = len(rays)
    out = np.zeros((n, max_hits), HIT_DTYPE)
    out["prim"] = -1
    counts = np.zeros(n, np.uint32)
    aside = np.zeros(n, bool)
    for lo in range(0, n, chunk):
        r = rays[lo:lo + chunk]
        m = len(r)
        ray_i, order, prim, flags, dist, uu, vv = [], [], [], [], [], [], []
        if len(tris):
            with np.errstate(all="ignore"):   # (the head of the test on every pair, the rest on the pairs that get there)
                h = _mt_head(r[:, None, :3], r[:, None, 3:], tris[None, :, 0], tris[None, :, 1], tris[None, :, 2])
            aside[lo:lo + m] |= h["bad"].any(axis=1)
            i, j = np.nonzero(h["r2"])
            res = triangle(r[i], tris[j])
            np.logical_or.at(aside, lo + i, res["set_aside"])
            a = res["accepted"]
            i, j = i[a], j[a]
            ray_i.append(i), order.append(tri_id[j] * 2), prim.append(tri_id[j])
            flags.append(np.where(res["backface"][a], FLAG_BACKFACE, 0)), dist.append(res["dist"][a])
            uu.append(res["u"][a]), vv.append(res["v"][a])
        if len(cen):
            s = sphere(r[:, None, :], cen[None, :, :], rad[None, :])
            aside[lo:lo + m] |= s["set_aside"].any(axis=1)
            for k in (0, 1):
                i, j = np.nonzero(s["count"] > k)
                ex = s["exit"][i, j, k]
                ray_i.append(i), order.append(sph_id[j] * 2 + ex), prim.append(sph_id[j])
                flags.append(FLAG_SPHERE | np.where(ex, FLAG_EXIT, 0)), dist.append(s["dist"][i, j, k])
                uu.append(np.zeros(len(i), F32)), vv.append(np.zeros(len(i), F32))
        ray_i, order, prim, flags = (np.concatenate(x).astype(np.int64) for x in (ray_i, order, prim, flags))
        dist, uu, vv = (np.concatenate(x).astype(F32) for x in (dist, uu, vv))
        push = np.lexsort((order, ray_i))                    # the order in which ray_cast pushes them
        ray_i, prim, flags, dist, uu, vv = (x[push] for x in (ray_i, prim, flags, dist, uu, vv))
        np.logical_or.at(aside, lo + ray_i, np.isnan(dist))  # partial_cmp().unwrap() panics
        srt = np.lexsort((dist, ray_i))                      # stable: equal distances keep the push order
        ray_i, prim, flags, dist, uu, vv = (x[srt] for x in (ray_i, prim, flags, dist, uu, vv))
        cnt = np.bincount(ray_i, minlength=m)
        counts[lo:lo + m] = cnt
        first = np.concatenate([[0], np.cumsum(cnt)[:-1]])
        slot = np.arange(len(ray_i)) - first[ray_i]
        keep = slot < max_hits
        rows, cols = lo + ray_i[keep], slot[keep]
        for f, x in (("prim", prim), ("flags", flags), ("dist", dist), ("u", uu), ("v", vv)):
            out[f][rows, cols] = x[keep]
    return out, counts, aside


# ---------------------------------------------------------------------------------------------------------------------
# The guard layer: the f32 verdicts against the same formulas in float64
# ---------------------------------------------------------------------------------------------------------------------
ROUNDING_UNIT = 2.0 ** -24    # of f32
ROUNDING_OPS = 8.0            # roundings that meet in one numerator or in det: two edge differences, a product and a difference per
#                               cross-product component, a product and two sums in the dot product, and the bound's own slack


def rounding_bounds(rays, tris):
    """A-priori bounds, from the inputs alone, on what f32 rounding can do to u, v, u + v and dist of a pair (standard forward
    error analysis: a sum of products carries at most ROUNDING_OPS * 2^-24 * the sum of the ABSOLUTE values of its products).
    A direction 1e-5 from the plane under |d| = 1e3 makes |det| = 1e-2 out of products of size 1e3: f32 keeps two digits of
    it, and no reading of the source can do better - these bounds say so without looking at any f32 result."""
    rays, tris = np.asarray(rays, F64), np.asarray(tris, F64)
    o, d = np.abs(rays[..., :3]), np.abs(rays[..., 3:])
    v0 = tris[..., 0, :]
    e1, e2 = np.abs(tris[..., 1, :] - v0), np.abs(tris[..., 2, :] - v0)
    tvec = np.abs(rays[..., :3] - v0)

    def across(a, b):   # |a x b| term by term
        return np.stack([a[..., 1] * b[..., 2] + a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] + a[..., 0] * b[..., 2],
                         a[..., 0] * b[..., 1] + a[..., 1] * b[..., 0]], axis=-1)

    k = ROUNDING_OPS * ROUNDING_UNIT
    res = triangle(rays, tris, F64)
    with np.errstate(all="ignore"):
        adet = np.abs(res["det"])
        rel_det = k * np.sum(e1 * across(d, e2), axis=-1) / adet
        eu = k * np.sum(tvec * across(d, e2), axis=-1) / adet + (rel_det + k) * np.abs(res["u"])
        ev = k * np.sum(d * across(tvec, e1), axis=-1) / adet + (rel_det + k) * np.abs(res["v"])
        ed = k * np.sum(e2 * across(tvec, e1), axis=-1) / adet + (rel_det + k) * np.abs(res["dist"])
        return dict(det=rel_det * adet, u=eu, v=ev, upv=eu + ev + k, dist=ed), res


def well_conditioned(rays, tris):
    """Pairs of which every decision the float64 evaluation REACHES is at least MARGIN from its threshold - |det| from 1e-6, u
    from 0 and 1, v from 0, u + v from 1, dist from 1e-6 - AND further from it than f32 rounding can carry the value
    (rounding_bounds: at most MARGIN for u, v and u + v, MARGIN * |dist| for dist): without the second condition the set holds pairs on which f32 and float64 differ by 0.35 in u and by
    their verdict, in the oracle exactly as here (measured on gen_pairs(): 94 of 52 370).  -> (mask, the float64 result)."""
    eps = float(EPSILON)
    b, r = rounding_bounds(rays, tris)
    with np.errstate(all="ignore"):
        far = lambda x, t, e: (np.abs(x - t) >= MARGIN) & (e <= MARGIN)
        ok = far(np.abs(r["det"]), eps, b["det"])
        ok = ok & (~r["r1"] | (far(r["u"], 0.0, b["u"]) & far(r["u"], 1.0, b["u"])))
        ok = ok & (~r["r2"] | (far(r["v"], 0.0, b["v"]) & far(r["upv"], 1.0, b["upv"])))
        ok = ok & (~r["r3"] | far(r["dist"], eps, b["dist"] / np.abs(r["dist"])))   # (dist has a scale: relative)
    return ok & ~r["set_aside"], r


def guard(rays, tris):
    """-> dict: pairs (well-conditioned ones), hits among them, verdict_mismatches, and the largest deviation of the f32
    layer from float64 on the accepted ones: dist relative, u and v absolute."""
    r32 = triangle(rays, tris, F32)
    wc, r64 = well_conditioned(rays, tris)
    wc = wc & ~r32["set_aside"]
    hit = wc & r64["accepted"]
    mism = int((wc & (r32["accepted"] != r64["accepted"])).sum())
    both = hit & r32["accepted"]
    dev = {"dist_rel": float(np.max(np.abs(r32["dist"][both].astype(F64) - r64["dist"][both]) / np.abs(r64["dist"][both]), initial=0.0)),
           "u_abs": float(np.max(np.abs(r32["u"][both].astype(F64) - r64["u"][both]), initial=0.0)),
           "v_abs": float(np.max(np.abs(r32["v"][both].astype(F64) - r64["v"][both]), initial=0.0))}
    return dict(pairs=int(wc.sum()), hits=int(hit.sum()), verdict_mismatches=mism, deviation=dev)


# ---------------------------------------------------------------------------------------------------------------------
# Generators (deterministic, seeded)
# ---------------------------------------------------------------------------------------------------------------------
def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _sphere_dirs(rng, n):
    return _unit(rng.normal(size=(n, 3)))


def _lengths(rng, n, unit_share=0.5):
    """|d|: 1 for a share of the rays, log-uniform over 1e-3 ... 1e3 for the others."""
    s = 10.0 ** rng.uniform(-3.0, 3.0, n)
    s[rng.random(n) < unit_share] = 1.0
    return s


def gen_pairs(n=PAIR_COUNT, seed=PAIR_SEED):
    """Adversarial ray / triangle pairs -> (rays [n, 6], tris [n, 3, 3]) in f32.  Triangles a few units across, 15 % needles and
    15 % tiny ones (|e1 x e2| down to 1e-7); targets in the interior, on an edge (one barycentric exactly 0) and on a vertex;
    directions generic, within 1e-8 ... 1e-4 of the triangle's plane (det around 1e-6) and axis-parallel with exact zeros;
    |d| over 1e-3 ... 1e3; start distances over 1e-7 ... 10 (dist around 1e-6), 15 % of the starts behind the target."""
    rng = np.random.default_rng(seed)
    v0 = rng.uniform(-3.0, 3.0, (n, 3))
    e1 = _sphere_dirs(rng, n) * rng.uniform(0.5, 3.0, (n, 1))
    e2 = _sphere_dirs(rng, n) * rng.uniform(0.5, 3.0, (n, 1))
    shape = rng.random(n)
    needle = shape < 0.15
    side = _unit(np.cross(e1, _sphere_dirs(rng, n)))
    e2n = e1 * rng.uniform(0.2, 1.5, (n, 1)) + side * (10.0 ** rng.uniform(-7.0, -1.0, (n, 1))) / np.linalg.norm(e1, axis=1, keepdims=True)
    e2 = np.where(needle[:, None], e2n, e2)
    tiny = (shape >= 0.15) & (shape < 0.30)
    shrink = np.where(tiny, 10.0 ** rng.uniform(-3.5, -0.5, n), 1.0)[:, None]
    tris = np.stack([v0, v0 + e1 * shrink, v0 + e2 * shrink], axis=1).astype(F32)
    t64 = tris.astype(F64)
    v0, e1, e2 = t64[:, 0], t64[:, 1] - t64[:, 0], t64[:, 2] - t64[:, 0]
    # the target point
    bu, bv = rng.random(n), rng.random(n)
    fold = bu + bv > 1.0
    bu, bv = np.where(fold, 1.0 - bu, bu), np.where(fold, 1.0 - bv, bv)
    kind = rng.random(n)
    edge, which = (kind >= 0.5) & (kind < 0.8), rng.integers(0, 3, n)
    w = rng.random(n)
    bu = np.where(edge, np.where(which == 0, 0.0, np.where(which == 1, w, w)), bu)
    bv = np.where(edge, np.where(which == 0, w, np.where(which == 1, 0.0, 1.0 - w)), bv)
    vert = kind >= 0.8
    bu = np.where(vert, (which == 1) * 1.0, bu)
    bv = np.where(vert, (which == 2) * 1.0, bv)
    p = v0 + bu[:, None] * e1 + bv[:, None] * e2
    # the direction
    normal = np.cross(e1, e2)
    nl = np.linalg.norm(normal, axis=1, keepdims=True)
    normal = np.where(nl > 0, normal / np.where(nl > 0, nl, 1.0), _sphere_dirs(rng, n))
    dk = rng.random(n)
    dirs = _sphere_dirs(rng, n)
    inplane = _unit(e1 * rng.normal(size=(n, 1)) + _unit(np.cross(normal, e1)) * rng.normal(size=(n, 1)))
    graze = _unit(inplane + normal * (10.0 ** rng.uniform(-8.0, -4.0, (n, 1))) * rng.choice([-1.0, 1.0], (n, 1)))
    dirs = np.where(((dk >= 0.5) & (dk < 0.8))[:, None], graze, dirs)
    axis = np.zeros((n, 3))
    axis[np.arange(n), rng.integers(0, 3, n)] = rng.choice([-1.0, 1.0], n)
    dirs = np.where((dk >= 0.8)[:, None], axis, dirs)
    start = 10.0 ** rng.uniform(-7.0, 1.0, n) * np.where(rng.random(n) < 0.15, -1.0, 1.0)
    o = p - dirs * start[:, None]
    d = dirs * _lengths(rng, n, 0.25)[:, None]
    return np.concatenate([o, d], axis=1).astype(F32), tris


def _pin_case(perm, scale, flip, o, d):
    """One pair of the exactly representable family: the triangle (0,0,0), (s,0,0), (0,s,0) (s a power of two; flip: the last two
    swapped - a backface) with the axes permuted, and the ray (o, d) in the same frame."""
    s = float(scale)
    tri = np.array([[0, 0, 0], [s, 0, 0], [0, s, 0]], F64)
    if flip:
        tri = tri[[0, 2, 1]]
    return np.concatenate([np.asarray(o, F64)[perm], np.asarray(d, F64)[perm]]).astype(F32), tri[:, perm].astype(F32)


def gen_threshold_pairs():
    """Each threshold of Triangle::intersect pinned from both sides: (rays [k, 6], tris [k, 3, 3], what [k]: (quantity, side)).
    A pair is constructed in float64 in a family where the f32 arithmetic is exact - an axis-aligned right triangle with
    power-of-two legs s and a ray along the third axis: det = -+ s^2 d_z, u = o_x / s, v = o_y / s, dist = -o_z / d_z - and ONE
    input is nudged by np.nextafter until the f32 model's det, dist, u, v or u + v lands exactly on the threshold, then one ulp
    below it, then one ulp above it (asserted on the model's own value).  6 thresholds x 3 axis permutations x 2 leg lengths x
    2 windings = 72 triplets."""
    rays, tris, what = [], [], []
    perms = ([0, 1, 2], [1, 2, 0], [2, 0, 1])
    for perm in perms:
        for scale in (1.0, 4.0):
            for flip in (False, True):
                s = scale
                # (quantity, threshold, the input that is nudged -> (o, d) of the pair; for the flipped triangle u and v swap)
                ux, vy = (1, 0) if flip else (0, 1)

                def pair(x, q):
                    o, d = np.array([0.25 * s, 0.25 * s, 1.0]), np.array([0.0, 0.0, -1.0])
                    if q == "det":
                        d[2] = -x / (s * s)
                    elif q == "dist":
                        o[2] = x
                    elif q == "u0":
                        o[ux] = x * s
                    elif q == "u1":
                        o[ux], o[vy] = x * s, 0.0
                    elif q == "v0":
                        o[vy] = x * s
                    elif q == "upv":
                        o[ux], o[vy] = 0.25 * s, x * s
                    return _pin_case(perm, s, flip, o, d)

                def value(x, q):
                    r, t = pair(x, q)
                    res = triangle(r, t)
                    return {"det": np.abs(res["det"]), "dist": res["dist"], "u0": res["u"], "u1": res["u"], "v0": res["v"],
                            "upv": res["upv"]}[q]

                for q, thr, x0 in (("det", EPSILON, EPSILON), ("dist", EPSILON, EPSILON), ("u0", F32(0), F32(0)), ("u1", F32(1), F32(1)),
                                   ("v0", F32(0), F32(0)), ("upv", F32(1), F32(0.75))):
                    assert value(x0, q) == thr, (q, perm, scale, flip, value(x0, q))
                    lo = hi = x0
                    for _ in range(8):    # nudge down until the model's value is one step below the threshold ...
                        lo = np.nextafter(lo, F32(-np.inf))
                        if value(lo, q) != thr:
                            break
                    for _ in range(8):    # ... and up until it is one step above
                        hi = np.nextafter(hi, F32(np.inf))
                        if value(hi, q) != thr:
                            break
                    below, above = value(lo, q), value(hi, q)
                    assert below < thr and above > thr, (q, below, above)
                    if q not in ("u0", "v0"):   # (below 0 the next value is the smallest denormal's image, not an ulp of 0)
                        assert below == np.nextafter(thr, F32(-np.inf)) and above == np.nextafter(thr, F32(np.inf)), (q, below, above)
                    for x, side in ((lo, "below"), (x0, "on"), (hi, "above")):
                        r, t = pair(x, q)
                        rays.append(r), tris.append(t), what.append((q, side))
    return np.array(rays, F32), np.array(tris, F32), what


# ---- cast scenes -----------------------------------------------------------------------------------------------------
GRID = 24          # the height field: GRID x GRID cells, two triangles each, over [-3, 3]^2


def _height(x, z):
    return 0.35 * np.sin(1.3 * x) * np.cos(0.9 * z) + 0.08 * x - 0.05 * z


def _corner_triangles():
    """Four tiny triangles at four corners of the box (-BOX, BOX)^3: they make it the scene's bounding box."""
    out = []
    for c in ((-1, -1, -1), (1, 1, 1), (-1, 1, -1), (1, -1, 1)):
        c = np.array(c, F64) * BOX
        out.append([c, c - np.sign(c) * [0.01, 0, 0], c - np.sign(c) * [0, 0.01, 0]])
    return np.array(out, F32)


def _mesh():
    xs = np.linspace(-3.0, 3.0, GRID + 1)
    x, z = np.meshgrid(xs, xs, indexing="ij")
    p = np.stack([x, _height(x, z), z], axis=-1).astype(F32)     # shared vertices: the same f32 bits in every triangle
    tris = []
    for i in range(GRID):
        for j in range(GRID):
            tris.append([p[i, j], p[i + 1, j], p[i + 1, j + 1]])
            tris.append([p[i, j], p[i + 1, j + 1], p[i, j + 1]])
    return np.array(tris, F32), p


def scene_mixed():
    """A 24 x 24 height field (two mesh models, spheres between them in model order) and 40 spheres on, through and just above
    it: two identical ones in different models, a concentric pair, one tangent to a mesh triangle, one of radius 1e-3 on a
    mesh vertex, one that encloses everything.  -> dict(models, translucent: model indices of opacity 0.5 in the translucent
    variant, tangent: (sphere's model index, the triangle it touches))."""
    rng = np.random.default_rng(41)
    tris, p = _mesh()
    half = GRID * GRID   # triangles of the first 12 rows
    spheres = [((0.0, 0.5, 0.0), 30.0),                                   # encloses everything
               ((-1.2, 0.8, 0.7), 0.3), ((-1.2, 0.8, 0.7), 0.6),          # concentric
               ((0.5, 0.6, 0.2), 0.5)]                                    # ... its twin is appended below (index 25)
    k = 2 * (10 * GRID + 13)
    t = tris[k].astype(F64)
    nrm = _unit(np.cross(t[1] - t[0], t[2] - t[0]))
    spheres.append((tuple(t.mean(axis=0) + nrm * 0.25), 0.25))            # tangent to mesh triangle k
    spheres.append((tuple(p[7, 9].astype(F64)), 1e-3))                    # tiny, centred on a mesh vertex
    while len(spheres) < 40:
        if len(spheres) == 25:
            spheres.append(spheres[3])
            continue
        x, z, r = rng.uniform(-2.8, 2.8), rng.uniform(-2.8, 2.8), rng.uniform(0.1, 0.5)
        place = len(spheres) % 3
        y = _height(x, z) + (0.0 if place == 0 else rng.uniform(-0.8, 0.8) * r if place == 1 else r + 1e-4)
        spheres.append(((x, y, z), r))
    sph = [("sphere", np.array(c, F32), F32(r)) for c, r in spheres]
    models = [("mesh", tris[:half])] + sph[:20] + [("mesh", tris[half:])] + sph[20:] + [("mesh", _corner_triangles())]
    translucent = [0, 2, 3, 4, 9, 14, 21, 23, 26, 30]   # the first mesh, the outer concentric sphere, a twin, ...
    return dict(name="mixed", models=models, translucent=translucent, tangent=(5, k))


def scene_balls():
    """1 000 spheres, no mesh but the corner triangles: leaf records that hold spheres only.  Radii log-uniform over
    1e-3 ... 1, centres uniform in [-3, 3]^3: many overlap."""
    rng = np.random.default_rng(43)
    c = rng.uniform(-3.0, 3.0, (1000, 3)).astype(F32)
    r = (10.0 ** rng.uniform(-3.0, 0.0, 1000)).astype(F32)
    models = [("sphere", c[i], r[i]) for i in range(1000)] + [("mesh", _corner_triangles())]
    return dict(name="balls", models=models, translucent=list(range(0, 1000, 7)))


def _scaled(rng, o, dirs):
    """Rays from unit directions: the first half with |d| = 1, the second with |d| log-uniform over 1e-3 ... 1e3."""
    n = len(o)
    s = np.ones(n)
    s[n // 2:] = 10.0 ** rng.uniform(-3.0, 3.0, n - n // 2)
    return np.concatenate([o, _unit(dirs) * s[:, None]], axis=1).astype(F32)


def _hemisphere(rng, normal, inward_share=0.0):
    d = _sphere_dirs(rng, len(normal))
    d = np.where((np.sum(d * normal, axis=1) < 0)[:, None], -d, d)
    return np.where((rng.random(len(d)) < inward_share)[:, None], -d, d)


def gen_rays(scene, per_class=RAYS_PER_CLASS, seed=RAY_SEED):
    """-> (rays [5 * per_class, 6] f32, start_prims [..] (the primitive a ray leaves, -1: none), classes [..]).  Classes:
    0 through points on mesh edges and vertices (a scene without a mesh: through the spheres' boxes);
    1 tangent to spheres, the impact parameter r (1 + e), e = 0 and +-1e-4;
    2 from a sphere's f32 surface point c + n r, outwards and inwards;
    3 from point + normal * 1e-5 like a bounce ray, off spheres and off mesh triangles;
    4 from inside spheres.  In every class the first half has |d| = 1, the second |d| log-uniform over 1e-3 ... 1e3."""
    rng = np.random.default_rng(seed + len(scene["models"]))
    tris, tri_id, cen, rad, sph_id, _ = flatten(scene["models"])
    real = np.abs(tris).max(axis=(1, 2)) < 0.5 * BOX if len(tris) else np.zeros(0, bool)    # not the corner triangles
    tris, tri_id = tris[real].astype(F64), tri_id[real]
    c64, r64 = cen.astype(F64), rad.astype(F64)
    n = per_class
    inner = np.nonzero(r64 < 5.0)[0]          # the spheres one can stand outside of
    out, starts = [], []

    def region(m):
        o = rng.uniform([-2.6, 0.9, -2.6], [2.6, 2.6, 2.6], (m, 3))
        o[:, 1] *= np.where(rng.random(m) < 0.3, -1.0, 1.0)
        return o

    # 0: through mesh edge / vertex points
    if len(tris):
        t, k, w = rng.integers(0, len(tris), n), rng.integers(0, 3, n), rng.random(n)
        w[rng.random(n) < 0.3] = 1.0                                      # exactly a vertex
        p = tris[t, k] * w[:, None] + tris[t, (k + 1) % 3] * (1.0 - w[:, None])
    else:
        s = rng.choice(inner, n)
        p = c64[s] + r64[s, None] * rng.uniform(-1.0, 1.0, (n, 3))
    o = region(n)
    out.append(_scaled(rng, o, p - o)), starts.append(np.full(n, -1))
    # 1: tangent to spheres
    s = rng.choice(inner, n)
    w = _sphere_dirs(rng, n)
    dist = r64[s] * rng.uniform(1.2, 6.0, n) + 0.05
    o = c64[s] - w * dist[:, None]
    side = _unit(np.cross(w, _sphere_dirs(rng, n)))
    impact = r64[s] * (1.0 + rng.choice([0.0, 1e-4, -1e-4], n))
    sin = impact / dist
    out.append(_scaled(rng, o, w * np.sqrt(1.0 - sin * sin)[:, None] + side * sin[:, None])), starts.append(np.full(n, -1))
    # 2: from the f32 surface point of a sphere, outwards (half) and inwards
    s = rng.choice(inner, n)
    nrm = _sphere_dirs(rng, n).astype(F32)
    p = (cen[s] + nrm * rad[s, None]).astype(F32)                         # f32 operations
    d = _hemisphere(rng, nrm.astype(F64))
    d[n // 4: n // 2] *= -1.0
    d[3 * n // 4:] *= -1.0
    out.append(_scaled(rng, p.astype(F64), d)), starts.append(sph_id[s])
    # 3: bounce rays: point + normal * 1e-5 (f32 operations), into the normal's hemisphere (10 %: the other one)
    use_tri = (rng.random(n) < 0.5) & (len(tris) > 0)
    s = rng.choice(inner, n)
    nrm = _sphere_dirs(rng, n)
    p = c64[s] + nrm * r64[s, None]
    prim = sph_id[s].copy()
    if len(tris):
        t = rng.integers(0, len(tris), n)
        bu, bv = rng.random(n), rng.random(n)
        fold = bu + bv > 1.0
        bu, bv = np.where(fold, 1.0 - bu, bu), np.where(fold, 1.0 - bv, bv)
        e1, e2 = tris[t, 1] - tris[t, 0], tris[t, 2] - tris[t, 0]
        tn = _unit(np.cross(e1, e2)) * rng.choice([-1.0, 1.0], (n, 1))
        p = np.where(use_tri[:, None], tris[t, 0] + bu[:, None] * e1 + bv[:, None] * e2, p)
        nrm = np.where(use_tri[:, None], tn, nrm)
        prim = np.where(use_tri, tri_id[t], prim)
    p32, n32 = p.astype(F32), nrm.astype(F32)
    o = (p32 + n32 * NORMAL_BIAS).astype(F32)
    out.append(_scaled(rng, o.astype(F64), _hemisphere(rng, nrm, 0.1))), starts.append(prim)
    # 4: from inside spheres (the enclosing one too: within 5 of its centre)
    s = rng.integers(0, len(cen), n)
    o = c64[s] + _sphere_dirs(rng, n) * (np.minimum(r64[s], 5.0) * rng.uniform(0.0, 0.99, n))[:, None]
    out.append(_scaled(rng, o, _sphere_dirs(rng, n))), starts.append(np.full(n, -1))
    rays = np.ascontiguousarray(np.concatenate(out), F32)
    return rays, np.concatenate(starts).astype(np.int64), np.repeat(np.arange(5), n)


def origins_inside_box(rays):
    return bool((np.abs(np.asarray(rays, F32)[:, :3]) < F32(BOX)).all())
