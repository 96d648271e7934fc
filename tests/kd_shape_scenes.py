"""Scenes that drive the KD-tree walkers to the ends of their range (tests/test_kd_tree_shapes.py): a NEST of primitives that
shrink geometrically towards one corner of the scene's box - its tree is one long chain, so a ray that leaves the corner has
a pending far child at every level - and TINY scenes: one primitive, a root that is a leaf, trees around the WF_LDS_NODES
slots the walkers stage in LDS, no primitive at all.

Scenes have the form of tests/geometry_model.py (dict(name, models, ...), models: ("mesh", tris) / ("sphere", centre, radius)),
so gm.ray_cast is their brute-force reference.  Every ray set keeps its origins strictly inside the scene's box (the corner
triangles make it LO .. HI on every axis), where kdtree-ray's slab test cannot fail (geometry_model.py, "taken as given").
"""
import contextlib
import ctypes as C
import os

import numpy as np

import geometry_model as gm
import scene_builder as sb

F32, F64 = np.float32, np.float64
LO, HI = 0.0, 1073741824.0              # the scene box (the `max` nest: -HI .. -LO)
NEST_OCTAVES = 66
NEST_SPHERE_OCTAVES = 8            # the even octaves below this one hold a sphere
NEST_CLUSTERS = range(9, 66, 2)      # the octaves that hold a cluster of triangles
NEST_CLUSTER_SIZE = 3
NEST_TOP = 805306368.0                 # the largest octave's distance from the corner
NEST_HITTABLE = range(33, 42)      # the smallest octaves a ray of |d| = 1 ... 100 can still hit (e^2 |d| > 1e-6)
NEST_SEED = 97
DEEP_ENV = {"PT_KD_MAX_LEAF": "1", "PT_KD_MAX_DEPTH": "62"}
RAYS_PER_CLASS = 2048              # a multiple of 64: a block of 64 consecutive rays is one wavefront
CLASS_NAMES = ("outward", "inward", "leaving", "near-axis", "alternating")
AXIS_SLACK = 8e-4                  # a direction component below PT_SLACK_K / PT_SLACK_MAX: the cast goes to k_wf_trace_exact


@contextlib.contextmanager
def kd_env(env):
    """The builder reads its PT_KD_* variables on every pth_kd_build: set them around the creation of one scene."""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _corner_triangles(edge_at_corner):
    """Four small triangles at four corners of the box LO .. HI: they make it the scene's bounding box.  The one in the nest's
    corner is smaller than the nest's smallest element."""
    out = []
    for c in ((0, 0, 0), (1, 1, 1), (0, 1, 0), (1, 0, 1)):
        c = np.array(c, F64)
        p = LO + (HI - LO) * c
        e = 0.0025 * (HI - LO) if c.any() else edge_at_corner
        s = 1.0 - 2.0 * c
        out.append([p, p + s * [e, 0, 0], p + s * [0, e, 0]])
    return np.array(out, F64)


def _mirror(p):
    """The `max` orientation: the nest's corner stays the coordinate origin - where float32 resolves the smallest elements -
    and the box becomes -HI .. -LO."""
    return -p


def nest_scene(corner, octaves=NEST_OCTAVES, seed=NEST_SEED, scale=1.0):
    """The nest at the box's minimum (`min`: box LO .. HI) or maximum (`max`: box -HI .. -LO) corner: the two orientations
    give both values of the near-is-below bit of the entry lists and both child orders.  Octave k holds one ELEMENT about
    s_k (1, 1, 1), s_k = NEST_TOP / 2^k, inside s_k (0.7 .. 1.3) on every axis, so planes separate the octaves: the
    surface-area heuristic cuts the large, nearly empty end off a node again and again and the tree becomes one chain, about
    one level per octave, down to the corner.  A ray that leaves the corner has a pending far child at every level.
    An element is a sphere (the even octaves below NEST_SPHERE_OCTAVES), one triangle, or - octaves NEST_CLUSTERS - a cluster
    of NEST_CLUSTER_SIZE triangles: the far child the chain pushes there is a subtree of its own, so the interval a popped
    entry carries decides which of its leaves are visited.

    Why this scale: a triangle of edge e is hit only while e^2 |d| > 1e-6 (the reference's determinant threshold), which a
    box of 4096 moves 20 octaves below the top.  Spheres do not keep hits alive further down: the builder grows a sphere's
    box by about 4e-3 of the scene's extent (kd_build.cpp: spheres reported in front of their surface), which puts a small
    sphere into every leaf around it, so only the large octaves hold spheres.
    `scale` shrinks the whole scene (the escape masks are built only where a ray's reach is a few units).
    -> dict(name, models, translucent, elements: per element (kind, first primitive, geometry), s_min, corner, camera)."""
    rng = np.random.default_rng(seed)
    models, elems, prim = [], [], 0
    s_min = scale * NEST_TOP * 0.5 ** (octaves - 1)
    for k in range(octaves):
        s = scale * NEST_TOP * 0.5 ** k
        c = s * (1.0 + rng.uniform(-0.1, 0.1, 3))
        if k < NEST_SPHERE_OCTAVES and k % 2 == 0:
            if corner == "max":
                c = _mirror(c)
            models.append(("sphere", c.astype(F32), F32(0.1 * s)))
            elems.append(("sphere", prim, (c.astype(F32), F32(0.1 * s)), k))
            prim += 1
            continue
        count = NEST_CLUSTER_SIZE if k in NEST_CLUSTERS else 1
        tris = []
        for j in range(count):
            cc = c + (s * rng.uniform(-0.2, 0.2, 3) if count > 1 else 0.0)
            e = (0.08 if count > 1 else 0.125) * s
            n = gm._unit(cc + s * rng.uniform(-0.3, 0.3, 3))      # faces the corner, roughly
            a = gm._unit(np.cross(n, rng.normal(size=3)))
            b = np.cross(n, a)
            tris.append([cc - e * a - 0.6 * e * b, cc + e * a - 0.6 * e * b, cc + 1.2 * e * b])
        t = np.array(tris, F64)
        if corner == "max":
            t = _mirror(t)
        t = t.astype(F32)
        models.append(("mesh", t))
        elems.append(("mesh", prim, t, k))
        prim += count
    corners = _corner_triangles(0.05 * s_min / scale) * scale
    models.append(("mesh", (_mirror(corners) if corner == "max" else corners).astype(F32)))
    # the camera sits inside the corner and looks out along the diagonal
    eye = 0.45 * s_min * np.array([1.0, 0.8, 1.1])
    target = np.array([1.0, 0.9, 1.05])
    if corner == "max":
        eye, target = _mirror(eye), _mirror(target)
    return dict(name=f"nest-{corner}" if scale == 1.0 else f"small-nest-{corner}", models=models, translucent=list(range(0, len(elems), 3)), elements=elems, s_min=s_min,
                corner=corner, camera=(tuple(eye), tuple(target), 0.9))


def nest_rays(scene, per_class=RAYS_PER_CLASS, seed=5):
    """-> (rays [5 * per_class, 6] f32, start_prims (-1: none), classes).  Classes (CLASS_NAMES):
    0 outward     from inside the corner (nearer to it than the smallest element) at the elements, with scatter;
    1 inward      from the far half of the box at the elements;
    2 leaving     from point + normal * 1e-5 (f32 operations) on the nest's primitives, like a bounce ray, with start_prims;
    3 near-axis   from inside the corner, one direction component below AXIS_SLACK (a quarter: exactly 0), the other two
                  heading out of the corner: k_wf_trace_exact walks them;
    4 alternating an outward and an inward ray in turn: in every block of 64, lanes on both sides of the stack's LDS limit.
    Within 0 - 3 every block of 64 is of one kind.  The first half of every class has |d| = 1, the second |d| log-uniform over
    1e-3 ... 1e3 (near-axis: |d| = 1 throughout, so that the small component is below the walker's limit as it stands)."""
    rng = np.random.default_rng(seed + len(scene["models"]))
    elems, s_min, n = scene["elements"], scene["s_min"], per_class
    mirrored = scene["corner"] == "max"
    # everything below in the frame of the `min` orientation (float64); world() mirrors positions, turn() directions
    world = (lambda p: _mirror(p)) if mirrored else (lambda p: p)
    turn = (lambda d: -d) if mirrored else (lambda d: d)

    def centre_size(e):
        if e[0] == "sphere":
            c, r = e[2][0].astype(F64), float(e[2][1])
        else:
            v = e[2].astype(F64).reshape(-1, 3)
            c, r = v.mean(axis=0), 0.5 * float(np.linalg.norm(v[0] - v[2]))
        return (_mirror(c) if mirrored else c), r

    cs = [centre_size(e) for e in elems]
    cen, size = np.array([c for c, _ in cs]), np.array([r for _, r in cs])

    def aim(o, m):
        k = rng.integers(0, len(elems), m)
        return cen[k] + rng.normal(size=(m, 3)) * (0.8 * size[k])[:, None] - o

    hittable = np.array([i for i, e in enumerate(elems) if NEST_HITTABLE.start <= e[3] < NEST_HITTABLE.stop])

    def outward(m):
        """Half aimed at any element, half at the smallest ones a ray can still hit (with |d| = 3 ... 300 the determinant
        threshold lets it): their leaves are popped from the top of a tall stack."""
        o = s_min * rng.uniform(0.08, 0.6, (m, 3))
        k = np.where(np.arange(m) % 2 == 0, rng.integers(0, len(elems), m), rng.choice(hittable, m))
        d = gm._unit(cen[k] + rng.normal(size=(m, 3)) * (0.8 * size[k])[:, None] - o)
        return o, d * np.where(np.arange(m) % 2 == 0, 1.0, 10.0 ** rng.uniform(0.0, 2.0, m))[:, None]

    def inward(m):
        o = rng.uniform(0.5 * (LO + HI), HI - 0.01 * (HI - LO), (m, 3))
        o[np.arange(m), rng.integers(0, 3, m)] = rng.uniform(LO + 0.1 * (HI - LO), HI - 0.01 * (HI - LO), m)
        return o, aim(o, m)

    def scaled(o, d):
        return gm._scaled(rng, world(o), turn(d)).astype(F32)

    out, starts = [], []
    o, d = outward(n)
    out.append(np.concatenate([world(o), turn(d)], axis=1).astype(F32)), starts.append(np.full(n, -1))
    out.append(scaled(*inward(n))), starts.append(np.full(n, -1))
    # 2: leaving a primitive (world frame from the start: the geometry is the scene's own f32 values)
    k = rng.choice([i for i, e in enumerate(elems) if 0.5 * NEST_TOP * 0.5 ** e[3] > 1e-4], n)   # (the offset stays inside the box)
    p, nrm, prim = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros(n, np.int64)
    for i, e in enumerate(elems[j] for j in k):
        if e[0] == "sphere":
            nrm[i] = gm._sphere_dirs(rng, 1)[0]
            p[i] = e[2][0].astype(F64) + nrm[i] * float(e[2][1])
            prim[i] = e[1]
        else:
            t = rng.integers(0, len(e[2]))
            v = e[2][t].astype(F64)
            bu, bv = rng.random(), rng.random()
            if bu + bv > 1.0:
                bu, bv = 1.0 - bu, 1.0 - bv
            p[i] = v[0] + bu * (v[1] - v[0]) + bv * (v[2] - v[0])
            nrm[i] = gm._unit(np.cross(v[1] - v[0], v[2] - v[0])) * rng.choice([-1.0, 1.0])
            prim[i] = e[1] + t
    o = (p.astype(F32) + nrm.astype(F32) * gm.NORMAL_BIAS).astype(F32)
    out.append(gm._scaled(rng, o.astype(F64), gm._hemisphere(rng, nrm, 0.1))), starts.append(prim)
    # 3: near-axis
    o = s_min * rng.uniform(0.08, 0.6, (n, 3))
    d = gm._unit(rng.uniform(0.3, 1.0, (n, 3)))
    small = rng.uniform(-AXIS_SLACK, AXIS_SLACK, n) * 0.95
    small[rng.random(n) < 0.25] = 0.0
    d[np.arange(n), rng.integers(0, 3, n)] = small
    out.append(np.concatenate([world(o), turn(d)], axis=1).astype(F32)), starts.append(np.full(n, -1))
    # 4: alternating
    (oo, do), (oi, di) = outward(n // 2), inward(n // 2)
    o, d = np.empty((n, 3)), np.empty((n, 3))
    o[0::2], o[1::2], d[0::2], d[1::2] = oo, oi, do, gm._unit(di)
    out.append(np.concatenate([world(o), turn(d)], axis=1).astype(F32)), starts.append(np.full(n, -1))
    rays = np.ascontiguousarray(np.concatenate(out), F32)
    return rays, np.concatenate(starts).astype(np.int64), np.repeat(np.arange(5), n)


# ---------------------------------------------------------------------------------------------------------------------
# nested boxes: long entry lists
# ---------------------------------------------------------------------------------------------------------------------
DOLLS_EXTENT = 4096.0              # the scene box: -DOLLS_EXTENT .. DOLLS_EXTENT
DOLLS_COUNT = 20


def dolls_scene(count=DOLLS_COUNT, seed=11):
    """Closed boxes nested about the coordinate origin, box k of half-width s_k = 0.75 DOLLS_EXTENT / 2^k: twelve triangles,
    each face a square of half-width 0.9 s_k in its own plane.  The nest above cannot give long entry lists: prep_entry_lists
    pads a primitive's box by 2.5e-7 of the scene's largest coordinate, which leaves 22 octaves, and the builder's surface-area
    heuristic cuts several octaves off a corner nest at once - about one level per octave.  Here a plane that skips a box
    would cut that box's other four faces, so the builder peels ONE face at a time, six levels per octave, and a face of box
    k has its home node some 6 k levels down.  -> dict(name, models, translucent, n_faces, camera)."""
    rng = np.random.default_rng(seed)
    models = []
    for k in range(count):
        s = 0.75 * DOLLS_EXTENT * 0.5 ** k
        tris = []
        for axis in range(3):
            u, v = (axis + 1) % 3, (axis + 2) % 3
            for sign in (-1.0, 1.0):
                q = np.zeros((4, 3))
                q[:, axis] = sign * s * (1.0 + rng.uniform(-0.03, 0.03))
                w = 0.9 * s
                q[:, u], q[:, v] = [-w, w, w, -w], [-w, -w, w, w]
                tris += [[q[0], q[1], q[2]], [q[0], q[2], q[3]]]
        models.append(("mesh", np.array(tris, F32)))
    corners = []
    for c in ((-1, -1, -1), (1, 1, 1), (-1, 1, -1), (1, -1, 1)):
        c = np.array(c, F64) * DOLLS_EXTENT
        corners.append([c, c - np.sign(c) * [0.0025 * DOLLS_EXTENT, 0, 0], c - np.sign(c) * [0, 0.0025 * DOLLS_EXTENT, 0]])
    models.append(("mesh", np.array(corners, F32)))
    return dict(name="dolls", models=models, translucent=list(range(0, count, 3)), n_faces=12 * count,
                camera=((0.001, 0.0012, 0.0009), (1.0, 0.9, 1.05), 0.9))


def dolls_rays(scene, per_class=RAYS_PER_CLASS, seed=6):
    """-> (rays [2 * per_class, 6] f32, start_prims (-1: none)): rays that leave a face of a box, from point + normal * 1e-5
    (f32 operations) like a bounce ray, with start_prims - every face equally often, so every entry-list length is walked -
    and rays from inside the innermost box.  The first half of each class has |d| = 1, the second |d| log-uniform over
    1e-3 ... 1e3."""
    rng = np.random.default_rng(seed)
    n = per_class
    tris = np.concatenate([np.asarray(m[1], F32) for m in scene["models"][:-1]]).astype(F64)
    prim = np.arange(n) % len(tris)
    v = tris[prim]
    bu, bv = rng.random(n), rng.random(n)
    fold = bu + bv > 1.0
    bu, bv = np.where(fold, 1.0 - bu, bu), np.where(fold, 1.0 - bv, bv)
    e1, e2 = v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]
    p = v[:, 0] + bu[:, None] * e1 + bv[:, None] * e2
    nrm = gm._unit(np.cross(e1, e2)) * rng.choice([-1.0, 1.0], (n, 1))
    o = (p.astype(F32) + nrm.astype(F32) * gm.NORMAL_BIAS).astype(F32)
    leaving = gm._scaled(rng, o.astype(F64), gm._hemisphere(rng, nrm, 0.1))
    s_min = 0.75 * DOLLS_EXTENT * 0.5 ** (len(scene["models"]) - 2)
    inside = gm._scaled(rng, s_min * rng.uniform(-0.8, 0.8, (n, 3)), gm._sphere_dirs(rng, n))
    rays = np.ascontiguousarray(np.concatenate([leaving, inside]), F32)
    return rays, np.concatenate([prim, np.full(n, -1)]).astype(np.int64)


# ---------------------------------------------------------------------------------------------------------------------
# tiny scenes
# ---------------------------------------------------------------------------------------------------------------------
def scattered_scene(n_prims, seed=3, name=None):
    """n_prims primitives scattered in 0 .. 4 on every axis, spheres and single triangles in turn, and NO corner triangles: the
    primitives' own bounds are the scene's box (generic_rays keeps its origins inside them)."""
    rng = np.random.default_rng(seed)
    models = []
    for k in range(n_prims):
        c = rng.uniform(0.6, 3.4, 3)
        if k % 2 == 1:
            models.append(("sphere", c.astype(F32), F32(rng.uniform(0.05, 0.3))))
        else:
            models.append(("mesh", (c + rng.uniform(-0.4, 0.4, (1, 3, 3))).astype(F32)))
    eye, target = (2.0, 2.2, 7.0), (2.0, 2.0, 2.0)
    return dict(name=name or f"scattered-{n_prims}", models=models, translucent=list(range(0, n_prims, 3)),
                camera=(eye, target, 0.7))


def scene_bounds(scene):
    tris, _, cen, rad, _, _ = gm.flatten(scene["models"])
    lo = np.concatenate([tris.reshape(-1, 3), cen - rad[:, None]]).min(axis=0)
    hi = np.concatenate([tris.reshape(-1, 3), cen + rad[:, None]]).max(axis=0)
    return lo.astype(F64), hi.astype(F64)


def generic_rays(scene, n, seed=9):
    """Rays for a tiny scene: origins strictly inside the scene's box, half aimed at its primitives, half anywhere; the
    first half of each with |d| = 1, the second |d| log-uniform over 1e-3 ... 1e3.  A scene without primitives: origins in
    the unit box."""
    rng = np.random.default_rng(seed)
    if not scene["models"]:
        o = rng.uniform(0.0, 1.0, (n, 3))
        return gm._scaled(rng, o, gm._sphere_dirs(rng, n))
    lo, hi = scene_bounds(scene)
    o = lo + (hi - lo) * rng.uniform(0.02, 0.98, (n, 3))
    tris, _, cen, rad, _, _ = gm.flatten(scene["models"])
    pts = np.concatenate([tris.astype(F64).mean(axis=1).reshape(-1, 3), cen.astype(F64)])
    ext = np.concatenate([0.5 * np.ptp(tris.astype(F64), axis=1).max(axis=1) if len(tris) else np.zeros(0), rad.astype(F64)])
    k = rng.integers(0, len(pts), n)
    d = pts[k] + rng.normal(size=(n, 3)) * ext[k, None] - o
    anywhere = rng.random(n) < 0.5
    d[anywhere] = gm._sphere_dirs(rng, int(anywhere.sum()))
    return gm._scaled(rng, o, d)


def tiny_scenes(node_counts):
    """The fixed tiny scenes, then the scattered scenes whose primitive counts `node_counts` ({label: (n_prims, seed)}, searched with
    pth_kd_build by the tests) give trees just below, at and just above WF_LDS_NODES slots."""
    one_tri = dict(name="one-triangle", models=[("mesh", np.array([[[1.0, 1.0, 2.0], [3.0, 1.2, 2.1], [1.5, 3.0, 1.8]]], F32))],
                   translucent=[], camera=((2.0, 2.0, 6.0), (2.0, 2.0, 2.0), 0.7))
    one_sph = dict(name="one-sphere", models=[("sphere", np.array([2.0, 2.0, 2.0], F32), F32(0.8))], translucent=[],
                   camera=((2.0, 2.2, 6.0), (2.0, 2.0, 2.0), 0.7))
    empty = dict(name="empty", models=[], translucent=[], camera=((2.0, 2.0, 6.0), (2.0, 2.0, 2.0), 0.7))
    max_leaf = _max_leaf()
    out = [one_tri, one_sph, scattered_scene(max_leaf, name="root-is-a-leaf"),
           scattered_scene(max_leaf + 1, name="max-leaf-plus-one"), empty]
    out += [scattered_scene(n, seed, name=f"slots-{label}") for label, (n, seed) in node_counts.items()]
    return out


def _max_leaf():
    import kd_walk_model as kw
    return kw.PT_KD_MAX_LEAF


# ---------------------------------------------------------------------------------------------------------------------
# the pt_scene_desc
# ---------------------------------------------------------------------------------------------------------------------
def built(pta, scene, translucent=False):
    """As tests/test_geometry_model.py built(): model k has material k, flat normals, one point light and one directional
    light; the camera is the scene's own."""
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
    if not mats:   # (a material table is never empty)
        mats.append(pta.Material((C.c_float * 3)(0.5, 0.5, 0.5), (C.c_float * 3)(0, 0, 0), 1.0, 0.0, 0.6, 1.5, -1, -1, -1, -1, -1, -1))
    lights = [sb._light(pta, pta.PT_LIGHT_POINT, (1.5, 3.5, 2.0), (90.0, 85.0, 80.0)),
              sb._light(pta, pta.PT_LIGHT_DIRECTIONAL, 3.0 * sb._unit([-0.3, -0.9, -0.25]), (0.9, 1.0, 1.1))]
    eye, target, fov = scene["camera"]
    return sb.BuiltScene(pta, np.array(tris, np.float32).reshape(-1, 24), models, mats, [], np.zeros(0, np.uint8), lights,
                         sb.make_camera(pta, eye, target, fov), (0.25, 0.3, 0.45))
