"""The temporal history (include/ptgpu.h pt_history_advance) restated without csrc/: numpy float32, one operation
per step, in the order the header writes them.

  view_constants   the constants of a camera for W x H: Python floats (f64) for the adjugate, tanf from the host libm
  advance          one frame joins a history: planes, counts, surf and the map
  plane_records    synthetic AOV pixel records: pixel-centre rays in float64 onto analytic planes
  orbit_eye, e2e_scene   the cameras and the scene of the end-to-end case
"""
import collections
import ctypes as C
import ctypes.util
import math

import numpy as np

f32 = np.float32
Params = collections.namedtuple("Params", "normal_cos plane_tol max_samples rotate")
DEFAULTS = Params(0.97, 0.01, 16, 8)          # PT_HISTORY_DEFAULT_* (test_history_model holds them to the header)
NO_SURFACE, OUTSIDE = -1, -2                 # map codes; -3 .. -6: the test the primary tap failed
View = collections.namedtuple("View", "c3 M tx ty")   # c3 [3] f32, M [3, 3] f32, tx, ty f32

_libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.tanf.restype = C.c_float
_libm.tanf.argtypes = [C.c_float]


def camera_fields(camera):
    """(16 transform floats column-major, fov) of a pta.Camera or a dict in ISF form, as float32."""
    if isinstance(camera, dict):
        return np.array([v for col in camera["transform"] for v in col], f32), f32(camera["fov"])
    return np.array(list(camera.transform), f32), f32(camera.fov)


def view_constants(camera, width, height):
    t, fov = camera_fields(camera)
    col = [[float(t[4 * k + r]) for r in range(3)] for k in range(4)]
    a = [[col[c][r] for c in range(3)] for r in range(3)]          # a[row][column], f64
    cof = [[0.0] * 3 for _ in range(3)]
    for i in range(3):
        for j in range(3):
            r0, r1, k0, k1 = (i + 1) % 3, (i + 2) % 3, (j + 1) % 3, (j + 2) % 3
            cof[i][j] = a[r0][k0] * a[r1][k1] - a[r0][k1] * a[r1][k0]
    det = a[0][0] * cof[0][0] + a[0][1] * cof[0][1] + a[0][2] * cof[0][2]
    if det == 0.0 or not math.isfinite(det):
        raise ValueError("singular camera transform")
    m = np.array([[cof[c][r] / det for c in range(3)] for r in range(3)]).astype(f32)
    ty = f32(_libm.tanf(f32(fov / f32(2.0))))
    tx = f32(ty * f32(f32(width) / f32(height)))
    return View(np.array(col[3], f32), m, tx, ty)


def empty(n):
    """The planes of a history that has seen no frame."""
    surf = np.zeros((n, 8), f32)
    return {"accum": np.zeros((n, 3), f32), "moments": np.zeros((n, 2), f32), "count": np.zeros(n, np.uint32), "surf": surf}


def _dot(ax, ay, az, bx, by, bz):
    return ((ax * bx + ay * by).astype(f32) + (az * bz).astype(f32)).astype(f32)


def surface_of(aov, samples):
    """(valid [n], surf [n, 8]) of the new view from its pixel records."""
    r = np.ascontiguousarray(aov, f32).reshape(-1, 16)
    n = len(r)
    fn = f32(samples)
    cov = r[:, 7]
    with np.errstate(all="ignore"):
        valid = (cov > 0) & ((cov + cov).astype(f32) >= fn)
        P = (r[:, 8:11] / cov[:, None]).astype(f32)
        dist = (r[:, 3] / cov).astype(f32)
        nn = _dot(r[:, 0], r[:, 1], r[:, 2], r[:, 0], r[:, 1], r[:, 2])
        inv = (f32(1.0) / np.sqrt(nn).astype(f32)).astype(f32)
        u = np.where(((nn > 0) & (nn < np.inf))[:, None], (r[:, 0:3] * inv[:, None]).astype(f32), f32(0))
    surf = np.zeros((n, 8), f32)
    surf[:, 3] = -1.0
    surf[:, 7] = np.int32(-1).view(f32)
    surf[valid, 0:3] = P[valid]
    surf[valid, 3] = dist[valid]
    surf[valid, 4:7] = u[valid]
    surf[valid, 7] = r[valid, 14]
    return valid, surf


def _tap_code(prev, q, ok, P, u, dist, params):
    """0 where tap q passes, else the code of the first test it fails (-3 .. -6); lanes that are not `ok` get -3."""
    q = np.where(ok, q, 0)
    s = prev["surf"][q]
    code = np.zeros(len(q), np.int32)
    with np.errstate(all="ignore"):
        cs = _dot(u[:, 0], u[:, 1], u[:, 2], s[:, 4], s[:, 5], s[:, 6])
        e = (s[:, 0:3] - P).astype(f32)
        along = _dot(e[:, 0], e[:, 1], e[:, 2], u[:, 0], u[:, 1], u[:, 2])
        t4 = np.abs(along) <= (f32(params.plane_tol) * dist).astype(f32)
    code = np.where(t4, code, -6)
    code = np.where(cs >= f32(params.normal_cos), code, -5)
    code = np.where(s[:, 3] >= 0, code, -4)
    code = np.where(prev["count"][q] > 0, code, -3)
    return np.where(ok, code, -3).astype(np.int32)


def advance(prev, consts_prev, consts_new, samples, frame_accum, frame_moments, aov, params, width, height):
    """The history `prev` (None: empty) seen from consts_prev takes a frame of `samples` samples rendered from consts_new.
    Returns {"accum", "moments", "count", "surf", "map", "tap"}; tap: which tap of the footprint gave the source (-1: none)."""
    n = width * height
    if prev is None:
        prev, consts_prev = empty(n), consts_new
    fa = np.ascontiguousarray(frame_accum, f32).reshape(n, 3)
    fm = np.ascontiguousarray(frame_moments, f32).reshape(n, 2)
    valid, surf = surface_of(aov, samples)
    P, dist, u = surf[:, 0:3], surf[:, 3], surf[:, 4:7]
    V = consts_prev
    M = V.M
    fw, fh = f32(width), f32(height)
    with np.errstate(all="ignore"):
        v = (P - V.c3[None, :]).astype(f32)
        qx = _dot(M[0, 0], M[0, 1], M[0, 2], v[:, 0], v[:, 1], v[:, 2])
        qy = _dot(M[1, 0], M[1, 1], M[1, 2], v[:, 0], v[:, 1], v[:, 2])
        qz = _dot(M[2, 0], M[2, 1], M[2, 2], v[:, 0], v[:, 1], v[:, 2])
        w = (-qz).astype(f32)
        front = valid & (w > 0)
        fx = ((((qx / w).astype(f32) / V.tx).astype(f32) + f32(1.0)).astype(f32) * f32(0.5)).astype(f32) * fw
        fy = ((f32(1.0) - ((qy / w).astype(f32) / V.ty).astype(f32)).astype(f32) * f32(0.5)).astype(f32) * fh
        fx, fy = fx.astype(f32), fy.astype(f32)
        inside = front & (fx >= 0) & (fx < fw) & (fy >= 0) & (fy < fh)
        fx, fy = np.where(inside, fx, f32(0)), np.where(inside, fy, f32(0))
        x0, y0 = np.floor(fx).astype(np.int64), np.floor(fy).astype(np.int64)
        sx = np.where((fx - x0.astype(f32)).astype(f32) >= f32(0.5), 1, -1)
        sy = np.where((fy - y0.astype(f32)).astype(f32) >= f32(0.5), 1, -1)
    hmap = np.full(n, NO_SURFACE, np.int32)
    hmap[valid] = OUTSIDE
    found = np.zeros(n, bool)
    tap = np.full(n, -1, np.int32)
    for k, (dx, dy) in enumerate(((0, 0), (1, 0), (0, 1), (1, 1))):
        x, y = x0 + dx * sx, y0 + dy * sy
        ok = inside & ~found & (x >= 0) & (x < width) & (y >= 0) & (y < height)
        q = x + y * width
        code = _tap_code(prev, q, ok, P, u, dist, params)
        if k == 0:
            hmap[inside] = code[inside]
        take = ok & (code == 0)
        hmap[take] = q[take]
        tap[take] = k
        found |= take
    src = np.where(found, hmap, 0)
    c = prev["count"][src].astype(np.uint32)
    A, m = prev["accum"][src].copy(), prev["moments"][src].copy()
    over = c > params.max_samples
    with np.errstate(all="ignore"):
        f = (f32(params.max_samples) / c.astype(f32)).astype(f32)
        A = np.where(over[:, None], (A * f[:, None]).astype(f32), A)
        m = np.where(over[:, None], (m * f[:, None]).astype(f32), m)
        c = np.where(over, np.uint32(params.max_samples), c)
        accum = np.where(found[:, None], (A + fa).astype(f32), fa)
        moments = np.where(found[:, None], (m + fm).astype(f32), fm)
    count = np.where(found, c + np.uint32(samples), np.uint32(samples)).astype(np.uint32)
    return {"accum": accum.astype(f32), "moments": moments.astype(f32), "count": count, "surf": surf, "map": hmap, "tap": tap}


# ---------------------------------------------------------------------------------------------------- synthetic frames
def look_at(eye, target, fov=0.9, up=(0.0, 1.0, 0.0)):
    """A rigid camera in ISF form (the construction of scene_builder.make_camera, in float64, narrowed once)."""
    eye, target, up = (np.array(v, float) for v in (eye, target, up))
    fwd = target - eye
    fwd /= np.linalg.norm(fwd)
    right = np.cross(fwd, up)
    right /= np.linalg.norm(right)
    upv = np.cross(right, fwd)
    cols = [list(right) + [0.0], list(upv) + [0.0], list(-fwd) + [0.0], list(eye) + [1.0]]
    return {"transform": [[float(f32(v)) for v in col] for col in cols], "fov": float(f32(fov)), "zfar": 100.0, "znear": 0.1}


def plane_records(camera, width, height, samples, planes):
    """[n, 16] float32 pixel records of a frame of `samples` identical samples through the pixel centres.  planes: a list of
    (point, normal, accept) - accept(P [n, 3]) -> bool [n] limits the plane's extent (None: unbounded); the primitive of plane
    k is k.  A ray takes the nearest plane in front of it; the normal faces the camera."""
    t, _ = camera_fields(camera)
    V = view_constants(camera, width, height)
    R = np.array([[float(t[4 * k + r]) for k in range(3)] for r in range(3)])
    o = np.array([float(v) for v in t[12:15]])
    ys, xs = np.divmod(np.arange(width * height), width)
    sx = ((xs + 0.5) / width * 2.0 - 1.0) * float(V.tx)
    sy = (1.0 - (ys + 0.5) / height * 2.0) * float(V.ty)
    d = np.stack([sx, sy, -np.ones_like(sx)], axis=1) @ R.T
    n = width * height
    best_t = np.full(n, np.inf)
    best_k = np.full(n, -1)
    best_n = np.zeros((n, 3))
    for k, (point, normal, accept) in enumerate(planes):
        point, normal = np.array(point, float), np.array(normal, float)
        normal /= np.linalg.norm(normal)
        with np.errstate(all="ignore"):
            tt = ((point - o) @ normal) / (d @ normal)
        hit = np.isfinite(tt) & (tt > 1e-9) & (tt < best_t)
        if accept is not None:
            hit &= accept(o + d * np.where(hit, tt, 0.0)[:, None])
        facing = np.where((d @ normal)[:, None] < 0, normal, -normal)
        best_t, best_k = np.where(hit, tt, best_t), np.where(hit, k, best_k)
        best_n = np.where(hit[:, None], facing, best_n)
    hit = best_k >= 0
    tt = np.where(hit, best_t, 0.0)
    rec = np.zeros((n, 16))
    fn = float(samples)
    rec[:, 0:3] = best_n * fn
    rec[:, 3] = tt * np.linalg.norm(d, axis=1) * fn
    rec[:, 4:7] = 0.5 * fn
    rec[:, 7] = fn
    rec[:, 8:11] = (o + d * tt[:, None]) * fn
    rec[:, 11] = 0.5 * fn
    rec[:, 15] = fn
    rec[~hit] = 0.0
    out = rec.astype(f32)
    out[:, 14] = best_k.astype(np.int32).view(f32)
    return out


def noise_planes(n, samples, seed):
    """Deterministic frame sums for the synthetic cases: (accum [n, 3], moments [n, 2]) float32."""
    rng = np.random.default_rng(seed)
    a = (rng.random((n, 3)) * samples).astype(f32)
    m = (rng.random((n, 2)) * samples).astype(f32)
    return a, m


# ---------------------------------------------------------------------------------------------------- the end-to-end case
E2E_CASE, E2E_SIZE, E2E_SAMPLES = "terrace", (24, 16), 4
ORBIT_STEP = 0.02          # radians about the vertical axis through the target, per frame


def orbit_eye(k, eye=(0.137, 1.371, 2.613), target=(0.02, 0.61, -0.52)):
    """The eye of frame k: scene_builder.make_camera's default eye turned by k * ORBIT_STEP about the target's vertical."""
    a = k * ORBIT_STEP
    dx, dz = eye[0] - target[0], eye[2] - target[2]
    return (target[0] + dx * math.cos(a) + dz * math.sin(a), eye[1], target[2] - dx * math.sin(a) + dz * math.cos(a))


def e2e_scene(pta, k):
    """(BuiltScene, camera, profile) of frame k of the end-to-end case: scene_builder's terrace under the point light."""
    import scene_builder as sb
    case = sb.Case("history-terrace", E2E_CASE, "none", "point", "opaque", 2, "FILMIC", 0, False)
    camera = sb.make_camera(pta, eye=orbit_eye(k))
    return sb.build(case, pta=pta, camera=camera), camera, sb.profile(case, E2E_SIZE[0], E2E_SIZE[1], E2E_SAMPLES, pta=pta)


def share(hmap, surf):
    """The reprojected share: surface pixels with a source over surface pixels."""
    surface = surf[:, 3] >= 0
    return float((hmap[surface] >= 0).sum()) / max(1, int(surface.sum()))
