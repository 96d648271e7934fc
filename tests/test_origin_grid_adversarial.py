"""Origin grids (host/og_raster.h, csrc/pt_grid_build.h, csrc/pt_grid.h) against brute force on hostile geometry: the families of
tests/escape_scenes.py, flat, tilted and placed, and the `specks` of tests/grid_scenes.py.  A grid is a candidate filter: it must
never list too little and never store a distance bound that is too large.  Two statements, no case set aside:

  A, lists.  For every hit in the brute-force sorted list of a ray that a walk may need, the primitive is in the looked-up cell or
     the global block, and its stored bound is at most the hit's distance from the grid's origin (orthographic grid: its key is
     at most minus the depth of the ray's origin).  Every cell's list ascends.
  B, walks.  tests/grid_walk_model.py restates og_next_hit and og_blocker on the lists; `closest` returns the oracle's first hit
     (primitive, entry / exit, distance bits), `blocked_*` says whether the oracle's list holds a hit that passes the reference's
     test.

Grid origins per scene: the camera (with the parameters pt_scene_create derives), the point light, a point 1e-2, 1e-4 and 1e-6 x the
scene's extent above the interior of a floor triangle, a point on a vertex; where the builder answers with a disabled grid, that
is a valid answer and only that it says so is asserted.  Ray sets (float32 before they go anywhere):
  a  aimed    at vertices, at edge points 0.5 and 0.01 along an edge and the same pushed outward by 0, +-1e-7, 1e-6, 1e-5, 1e-4 x the
              triangle's size, at sphere silhouettes at 1, 1 - 1e-7 ... 1 - 1e-3, 0.9 and 0 of the tangent cone;
  b  discs    dense over every speck (specks only; 240 rays per speck from the camera, 120 from the light);
  c  borders  cube-map coordinates on cell borders and 1, 2, 4 float32 steps to either side, face seams and cube corners,
              normalised in float32 and not (the camera grid admits directions up to sqrt 3 x 1.001);
  d  shadow   rays as the pipeline makes them from the first hits of a and b: origin = pos + n x 1e-5f with |n| in [0.2, 1.5], towards
              the point light (cell looked up with pos - light, as og_light_radiance does) and along -direction of the scene's
              directional light and of two axis-aligned ones.  A point-light hit is needed only if it passes the reference's own
              range test (mod.rs:319-321); "within ldist of the light" is not the same thing.
Rays whose list is longer than K = 32 hits are set aside from B (at most 0.1 % of a set; trace_all drops a NaN key and the oracle's
numeric-error count is not per ray, so those are all that can be set aside here).  Rows are capped per set (CAPS) and the
truncation is recorded.  Every test prints `OG-RECORD key=value ...` lines before it asserts
(profiles/r17_origin_grid_adversarial.txt keeps them)."""
import hashlib
import json

import numpy as np
import pytest

import escape_scenes as es
import grid_scenes as gs
import grid_walk_model as wm
from conftest import GOLDEN
from test_origin_grid import _host_twin, camera_origin

F32 = np.float32
K = 32
CAPS = dict(aimed=9000, aimed_extra=2500, discs=21000, discs_camera=42000, borders=4000, borders_extra=1500, shadow=4000)
SET_ASIDE_CAP = 1e-3
CASES = [(f, i) for f in es.FAMILIES for i in es.instances(f)] + [("specks", i) for i in gs.INSTANCES]
IDS = [f"{f}-{i}" for f, i in CASES]
AXIS_LIGHTS = ((0.0, -1.0, 0.0), (2.0, 0.0, 0.0))   # directional lights along an axis (the second not of unit length)

# Floors against vacuity, per family and set: half of what the first CPU run counted in the family's smallest instance.
MIN_CHECKED = {   # family: {set: (hits checked by A, rays with a hit in B)}
    "terraces": {
        "camera/aimed": (5111, 3933), "camera/borders": (1442, 1441), "light/aimed": (4969, 3895), "light/borders": (1441, 1394),
        "above0.01/aimed": (1442, 1068), "above0.01/borders": (629, 579), "above0.0001/aimed": (1476, 1024),
        "above0.0001/borders": (293, 268), "above1e-06/aimed": (309, 205), "above1e-06/borders": (146, 128),
        "vertex/aimed": (224, 180), "vertex/borders": (37, 36), "light_twin/shadow": (842, 838), "ortho0/shadow": (583, 579),
        "ortho1/shadow": (833, 825), "ortho2/shadow": (0, 0),
    },
    "hinges": {
        "camera/aimed": (5052, 3868), "camera/borders": (1344, 1344), "light/aimed": (4736, 3801), "light/borders": (1413, 1364),
        "above0.01/aimed": (1385, 1027), "above0.01/borders": (558, 520), "above0.0001/aimed": (1714, 1075),
        "above0.0001/borders": (503, 388), "above1e-06/aimed": (1094, 784), "above1e-06/borders": (536, 430),
        "vertex/aimed": (1034, 755), "vertex/borders": (325, 263), "light_twin/shadow": (837, 836), "ortho0/shadow": (569, 568),
        "ortho1/shadow": (826, 818), "ortho2/shadow": (771, 746),
    },
    "resting": {
        "camera/aimed": (8542, 4185), "camera/borders": (2354, 1474), "light/aimed": (6964, 4097), "light/borders": (1923, 1461),
        "above0.01/aimed": (1782, 1120), "above0.01/borders": (613, 509), "above0.0001/aimed": (1731, 1078),
        "above0.0001/borders": (351, 281), "above1e-06/aimed": (479, 220), "above1e-06/borders": (189, 132),
        "vertex/aimed": (447, 184), "vertex/borders": (119, 53), "light_twin/shadow": (1017, 937), "ortho0/shadow": (822, 737),
        "ortho1/shadow": (998, 912), "ortho2/shadow": (523, 402),
    },
    "skyline": {
        "camera/aimed": (5800, 3881), "camera/borders": (1276, 1127), "light/aimed": (5029, 3707), "light/borders": (1083, 1047),
        "above0.01/aimed": (1377, 1020), "above0.01/borders": (394, 384), "above0.0001/aimed": (1457, 1014),
        "above0.0001/borders": (473, 428), "above1e-06/aimed": (1566, 1069), "above1e-06/borders": (320, 279),
        "vertex/aimed": (614, 377), "vertex/borders": (93, 62), "light_twin/shadow": (842, 823), "ortho0/shadow": (649, 623),
        "ortho1/shadow": (529, 522), "ortho2/shadow": (890, 538),
    },
    "dome": {
        "camera/aimed": (10424, 4331), "camera/borders": (3172, 1497), "light/aimed": (13179, 4463),
        "light/borders": (4192, 1543), "above0.01/aimed": (2541, 1185), "above0.01/borders": (1093, 615),
        "above0.0001/aimed": (2662, 1186), "above0.0001/borders": (976, 551), "vertex/aimed": (1959, 957),
        "vertex/borders": (771, 416), "light_twin/shadow": (3018, 1939), "ortho0/shadow": (1334, 1088),
        "ortho1/shadow": (1878, 1327), "ortho2/shadow": (1638, 1202),
    },
    "normals": {
        "camera/aimed": (5649, 4043), "camera/borders": (1539, 1436), "light/aimed": (5386, 4045), "light/borders": (1532, 1410),
        "above0.01/aimed": (1444, 1068), "above0.01/borders": (602, 585), "above0.0001/aimed": (1468, 1044),
        "above0.0001/borders": (284, 259), "above1e-06/aimed": (6, 6), "above1e-06/borders": (106, 106), "vertex/aimed": (0, 0),
        "vertex/borders": (0, 0), "light_twin/shadow": (922, 855), "ortho0/shadow": (618, 573), "ortho1/shadow": (910, 836),
        "ortho2/shadow": (0, 0),
    },
    "reach": {
        "camera/aimed": (5214, 3975), "camera/borders": (1415, 1404), "light/aimed": (4991, 3914), "light/borders": (1467, 1378),
        "above0.01/aimed": (1433, 1097), "above0.01/borders": (537, 533), "above0.0001/aimed": (1503, 1067),
        "above0.0001/borders": (336, 314), "above1e-06/aimed": (1033, 718), "above1e-06/borders": (267, 249),
        "vertex/aimed": (58, 33), "vertex/borders": (2, 1), "light_twin/shadow": (833, 829), "ortho0/shadow": (600, 581),
        "ortho1/shadow": (823, 814), "ortho2/shadow": (98, 35),
    },
    "placed": {
        "camera/aimed": (4926, 3722), "camera/borders": (1252, 1090), "light/aimed": (4179, 3364), "light/borders": (1060, 1012),
        "above0.01/aimed": (3, 2), "above0.01/borders": (49, 49), "above0.0001/aimed": (0, 0), "above0.0001/borders": (77, 77),
        "above1e-06/aimed": (0, 0), "above1e-06/borders": (0, 0), "vertex/aimed": (0, 0), "vertex/borders": (0, 0),
        "light_twin/shadow": (285, 243), "ortho0/shadow": (336, 269), "ortho1/shadow": (0, 0), "ortho2/shadow": (0, 0),
    },
    "specks": {
        "camera/aimed": (10772, 4393), "camera/discs": (58157, 21000), "camera/borders": (2103, 1483),
        "light/aimed": (10802, 4388), "light/discs": (29864, 10498), "light/borders": (1931, 1429),
        "above0.01/aimed": (2876, 1227), "above0.01/borders": (630, 513), "above0.0001/aimed": (3705, 1225),
        "above0.0001/borders": (1112, 564), "above1e-06/aimed": (4095, 1246), "above1e-06/borders": (1406, 644),
        "vertex/aimed": (2958, 1188), "vertex/borders": (770, 517), "light_twin/shadow": (1345, 916),
        "ortho0/shadow": (828, 769), "ortho1/shadow": (884, 816), "ortho2/shadow": (1718, 1103),
    },
}


def record(**kw):
    print("OG-RECORD " + " ".join(f"{k}={v}" for k, v in kw.items()))


def cap(rows, n, rng):
    """(at most n of the rows, how many were dropped)."""
    if len(rows) <= n:
        return rows, 0
    return rows[np.sort(rng.choice(len(rows), n, replace=False))], len(rows) - n


# ---------------------------------------------------------------------------------------------------------------------
# ray sets
# ---------------------------------------------------------------------------------------------------------------------
def aimed_targets(P, O, rng, max_tris=400):
    """float64 points to aim at from O (set a)."""
    pts = []
    tri = P["tri"][~P["is_sphere"]].astype(np.float64)
    if len(tri):
        t = tri[rng.choice(len(tri), min(len(tri), max_tris), replace=False)]
        c = t.mean(axis=1)
        for k in range(3):
            a, b = t[:, k], t[:, (k + 1) % 3]
            pts.append(a)
            for s in (0.5, 0.01):
                m = a + s * (b - a)
                for eps in (0.0, 1e-7, -1e-7, 1e-6, 1e-5, 1e-4):
                    pts.append(m + eps * (m - c))
    sph = P["is_sphere"]
    ph = np.linspace(0, 2 * np.pi, 24, endpoint=False)
    fr = np.array([1.0, 1 - 1e-7, 1 - 1e-6, 1 - 1e-5, 1 - 1e-4, 1 - 1e-3, 0.9, 0.0])
    for c, r in zip(P["centre"][sph].astype(np.float64), np.abs(P["radius"][sph].astype(np.float64))):
        v = c - O
        D = np.linalg.norm(v)
        if D <= r:
            continue
        ax = v / D
        u = np.cross(ax, [0.3, 0.5, 0.8])
        u /= np.linalg.norm(u)
        w = np.cross(ax, u)
        sin_a = r / D
        cos_a = np.sqrt(1 - sin_a ** 2)
        ring = np.cos(ph)[:, None] * u + np.sin(ph)[:, None] * w                     # [24, 3]
        pts.append((O + D * cos_a * (cos_a * ax + sin_a * fr[:, None, None] * ring[None])).reshape(-1, 3))
    return np.concatenate(pts)


def rays_at(O32, pts):
    d = pts - O32.astype(np.float64)
    n = np.linalg.norm(d, axis=1)
    d = (d[n > 0] / n[n > 0, None]).astype(F32)
    return np.concatenate([np.broadcast_to(O32, d.shape), d], axis=1).astype(F32)


def disc_rays(P, O32, prims, per, rng):
    """`per` rays over the disc of every sphere of `prims` as O sees it (set b), grown by 2 % so that the rim is inside."""
    O = O32.astype(np.float64)
    pts = []
    for p in prims:
        c, r = P["centre"][p].astype(np.float64), abs(float(P["radius"][p]))
        ax = (c - O) / np.linalg.norm(c - O)
        u = np.cross(ax, [0.3, 0.5, 0.8])
        u /= np.linalg.norm(u)
        w = np.cross(ax, u)
        rho, phi = 1.02 * np.sqrt(rng.uniform(0, 1, per)), rng.uniform(0, 2 * np.pi, per)
        pts.append(c + r * (rho * np.cos(phi))[:, None] * u + r * (rho * np.sin(phi))[:, None] * w)
    return rays_at(O32, np.concatenate(pts))


def step32(x, k):
    """The float32 k steps from x (k < 0: below)."""
    x = np.asarray(x, F32).copy()
    for _ in range(abs(k)):
        x = np.nextafter(x, F32(np.inf if k > 0 else -np.inf))
    return x


def border_rays(O32, res, n, rng, toward):
    """Set c: directions whose cube-map coordinates sit on cell borders of a res^3 grid, on seams and corners, and 1, 2, 4 float32
    steps to either side; each direction as it is (the face's axis is +-1) and normalised in float32.  A quarter of the rows are
    corners and seams anywhere; the others are the borders of the cells that the directions `toward` (the aimed set: where the
    geometry is) fall into - both coordinates snapped, or one of them."""
    face = rng.integers(0, 6, n)
    kb = rng.integers(0, res + 1, (n, 2))
    kb[: n // 8] = rng.choice([0, res], (n // 8, 2))                 # cube corners
    kb[n // 8: n // 4, 0] = rng.choice([0, res], n // 4 - n // 8)    # seams
    uv = (2.0 * kb / res - 1.0).astype(F32)
    w = toward[rng.integers(0, len(toward), n - n // 4)].astype(np.float64)
    axis = np.abs(w).argmax(axis=1)
    j = np.arange(len(w))
    face[n // 4:] = 2 * axis + (w[j, axis] < 0)
    free = np.stack([w[j, (axis + 1) % 3], w[j, (axis + 2) % 3]], axis=1) / np.abs(w[j, axis])[:, None]
    snapped = (2.0 * np.round((free + 1.0) * 0.5 * res) / res - 1.0)
    keep = rng.integers(0, 3, len(w))                                # 0: both snapped, 1 / 2: that coordinate stays free
    uv[n // 4:, 0] = np.where(keep == 1, free[:, 0], snapped[:, 0]).astype(F32)
    uv[n // 4:, 1] = np.where(keep == 2, free[:, 1], snapped[:, 1]).astype(F32)
    steps = rng.choice([0, 1, -1, 2, -2, 4, -4], (n, 2))
    for k in (1, -1, 2, -2, 4, -4):
        for c in (0, 1):
            sel = steps[:, c] == k
            uv[sel, c] = step32(uv[sel, c], k)
    d = np.zeros((n, 3), F32)
    i, axis = np.arange(n), face // 2
    d[i, axis] = np.where(face % 2 == 1, -1.0, 1.0)
    d[i, (axis + 1) % 3] = uv[:, 0]
    d[i, (axis + 2) % 3] = uv[:, 1]
    unit = (d * (F32(1.0) / wm.mag3(d))[:, None]).astype(F32)
    d = np.concatenate([d, unit])
    return np.concatenate([np.broadcast_to(O32, d.shape), d], axis=1).astype(F32)


# ---------------------------------------------------------------------------------------------------------------------
# one scene with its ray sets and brute-force lists, made once; the statements evaluated on any grid of it
# ---------------------------------------------------------------------------------------------------------------------
class Scene:
    def __init__(self, pta, oracle, family, instance):
        self.family, self.instance, self.pta = family, instance, pta
        if family == "specks":
            self.scene, self.floors, self.specks = gs.make(pta, instance)
        else:
            (self.scene, self.floors), self.specks = es.make(pta, family, instance), []
        self.P = es.primitives(self.scene)
        self.n_prims = len(self.P["is_sphere"])
        self.osc = oracle.OracleScene(self.scene.desc, oracle.PTO_BRUTE_FORCE)
        d = self.scene.desc.contents
        self.cam = camera_origin(self.scene)
        self.light = np.array(list(d.lights[0].vec), F32)
        self.ldir = np.array(list(d.lights[1].vec), F32)
        tri, sph = ~self.P["is_sphere"], self.P["is_sphere"]
        lo = np.concatenate([self.P["tri"][tri].reshape(-1, 3), (self.P["centre"] - self.P["radius"][:, None])[sph]]).min(axis=0)
        hi = np.concatenate([self.P["tri"][tri].reshape(-1, 3), (self.P["centre"] + self.P["radius"][:, None])[sph]]).max(axis=0)
        self.extent = float(np.linalg.norm(hi.astype(np.float64) - lo.astype(np.float64)))
        self.rng = np.random.default_rng(1000 + CASES.index((family, instance)))
        self.dropped = {}
        self._sets, self._shadow = {}, None

    def trace(self, rays):
        return self.osc.trace_all(rays, K)

    def origins(self):
        """(name, origin, extra) of the grids whose rays start at the origin; extra ones get smaller ray sets."""
        floor = next(iter(self.floors.values()))
        t = self.P["tri"][floor[len(floor) // 2]].astype(np.float64)
        n = np.cross(t[1] - t[0], t[2] - t[0])
        n /= np.linalg.norm(n)
        mid = 0.5 * t[0] + 0.3 * t[1] + 0.2 * t[2]
        out = [("camera", self.cam, False), ("light", self.light, False)]
        out += [(f"above{h:g}", (mid + n * h * self.extent).astype(F32), True) for h in (1e-2, 1e-4, 1e-6)]
        return out + [("vertex", t[0].astype(F32), True)]

    def grid(self, name, origin, res=0):
        """The host-built grid of an origin: the camera's with the parameters pt_scene_create derives, the others for rays that start
        at the origin with directions as long as set c makes them (a cube-map direction is up to sqrt 3 long)."""
        if name == "camera":
            return _host_twin(self.pta, self.scene, 0, res)
        return self.pta.OriginGrid(self.scene, origin, res, 0.0, F32(np.sqrt(3.0) * 1.001))

    def from_origin(self, name, origin, extra, res):
        """Sets a - c from one origin: {set: (rays, trace)}."""
        if name not in self._sets:
            sets, big = {}, "" if not extra else "_extra"
            rays, drop = cap(rays_at(origin, aimed_targets(self.P, origin.astype(np.float64), self.rng)), CAPS["aimed" + big], self.rng)
            self.dropped[(name, "aimed")] = drop
            sets["aimed"] = rays
            if self.specks and not extra:
                per, most = (240, CAPS["discs_camera"]) if name == "camera" else (120, CAPS["discs"])   # (the camera's feed the 500-per-wall floor)
                rays, drop = cap(disc_rays(self.P, origin, [s["prim"] for s in self.specks], per, self.rng), most, self.rng)
                self.dropped[(name, "discs")] = drop
                sets["discs"] = rays
            sets["borders"] = border_rays(origin, res, CAPS["borders" + big] // 2, self.rng, sets["aimed"][:, 3:])
            self._sets[name] = {k: (v, self.trace(v)) for k, v in sets.items()}
        return self._sets[name]

    def shadow(self):
        """Set d: dict(pos, point=(srays, trace, ldist), ortho=[(direction of the rays, srays, trace)])."""
        if self._shadow is None:
            cam = self._sets["camera"]
            rays = np.concatenate([cam[k][0] for k in ("aimed", "discs") if k in cam])
            hits = np.concatenate([cam[k][1][0][:, 0] for k in ("aimed", "discs") if k in cam])
            cnt = np.concatenate([cam[k][1][1] for k in ("aimed", "discs") if k in cam])
            sel, drop = cap(np.nonzero(cnt > 0)[0], CAPS["shadow"], self.rng)
            self.dropped[("camera", "shadow")] = drop
            rays, hits = rays[sel], hits[sel]
            tpar = np.where((hits["flags"] & 2) != 0, hits["dist"] / wm.mag3(rays[:, 3:]), hits["dist"]).astype(F32)
            pos = (rays[:, :3] + (rays[:, 3:] * tpar[:, None]).astype(F32)).astype(F32)
            gn = self.rng.normal(size=pos.shape).astype(F32)
            gn *= (self.rng.uniform(0.2, 1.5, len(pos)).astype(F32) / wm.mag3(gn))[:, None]
            so = (pos + (gn * F32(0.00001)).astype(F32)).astype(F32)
            direction = (pos - self.light).astype(F32)
            ldist = wm.mag3(direction)
            sd = (F32(-1.0) * (direction * (F32(1.0) / ldist)[:, None]).astype(F32)).astype(F32)
            srays = np.concatenate([so, sd], axis=1).astype(F32)
            ortho = []
            for ldir in (self.ldir,) + tuple(np.array(v, F32) for v in AXIS_LIGHTS):
                od = (F32(-1.0) * ldir).astype(F32)
                orays = np.concatenate([so, np.broadcast_to(od, so.shape)], axis=1).astype(F32)
                ortho.append((od, orays, self.trace(orays)))
            self._shadow = dict(pos=pos, point=(srays, self.trace(srays), ldist), ortho=ortho)
        return self._shadow


_SCENES = {}


@pytest.fixture(scope="module")
def scenes(pta, oracle):
    def get(family, instance):
        if (family, instance) not in _SCENES:
            _SCENES[(family, instance)] = Scene(pta, oracle, family, instance)
        return _SCENES[(family, instance)]
    yield get
    _SCENES.clear()


class Tally:
    """What one (scene, statement) run counted; `bad` collects the first violations."""

    def __init__(self):
        self.rows, self.bad = [], []
        self.ratio = 0.0          # largest undershoot / bound over the sphere entry hits of specks
        self.undershoot = {}      # wall -> camera rays whose first hit is a speck reported closer than D - r (D from the camera)

    def add(self, **kw):
        self.rows.append(kw)

    def fail(self, *what):
        if len(self.bad) < 8:
            self.bad.append(what)


def statement_a_origin(sc, lists, origin, rays, trace, tally, tag):
    """A for rays that start at the grid's origin."""
    hits, counts = trace
    valid = np.arange(K)[None, :] < np.minimum(counts, K)[:, None]
    cells = lists.grid.cells(rays[:, 3:])
    rank, word, is_global, found = lists.lookup(cells, np.where(valid, hits["prim"], -1))
    sphere = (hits["flags"] & 2) != 0
    dlen = np.linalg.norm(rays[:, 3:].astype(np.float64), axis=1)
    dist_o = np.where(sphere, hits["dist"].astype(np.float64), hits["dist"].astype(np.float64) * dlen[:, None])
    missing = valid & ~found
    over = valid & found & ~is_global & (word.astype(np.float64) > dist_o)
    for i, k in np.argwhere(missing)[:3]:
        tally.fail(tag, "missing", int(i), int(hits["prim"][i, k]), bool(sphere[i, k]))
    for i, k in np.argwhere(over)[:3]:
        tally.fail(tag, "bound", int(i), int(hits["prim"][i, k]), bool(sphere[i, k]), float(word[i, k]), float(dist_o[i, k]))
    tally.add(set=tag, rays=len(rays), checked=int(valid.sum()), missing=int(missing.sum()), over=int(over.sum()),
              over_spheres=int((over & sphere).sum()))
    if sc.specks:   # undershoot against the bound, over the entry hits of the spheres
        O = origin.astype(np.float64)
        p = np.where(valid, hits["prim"], 0)
        Dr = np.linalg.norm(sc.P["centre"][p].astype(np.float64) - O, axis=2) - np.abs(sc.P["radius"][p].astype(np.float64))
        entry = valid & found & ~is_global & sphere & ((hits["flags"] & 4) == 0)
        under, bound = Dr - dist_o, Dr - word.astype(np.float64)
        sel = entry & (under > 0)
        if sel.any():
            with np.errstate(divide="ignore"):
                tally.ratio = max(tally.ratio, float(np.max(np.where(bound[sel] > 0, under[sel] / bound[sel], np.inf))))
        first = (counts > 0) & sphere[:, 0] & ((hits["flags"][:, 0] & 4) == 0) & (under[:, 0] > 0) & tag.startswith("camera/")
        where = {s["prim"]: s["where"] for s in sc.specks}
        for q in hits["prim"][first, 0]:
            w = where.get(int(q))
            tally.undershoot[w] = tally.undershoot.get(w, 0) + 1


def statement_b_origin(lists, rays, trace, tally, tag):
    got, want = wm.closest(lists, rays, trace), wm.first_of(trace)
    wrong = ~wm.same_hit(got, want) & ~got["truncated"]
    for i in np.nonzero(wrong)[0][:3]:
        tally.fail(tag, "closest", int(i), int(got["prim"][i]), float(got["key"][i]), int(want["prim"][i]), float(want["key"][i]))
    tally.add(set=tag, rays=len(rays), hit_rays=int((trace[1] > 0).sum()), wrong=int(wrong.sum()), set_aside=int(got["truncated"].sum()))


def statement_point(lists, sh, tally, tag, want):
    srays, trace, ldist = sh["point"]
    r = wm.blocked_point(lists, srays, trace, sh["pos"], ldist)
    if want == "A":
        hits = trace[0]
        sphere = (hits["flags"] & 2) != 0
        sd = srays[:, None, 3:].astype(np.float64)
        t = np.where(sphere, hits["dist"] / np.linalg.norm(sd, axis=2), hits["dist"]).astype(np.float64)
        x = srays[:, None, :3].astype(np.float64) + sd * t[:, :, None]
        dist_o = np.linalg.norm(x - np.array(list(lists.grid.c.origin), np.float64), axis=2)
        missing = r["needed"] & ~r["found"]
        over = r["needed"] & r["found"] & ~r["is_global"] & (r["word"].astype(np.float64) > dist_o)
        for i, k in np.argwhere(missing | over)[:3]:
            tally.fail(tag, "missing" if missing[i, k] else "bound", int(i), int(hits["prim"][i, k]), float(r["word"][i, k]), float(dist_o[i, k]))
        tally.add(set=tag, rays=len(srays), checked=int(r["needed"].sum()), missing=int(missing.sum()), over=int(over.sum()),
                  over_spheres=int((over & sphere).sum()))
    else:
        wrong = (r["blocked"] != r["expected"]) & ~r["truncated"]
        for i in np.nonzero(wrong)[0][:3]:
            tally.fail(tag, "blocked_point", int(i), bool(r["blocked"][i]), bool(r["expected"][i]))
        tally.add(set=tag, rays=len(srays), hit_rays=int(r["expected"].sum()), wrong=int(wrong.sum()), set_aside=int(r["truncated"].sum()))


def statement_ortho(lists, srays, trace, tally, tag, want):
    r = wm.blocked_ortho(lists, srays, trace)
    if want == "A":
        missing = r["needed"] & ~r["found"]
        over = r["needed"] & r["found"] & ~r["is_global"] & (r["word"] > r["limit"][:, None])
        for i, k in np.argwhere(missing | over)[:3]:
            tally.fail(tag, "missing" if missing[i, k] else "key", int(i), int(trace[0]["prim"][i, k]), float(r["word"][i, k]), float(r["limit"][i]))
        tally.add(set=tag, rays=len(srays), checked=int(r["needed"].sum()), missing=int(missing.sum()), over=int(over.sum()),
                  over_spheres=int((over & ((trace[0]["flags"] & 2) != 0)).sum()))
    else:
        wrong = (r["blocked"] != r["expected"]) & ~r["truncated"]
        for i in np.nonzero(wrong)[0][:3]:
            tally.fail(tag, "blocked_ortho", int(i), bool(r["blocked"][i]), bool(r["expected"][i]))
        tally.add(set=tag, rays=len(srays), hit_rays=int(r["expected"].sum()), wrong=int(wrong.sum()), set_aside=int(r["truncated"].sum()))


def run_statements(sc, want, grids=None):
    """Statement `want` ('A' or 'B') of scene sc on the host-built grids, or on `grids` = {name: grid} (the device's camera grid
    and light grids: 'camera', 'light_twin', 'ortho0').  Returns the Tally."""
    tally = Tally()
    host = grids is None
    for name, origin, extra in sc.origins():
        if not host and name != "camera":
            continue
        grid = sc.grid(name, origin) if host else grids["camera"]
        if not grid.enabled:   # a valid answer; say so
            tally.add(set=f"{name}", disabled=1)
            continue
        lists = wm.Lists(grid, sc.n_prims)
        if not lists.lists_sorted():
            tally.fail(name, "a cell's list does not ascend")
        for tag, (rays, trace) in sc.from_origin(name, origin, extra, grid.res).items():
            if want == "A":
                statement_a_origin(sc, lists, origin, rays, trace, tally, f"{name}/{tag}")
            else:
                statement_b_origin(lists, rays, trace, tally, f"{name}/{tag}")
    sh = sc.shadow()
    twin = _host_twin(sc.pta, sc.scene, 1, 0) if host else grids["light_twin"]
    if twin.enabled:
        lists = wm.Lists(twin, sc.n_prims)
        if not lists.lists_sorted():
            tally.fail("light_twin", "a cell's list does not ascend")
        statement_point(lists, sh, tally, "light_twin/shadow", want)
    else:
        tally.add(set="light_twin", disabled=1)
    for k, (od, srays, trace) in enumerate(sh["ortho"]):
        if not host and k > 0:
            break
        og = sc.pta.OriginGrid(sc.scene, direction=od) if host else grids["ortho0"]
        if not og.enabled:
            tally.add(set=f"ortho{k}", disabled=1)
            continue
        lists = wm.Lists(og, sc.n_prims)
        if not lists.lists_sorted():
            tally.fail(f"ortho{k}", "a cell's list does not ascend")
        statement_ortho(lists, srays, trace, tally, f"ortho{k}/shadow", want)
    return tally


def report(sc, want, tally, where="host"):
    for row in tally.rows:
        record(statement=want, lists=where, family=sc.family, instance=sc.instance, **row)
    for (name, what), n in sc.dropped.items():
        if n:
            record(statement=want, lists=where, family=sc.family, instance=sc.instance, set=f"{name}/{what}", rows_dropped_by_cap=n)
    if want == "A" and sc.specks:
        record(statement=want, lists=where, family=sc.family, instance=sc.instance, undershoot_over_bound=f"{tally.ratio:.4f}",
               **{f"undershoot_rays_{k}": v for k, v in sorted(tally.undershoot.items(), key=str)})


def check(sc, want, tally):
    assert not tally.bad, tally.bad
    assert all(r.get("missing", 0) == 0 and r.get("over", 0) == 0 and r.get("wrong", 0) == 0 for r in tally.rows)
    for r in tally.rows:   # the cap on what is set aside, per set
        assert r.get("set_aside", 0) <= SET_ASIDE_CAP * r.get("rays", 0), r
    # floors against vacuity: half of what the first CPU run counted, the smallest instance of the family
    for r in tally.rows:
        if not r.get("disabled"):
            floor = MIN_CHECKED[sc.family].get(r["set"], (0, 0))[0 if want == "A" else 1]   # (no entry: declined in that run)
            assert r["checked" if want == "A" else "hit_rays"] >= floor, (r, floor)
    if want == "A" and sc.specks:
        assert tally.ratio <= 1.0, tally.ratio
        for w in (0, 1, 2, 3):
            assert tally.undershoot.get(w, 0) >= 500, (w, tally.undershoot)


@pytest.mark.parametrize("family,instance", CASES, ids=IDS)
def test_lists_hold_every_needed_hit(scenes, family, instance):
    """Statement A on the host-built grids."""
    sc = scenes(family, instance)
    tally = run_statements(sc, "A")
    report(sc, "A", tally)
    check(sc, "A", tally)


@pytest.mark.parametrize("family,instance", CASES, ids=IDS)
def test_walks_return_the_oracles_answer(scenes, family, instance):
    """Statement B on the host-built grids."""
    sc = scenes(family, instance)
    tally = run_statements(sc, "B")
    report(sc, "B", tally)
    check(sc, "B", tally)


# ---------------------------------------------------------------------------------------------------------------------
# nothing else moved: the lists of triangle scenes are the parent's, byte for byte
# ---------------------------------------------------------------------------------------------------------------------
DIGEST_SCENES = ("cube", "head", "reflection", "generated20000")
SPHERE_SCENES = ("spheres", "white_furnace_indirect")


def _sha(a):
    return hashlib.sha1(np.ascontiguousarray(a).tobytes()).hexdigest()


def grid_digests(pta, scene_cache):
    """{scene: {grid: {array: SHA-1}}} of the host builder's camera grid and first light grid.  Triangle scenes: cell_off,
    ref_prim and the bits of ref_mindist.  Sphere scenes: cell_off and ref_prim sorted within the global block and within each
    cell (the order within a cell may move with the spheres' distance words)."""
    out = {}
    for name in DIGEST_SCENES + SPHERE_SCENES:
        scene = pta.HostScene.generate_ps5(20000, seed=0) if name == "generated20000" else scene_cache(name)
        out[name] = {}
        for which in range(1 + min(1, int(scene.desc.contents.n_lights))):
            g = _host_twin(pta, scene, which, 0)
            assert g.enabled, (name, which)
            n = g.n_refs
            if name in SPHERE_SCENES:
                off = g.cell_off.astype(np.int64)
                owner = np.concatenate([np.full(int(off[0]), -1, np.int64), np.repeat(np.arange(len(off) - 1), np.diff(off))])
                order = np.lexsort((g.ref_prim[:n], owner))
                d = dict(cell_off=_sha(g.cell_off), ref_prim_sets=_sha(g.ref_prim[:n][order]))
            else:
                d = dict(cell_off=_sha(g.cell_off), ref_prim=_sha(g.ref_prim[:n]), ref_mindist=_sha(g.ref_mindist[:n].view(np.uint32)))
            out[name]["camera" if which == 0 else "light0"] = d
            g.close()
    return out


def test_lists_of_the_golden_scenes_are_unchanged(pta, scene_cache):
    """tests/golden/origin_grid_digests.json was written by the builder as it was before sphere_footprint's distance bound changed:
    triangle-only scenes (every benchmark configuration is one) keep their lists byte for byte, sphere scenes keep every cell's set
    of primitives."""
    want = json.loads((GOLDEN / "origin_grid_digests.json").read_text())
    assert grid_digests(pta, scene_cache) == want


# ---------------------------------------------------------------------------------------------------------------------
# the device: its lists, and frames through them
# ---------------------------------------------------------------------------------------------------------------------
_GPU = {}


@pytest.fixture(scope="module")
def gpu_scenes(pta, scenes):
    def get(family, instance):
        if (family, instance) not in _GPU:
            _GPU[(family, instance)] = pta.GpuScene(scenes(family, instance).scene)
        return _GPU[(family, instance)]
    yield get
    for g in _GPU.values():
        g.close()
    _GPU.clear()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def frames_differ(got, want):
    """(pixels whose rgb8 differs, pixels whose accumulator differs in a bit - NaN equals NaN)."""
    g, w = np.asarray(got[1], np.float32), np.asarray(want[1], np.float32)
    same = (bits(g) == bits(w)) | (np.isnan(g) & np.isnan(w))
    return int((got[0] != want[0]).any(axis=1).sum()), int((~same).any(axis=1).sum())


@pytest.mark.gpu
@pytest.mark.parametrize("family,instance", CASES, ids=IDS)
def test_device_lists_equal_the_host_twins_and_hold_a_and_b(pta, scenes, gpu_scenes, family, instance):
    """The camera grid and both light grids the device built equal the host twins byte for byte (a grid the host builder declines
    is declined on the device, and with it the other light's: a scene's shadow rays take the light grids only if every light has
    one), and statements A and B hold on the device's arrays."""
    sc, g = scenes(family, instance), gpu_scenes(family, instance)
    grids, declined = {}, []
    light_grids = g.info().as_dict()["light_grids"]
    for which, name in ((0, "camera"), (1, "light_twin"), (2, "ortho0")):
        dev = pta.OriginGrid.from_device(g, which)
        host = _host_twin(pta, sc.scene, which, dev.res if dev.enabled else 0)
        record(lists="device", family=family, instance=instance, grid=name, enabled=int(dev.enabled), res=dev.res, n_global=dev.n_global,
               n_refs=dev.n_refs, host_twin_enabled=int(host.enabled))
        if not host.enabled:
            declined.append(name)
        if which == 0 or light_grids:   # (a scene's shadow rays take the light grids only if EVERY light has one: all or none)
            assert dev.enabled == host.enabled, (name, dev.enabled, host.enabled)
        else:
            assert not dev.enabled, name
        if dev.enabled:
            assert host.res == dev.res and host.n_global == dev.n_global and host.n_refs == dev.n_refs, name
            assert np.array_equal(host.cell_off, dev.cell_off), name
            assert np.array_equal(host.ref_prim[:host.n_refs], dev.ref_prim[:dev.n_refs]), name
            assert np.array_equal(host.ref_mindist[:host.n_refs].view(np.uint32), dev.ref_mindist[:dev.n_refs].view(np.uint32)), name
        host.close()
        grids[name] = dev
    # the device may go without light grids only where the host builder declines one of them
    assert light_grids == 2 or (light_grids == 0 and set(declined) & {"light_twin", "ortho0"}), (light_grids, declined)
    for want in "AB":
        tally = run_statements(sc, want, grids)
        report(sc, want, tally, "device")
        check(sc, want, tally)


@pytest.mark.gpu
@pytest.mark.parametrize("family,instance", CASES, ids=IDS)
def test_frames_equal_the_oracle_on_every_path(pta, oracle, scenes, gpu_scenes, family, instance):
    """96 x 64 at 4 samples, 0 and 2 bounces: the default path, PT_FLAG_NO_GRIDS and PT_FLAG_MEGAKERNEL give the oracle's frame bit
    for bit (rgb8 and the float32 accumulator).  The scene must have its camera grid and both light grids, else the default path
    says nothing about them.

    placed-3 (the skyline scaled by 1e-2) had no light grids at first: the point light is 0.022 above a floor of 2e-3 triangles,
    inside the radius within which the builder sent everything to the global list (the ray offset worth 1/8 cell), 202
    primitives where a grid may have 64.  That radius is now the ray offset worth 8 cells (host/origin_grid.cpp): the margin
    carries the offset's angle anyway."""
    sc, g = scenes(family, instance), gpu_scenes(family, instance)
    bad = []
    for bounces in (0, 2):
        prof = pta.Profile.make(96, 64, 4, bounces)
        rgb, acc, stats = sc.osc.render(prof)
        for flags in (0, pta.PT_FLAG_NO_GRIDS, pta.PT_FLAG_MEGAKERNEL):
            d = frames_differ(g.render(prof, pta.Opts.make(flags=flags)), (rgb, acc))
            record(frames=family, instance=instance, bounces=bounces, flags=flags, rgb8_differ=d[0], accum_differ=d[1],
                   oracle_numeric_errors=stats["numeric_errors"])
            if d != (0, 0):
                bad.append((bounces, flags, d))
    info = g.info().as_dict()
    record(frames=family, instance=instance, cam_grid_res=info["cam_grid_res"], light_grids=info["light_grids"])
    assert not bad, bad
    assert info["cam_grid_res"] > 0 and info["light_grids"] == 2, info


# (wall, r, placement) of the speck views: wall 1 is the one 3.1 away; (1, 1e-3, 2e-4) is the view in which the parent's bound let
# the default path return the wall where the oracle's first hit is the speck
SPECK_VIEWS = [(1, 1e-3, 2e-4), (1, 1e-3, 3e-4), (1, 3e-3, 2e-4), (1, 1e-3, "front"), (1, 3e-4, "sunk"), (1, 3e-4, 1e-4),
               (0, 1e-3, 2e-4), (2, 1e-3, 2e-4), (3, 1e-3, 2e-4), (3, 3e-4, "front"), ("floor", 1e-3, 2e-4)]


DIRECTED_VIEWS = [(1e-3, 2e-4), (1e-3, 3e-4), (3e-3, 2e-4)]   # grid_scenes.directed: the wall on the view axis, one speck behind it


def _speck_frames(pta, oracle, built, views, prof, bad):
    g = pta.GpuScene(built)
    for label, rec in views:
        cam = gs.speck_view(pta, built, rec)
        built._desc.camera = cam
        g.set_camera(cam)
        rgb, acc, stats = oracle.OracleScene(built.desc, oracle.PTO_BRUTE_FORCE).render(prof)
        info = g.info().as_dict()
        for flags in (0, pta.PT_FLAG_NO_GRIDS, pta.PT_FLAG_MEGAKERNEL):
            d = frames_differ(g.render(prof, pta.Opts.make(flags=flags)), (rgb, acc))
            record(speck_view=label, flags=flags, rgb8_differ=d[0], accum_differ=d[1], cam_grid_res=info["cam_grid_res"],
                   light_grids=info["light_grids"], oracle_numeric_errors=stats["numeric_errors"])
            if d != (0, 0):
                bad.append((label, flags, d))
        if not (info["cam_grid_res"] > 0 and info["light_grids"] == 2):
            bad.append((label, "a grid is missing", info["cam_grid_res"], info["light_grids"]))
    g.close()


@pytest.mark.gpu
def test_speck_frames_equal_the_oracle_on_every_path(pta, oracle):
    """The flat speck scene and the directed scenes seen through narrow cameras (scene_builder.make_camera) in which one speck is
    24 pixels across, one pt_scene_set_camera per view on one scene: 96 x 64 at 4 samples and 0 bounces on the three paths
    against the oracle.

    Observed on the MI355X with the parent's libraries (pixels that differ from the oracle: default / NO_GRIDS / MEGAKERNEL):
    wall 1 (3.1 away), every view 0 / 0 / 0 - the walk model on the parent's lists says 0 wrong rays there too; wall 2 (30 away),
    r 1e-3 k, gap 2e-4 k: 33 / 0 / 0 (the model: 35 wrong rays in 33 pixels); wall 3 (300 away), the same speck: 396 / 63 / 61
    (the model: 587 wrong rays in 396 pixels); the floor speck: 1 / 0 / 0 (the model: 1 ray); the directed scene at r 1e-3, gaps
    2e-4 and 3e-4: 470 / 0 / 0 (the model: 765 wrong rays in 470 pixels), at r 3e-3, gap 2e-4: 21 / 0 / 0 (the model: 27 rays in
    21 pixels).

    With the bound of sphere_footprint derived from the quadratic the default path equals the oracle in every view.  The view
    of wall 3 (300 away, r = 0.097, the wall 0.019 in front of the speck) then still differed on the two paths that walk the
    KD-tree, NO_GRIDS in 63 pixels and MEGAKERNEL in 61, as on the parent: the quadratic reports that speck up to 0.24 in
    front of its surface, outside the sphere's own box, and the walk ends where the next node starts behind the best hit.
    host/kd_build.cpp now enters a sphere with its box grown by that undershoot."""
    prof = pta.Profile.make(96, 64, 4, 0)
    bad = []
    built, _, specks = gs.make(pta, 0)
    views = [(f"{w}/{r:g}/{p}", next(s for s in specks if (s["where"], s["r"], s["place"]) == (w, r, p))) for w, r, p in SPECK_VIEWS]
    _speck_frames(pta, oracle, built, views, prof, bad)
    for r, gap in DIRECTED_VIEWS:
        built, rec = gs.directed(pta, r, gap)
        _speck_frames(pta, oracle, built, [(f"directed/{r:g}/{gap:g}", rec)], prof, bad)
    assert not bad, bad
