"""Hostile scenes for the escape masks (csrc/pt_escape_build.h): geometry that sits at the builder's thresholds, seeded and
deterministic, plain numpy.  Every family is a tessellated floor patch (triangles 0.05 - 0.3 across) plus what the family is
about; `make(pta, name, instance)` returns the scene_builder.BuiltScene and a dict {name: primitive indices} of its "floor"
primitives - the ones expected to have masks.  Every scene has at most 3 000 primitives (the oracle's brute force is cheap),
the background (0.3, 0.5, 0.9) (a masked miss changes the pixel), one point and one directional light, the camera looking at
the structure, material k on model k with metalness / roughness alternated as in tests/test_geometry_model.py::built.

What each family probes (k_escape_build's thresholds: cut = H_LO / 4 = 1.25e-6, cut_c = H_LO / 16 = 3.125e-7, H_LO = 5e-6,
H_HI = 1e-3, dist > 2 (r_o + rb), dq > 1.05 (r_o + rqf), H_LO < 2e-6 reach_a, sin_b, rho + 2e-5):
  terraces   neighbouring strips raised by steps on both sides of cut_c, cut, H_LO, H_HI and beyond;
  hinges     pairs of strips that share an edge, tilted about it by +-1e-6 ... +-1e-1 rad: nearly coplanar convex and concave
             neighbours (cut, cut_c, sin_b, the leaf-primitive test);
  resting    needles, tetrahedra and spheres on, above (gaps 1e-6 ... 1e-2) and sunk into the floor, tangent sphere pairs, over
             a triangle's interior, its vertex and just outside its edge (cut, the leaf-primitive test);
  skyline    thin poles and a wall 10 x, 100 x and 1000 x the triangle size away, narrower than a cell and some narrower than
             alpha_stop, straddling cell borders, face seams and cube corners as seen from the patch centre (rho, alpha_stop,
             the node test);
  dome       a convex dome of ~300 facets whose neighbours fall away below each facet's plane, a pole beside it and a second
             dome above it (sin_b, reach_b);
  normals    vertex normals opposite to the winding, of length 1.5 and 60 degrees off the geometric normal, a coincident
             duplicate wound the other way, a zero-area triangle (the side a mask faces, cut_c, the degenerate test);
  reach      lone floor triangles whose origin-set radius is 1.0, 1.2, 1.3 and 2.0 (the reach_a limit is ~1.25) and a floor
             with tall geometry at the rim;
  placed     terraces and skyline scaled by 1e-2 and 1e2 and translated by (1000, -2000, 500) (the absolute thresholds against
             the scene's size, the rounding of large coordinates).
Half of the instances of every family are tilted by a fixed rotation about no axis, so that no plane coincides with a KD split
or a cube-map face."""
import ctypes as C

import numpy as np

import scene_builder as sb

BACKGROUND = (0.3, 0.5, 0.9)
STEPS = (1e-7, 1e-6, 1.25e-6, 1.3e-6, 2e-6, 5e-6, 1e-5, 1e-4, 1e-3, 1e-2)
HINGE_ANGLES = (1e-6, 1e-5, 1e-4, 1e-3, 1e-2, 1e-1)
GAPS = (1e-6, 1e-5, 1e-4, 1e-3, 1e-2)
REACH_RADII = (1.0, 1.2, 1.3, 2.0)
MAX_PRIMS = 3000


def _rotation(axis, angle):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


TILT = _rotation((0.37, 0.21, -0.58), 0.83)   # the fixed rotation of the tilted instances


# ---------------------------------------------------------------------------------------------------------------------
# pieces (local frame: the floor is y = 0, its normal +y)
# ---------------------------------------------------------------------------------------------------------------------
def patch(x0, z0, nx, nz, s, height=None):
    """nx x nz quads of side s from (x0, z0), two triangles each, wound so that the geometric normal is +y; height(x, z)
    gives y (default 0).  [2 nx nz, 3, 3], quad-major: triangle 2 q and 2 q + 1 are quad q = ix * nz + iz."""
    ix, iz = np.meshgrid(np.arange(nx), np.arange(nz), indexing="ij")
    ix, iz = ix.reshape(-1), iz.reshape(-1)

    def p(dx, dz):
        x, z = x0 + (ix + dx) * s, z0 + (iz + dz) * s
        y = np.zeros_like(x) if height is None else height(x, z)
        return np.stack([x, y, z], axis=1)
    p00, p01, p10, p11 = p(0, 0), p(0, 1), p(1, 0), p(1, 1)
    t = np.empty((len(ix), 2, 3, 3))
    t[:, 0] = np.stack([p00, p01, p10], axis=1)
    t[:, 1] = np.stack([p10, p01, p11], axis=1)
    return t.reshape(-1, 3, 3)


def pole(foot, up, height, width):
    """Two crossed quads (4 triangles) standing on `foot` along the unit vector `up`."""
    up = np.asarray(up, np.float64) / np.linalg.norm(up)
    a = np.cross(up, (0.31, 0.2, 0.93))
    a /= np.linalg.norm(a)
    b = np.cross(up, a)
    foot, out = np.asarray(foot, np.float64), []
    for side in (a, b):
        q = [foot - 0.5 * width * side, foot + 0.5 * width * side, foot + 0.5 * width * side + height * up,
             foot - 0.5 * width * side + height * up]
        out += [[q[0], q[1], q[2]], [q[0], q[2], q[3]]]
    return np.array(out)


def tetra(base, size):
    b = np.asarray(base, np.float64)
    v = [b + (0, 0, 0), b + (size, 0, 0.1 * size), b + (0.4 * size, 0, size), b + (0.45 * size, size, 0.4 * size)]
    return np.array([[v[0], v[1], v[2]], [v[0], v[3], v[1]], [v[1], v[3], v[2]], [v[2], v[3], v[0]]])


def dome(centre, radius, rings, segs, cap=0.5 * np.pi):
    """The cap of a sphere around +y down to the polar angle `cap`, flat facets wound outwards: segs + 2 segs (rings - 1)."""
    c = np.asarray(centre, np.float64)

    def p(i, j):
        th, ph = cap * i / rings, 2 * np.pi * (j % segs) / segs
        return c + radius * np.array([np.sin(th) * np.cos(ph), np.cos(th), np.sin(th) * np.sin(ph)])
    out = []
    for j in range(segs):
        out.append([p(0, 0), p(1, j + 1), p(1, j)])
        for i in range(1, rings):
            out += [[p(i, j), p(i, j + 1), p(i + 1, j + 1)], [p(i, j), p(i + 1, j + 1), p(i + 1, j)]]
    return np.array(out)


def mesh(tris, floor=None, normals=None):
    return dict(kind="mesh", tris=np.asarray(tris, np.float64).reshape(-1, 3, 3), normals=normals, floor=floor)


def sphere(centre, radius):
    return dict(kind="sphere", centre=np.asarray(centre, np.float64), radius=float(radius), floor=None)


# ---------------------------------------------------------------------------------------------------------------------
# the layouts: (models, centre of the structure, its extent)
# ---------------------------------------------------------------------------------------------------------------------
def terraces(R):
    """11 strips of 4 x 12 quads of 0.15; strip k + 1 stands STEPS[k] above or below strip k, the sign alternating by pairs (so
    the heights stay small and second neighbours differ by sums and differences of the steps)."""
    s, models, h = 0.15, [], 0.0
    for k in range(11):
        if k:
            h += STEPS[k - 1] * (1.0 if (k // 2) % 2 == 0 else -1.0)
        models.append(mesh(patch(k * 4 * s, 0.0, 4, 12, s, lambda x, z, h=h: np.full_like(x, h)), floor=f"strip{k}"))
    return models, np.array([22 * s, 0.0, 6 * s]), 44 * s


def hinges(R):
    """12 units on a 6 x 2 grid: two strips of 3 x 8 quads of 0.15 that share the edge x = x0; the second is turned about it by
    -angle (convex: it falls away) or +angle (concave: it rises)."""
    s, models = 0.15, []
    for i, ang in enumerate([sg * a for a in HINGE_ANGLES for sg in (-1.0, 1.0)]):
        x0, z0 = (i % 6) * 1.3, (i // 6) * 1.6
        flat = patch(x0 - 3 * s, z0, 3, 8, s)
        wing = patch(x0, z0, 3, 8, s)
        d = wing[:, :, 0] - x0
        wing[:, :, 0], wing[:, :, 1] = x0 + d * np.cos(ang), d * np.sin(ang)
        models.append(mesh(flat, floor=f"flat{i}"))
        models.append(mesh(wing, floor=f"wing{i}"))
    return models, np.array([3.25, 0.0, 1.4]), 8.0


def resting(R):
    """A floor of 16 x 16 quads of 0.2 and, on a 5 x 5 grid of sites, needles (1 : 1000), tetrahedra and spheres (radius 1e-3
    ... 0.1) at the gaps of GAPS above it, on it and sunk into it - over a triangle's interior, over a vertex and just outside
    an edge in turn; two tangent sphere pairs; one sphere of radius 0.5 at the rim."""
    s = 0.2
    models = [mesh(patch(0.0, 0.0, 16, 16, s), floor="floor")]
    needles, tetras, k = [], [], 0
    radii = (1e-3, 1e-2, 0.1, 3e-3, 0.03, 0.06, 0.02)
    for kind in range(3):
        for gi, gap in enumerate(GAPS + (0.0, None)):
            site = np.array([0.4 + 0.6 * (k % 5), 0.0, 0.4 + 0.6 * (k // 5)])
            where = k % 3   # 0: the interior of the triangle (site, +z, +x); 1: the vertex; 2: just outside its hypotenuse
            site += ((0.3 * s, 0, 0.3 * s), (0, 0, 0), (0.5 * s + 1e-3, 0, 0.5 * s + 1e-3))[where]
            if kind == 0:
                y = -1e-4 if gap is None else gap
                lean = 0.0 if gi % 2 == 0 else 0.2   # flat, or one end raised
                a = site + (0, y, 0)
                needles.append([a, a + (2e-4, 0, 0), a + (1e-4, lean, 0.2)])
            elif kind == 1:
                tetras.append(tetra(site + (0, -0.01 if gap is None else gap, 0), 0.02))
            else:
                r = radii[gi]
                models.append(sphere(site + (0, 0.5 * r if gap is None else r + gap, 0), r))
            k += 1
    models.append(mesh(np.array(needles)))
    models.append(mesh(np.concatenate(tetras)))
    for c, r1, r2 in (((2.9, 0.0, 0.5), 0.05, 0.03), ((2.9, 0.0, 1.7), 0.01, 0.1)):   # tangent pairs: one on the floor, one on it
        c = np.array(c)
        models.append(sphere(c + (0, r1, 0), r1))
        models.append(sphere(c + (0, 2 * r1 + r2, 0), r2))
    models.append(sphere((2.9, 0.5, 2.9), 0.5))
    return models, np.array([1.6, 0.0, 1.6]), 3.2


# directions (world frame) whose cube-map coordinates sit on cell borders (a multiple of 0.25), face seams and cube corners
SKYLINE_DIRS = ((1, 0.25, 0.25), (1, 0.5, 0.1), (1, 0.3, -0.75), (0.25, 0.5, -1), (-0.5, 0.25, -1), (-1, 0.75, 0.5),
                (1, 1, 0.3), (-1, 1, 0.5), (0.4, 1, 1), (0.2, 1, -1), (1, 1, 1), (-1, 1, 1), (1, 1, -1), (-1, 1, -1),
                (0.25, 1, 0.25), (-0.5, 1, 0.75), (-1, 0.25, -0.25), (0.75, 0.25, 1), (1, -0.25, 0.5), (-0.25, -1, 0.5),
                (0.5, -0.5, 1), (-1, -1, 1), (1, -0.75, -1), (0.25, -0.25, -1))


def skyline(R, s=0.2):
    """A floor of 12 x 12 quads of s and thin poles 10 s, 100 s and 1000 s from its centre, each centred on one of SKYLINE_DIRS
    as the WORLD sees it (so the tilted instance straddles the same borders) where that is above the floor; the poles subtend
    0.06 rad (below a cell, above alpha_stop) or 0.02 rad (below alpha_stop); a town of 30 poles and one wall 100 s away."""
    models = [mesh(patch(0.0, 0.0, 12, 12, s), floor="floor")]
    c = np.array([6 * s, 0.0, 6 * s])
    poles, k = [], 0
    for w in SKYLINE_DIRS:
        d = R.T @ (np.asarray(w, np.float64) / np.linalg.norm(w))   # local direction that the tilt turns into w
        if d[1] < 0.08:
            continue
        dist = s * (10.0, 100.0, 1000.0)[k % 3]
        ang = (0.06, 0.02)[(k // 3) % 2]
        mid = c + dist * d
        poles.append(pole(mid - (0, 0.5 * ang * dist, 0), (0, 1, 0), ang * dist, 0.1 * ang * dist))
        k += 1
    models.append(mesh(np.concatenate(poles)))
    # a far town: 6 x 5 poles in a block 0.15 rad wide, 100 s away - a subtree of the KD-tree that PT_ESCAPE_ALPHA 0.2 takes whole
    # and 0.01 opens pole by pole
    town = c + 100.0 * s * (R.T @ sb._unit([-0.6, 0.35, -1.0]))
    models.append(mesh(np.concatenate([pole(town + s * np.array([2.5 * i, 0.0, 2.5 * j]), (0, 1, 0), s * (2.0 + (i + 2 * j) % 3), 0.2 * s)
                                       for i in range(6) for j in range(5)])))
    far = 100.0 * s
    wall = np.array([c + (-far, 0.05 * far, -0.1 * far), c + (-far, 0.05 * far, 0.1 * far), c + (-far, 0.12 * far, 0.1 * far),
                     c + (-far, 0.12 * far, -0.1 * far)])
    models.append(mesh([[wall[0], wall[1], wall[2]], [wall[0], wall[2], wall[3]]]))
    return models, c, 12 * s


def dome_family(R):
    """A floor of 12 x 12 quads of 0.3, a dome of 304 flat facets (radius 1.2, its centre 0.3 below the floor) in a corner region, a
    pole beside it, a second dome (radius 1, 132 facets) above it."""
    models = [mesh(patch(0.0, 0.0, 12, 12, 0.3), floor="floor")]
    models.append(mesh(dome((2.4, -0.3, 2.4), 1.2, 10, 16), floor="dome"))
    models.append(mesh(pole((3.4, 0.0, 1.1), (0, 1, 0), 2.0, 0.05)))
    models.append(mesh(dome((2.4, 2.2, 2.4), 1.0, 6, 12, cap=0.6 * np.pi)))
    return models, np.array([1.8, 0.3, 1.8]), 3.6


def normals_family(R):
    """A floor of 18 x 12 quads of 0.2 in three parts: (a) vertex normals opposite to the winding, (b) vertex normals of length
    1.5 tilted 60 degrees off the geometric normal (the azimuth differs from vertex to vertex), (c) plain normals, with a
    sub-patch of 3 x 3 quads duplicated coincident and wound the other way, and a zero-area triangle in the patch."""
    s = 0.2
    a, b, c = patch(0.0, 0.0, 6, 12, s), patch(1.2, 0.0, 6, 12, s), patch(2.4, 0.0, 6, 12, s)
    na = np.tile(np.array([0.0, -1.0, 0.0]), (len(a), 3, 1))
    az = 7.3 * b[:, :, 0] + 4.1 * b[:, :, 2]
    nb = 1.5 * np.stack([np.sin(np.pi / 3) * np.cos(az), np.full_like(az, np.cos(np.pi / 3)), np.sin(np.pi / 3) * np.sin(az)], axis=2)
    dup = patch(2.4 + 2 * s, 4 * s, 3, 3, s)[:, ::-1, :]
    flat = np.array([[[3.0, 0.0, 0.3], [3.1, 0.0, 0.35], [3.2, 0.0, 0.4]]])   # three points of a line, in the floor
    models = [mesh(a, floor="opposite", normals=na), mesh(b, floor="long", normals=nb), mesh(c, floor="plain"),
              mesh(dup, floor="duplicate"), mesh(flat)]
    return models, np.array([1.8, 0.0, 1.2]), 3.6


def reach(R):
    """A floor of 16 x 16 quads of 0.2 with two poles of height 1 at corners of its rim (tall geometry declines the triangles
    within its bounding sphere's reach: at the rim the middle of the floor stays examined) and, far from it and from each
    other, four lone right triangles whose origin-set radius (0.745 x the leg + delta_in + 1e-3) is 1.0, 1.2, 1.3 and 2.0,
    each 0.01 above the one before it, a pole of height 2.5 beside each."""
    models = [mesh(patch(0.0, 0.0, 16, 16, 0.2), floor="floor")]
    poles = [pole((x, 0.0, z), (0, 1, 0), 1.0, 0.03) for x, z in ((-0.05, -0.05), (3.25, 3.25))]
    for k, r in enumerate(REACH_RADII):
        leg = (r - 1e-3) / 0.7454
        x0, y0 = 12.0 + 12.0 * k, 0.01 * (k + 1)
        models.append(mesh([[(x0, y0, 0.0), (x0, y0, leg), (x0 + leg, y0, 0.0)]], floor=f"big{r}"))
        poles.append(pole((x0 + 2 * leg + 1.5, y0 - 0.5, 0.5), (0, 1, 0), 2.5, 0.05))
    models.append(mesh(np.concatenate(poles)))
    return models, np.array([1.6, 0.0, 1.6]), 3.2


LAYOUTS = dict(terraces=terraces, hinges=hinges, resting=resting, skyline=skyline, dome=dome_family, normals=normals_family,
               reach=reach)
# placed: (layout, uniform scale, translation); the instances alternate flat / tilted like those of every family
PLACED = (("terraces", 1e-2, (0, 0, 0)), ("terraces", 1e2, (0, 0, 0)), ("skyline", 1.0, (1000.0, -2000.0, 500.0)),
          ("skyline", 1e-2, (0, 0, 0)), ("skyline", 1e2, (0, 0, 0)), ("terraces", 1.0, (1000.0, -2000.0, 500.0)))
FAMILIES = tuple(LAYOUTS) + ("placed",)


def instances(family):
    """The instance numbers of a family: even ones flat, odd ones tilted."""
    return tuple(range(len(PLACED))) if family == "placed" else (0, 1)


# ---------------------------------------------------------------------------------------------------------------------
# layout -> BuiltScene
# ---------------------------------------------------------------------------------------------------------------------
def make(pta, family, instance=0):
    """(BuiltScene, {floor name: primitive indices}) of instance `instance` of a family."""
    tilted = instance % 2 == 1
    R = TILT if tilted else np.eye(3)
    layout, scale, shift = PLACED[instance] if family == "placed" else (family, 1.0, (0, 0, 0))
    models, centre, extent = LAYOUTS[layout](R)
    return build(pta, models, centre, extent, R, scale, shift)


def lone_triangle(pta, normal, size=0.2):
    """A scene of one triangle with the geometric normal `normal` (nothing rises above its plane, nothing lies below it: its mask
    is the grazing band alone)."""
    n = np.asarray(normal, np.float64) / np.linalg.norm(normal)
    a = np.cross(n, (0.0, 0.0, 1.0) if abs(n[2]) < 0.9 else (1.0, 0.0, 0.0))
    a /= np.linalg.norm(a)
    b = np.cross(n, a)
    return build(pta, [mesh([[(0.0, 0.0, 0.0), size * a, size * b]], floor="floor")], np.zeros(3), 1.0)


def build(pta, models, centre, extent, R=np.eye(3), scale=1.0, shift=(0, 0, 0)):
    """(BuiltScene, floors) of a list of models (mesh / sphere) in the local frame, scaled, turned by R and moved by shift."""
    shift = np.asarray(shift, np.float64)

    def place(p):
        return (np.asarray(p, np.float64) * scale) @ R.T + shift
    tris, out_models, mats, floors, prim = [], [], [], {}, 0
    for k, m in enumerate(models):
        albedo = (0.35 + 0.6 * ((k * 7) % 10) / 10.0, 0.35 + 0.6 * ((k * 3) % 10) / 10.0, 0.35 + 0.6 * ((k * 9) % 10) / 10.0)
        mats.append(pta.Material((C.c_float * 3)(*albedo), (C.c_float * 3)(0, 0, 0), 1.0, 1.0 if k % 4 == 1 else 0.0,
                                 0.15 if k % 4 == 1 else 0.6, 1.5, -1, -1, -1, -1, -1, -1))
        if m["kind"] == "mesh":
            t = place(m["tris"])
            if m["normals"] is None:
                n = np.cross(m["tris"][:, 1] - m["tris"][:, 0], m["tris"][:, 2] - m["tris"][:, 0])
                ln = np.linalg.norm(n, axis=1, keepdims=True)
                n = np.where(ln > 0, n / np.where(ln > 0, ln, 1.0), np.array([0.0, 1.0, 0.0]))
                n = np.repeat(n[:, None, :], 3, axis=1)
            else:
                n = m["normals"]
            rec = np.zeros((len(t), 3, 8))
            rec[:, :, :3], rec[:, :, 3:6] = t, n @ R.T
            rec[:, 1, 6], rec[:, 2, 7] = 1.0, 1.0
            out_models.append(pta.Model(pta.PT_MODEL_MESH, k, len(tris), len(t), (C.c_float * 3)(0, 0, 0), 0.0))
            tris += list(rec.reshape(-1, 24))
            if m["floor"]:
                floors[m["floor"]] = np.arange(prim, prim + len(t))
            prim += len(t)
        else:
            c = place(m["centre"])
            out_models.append(pta.Model(pta.PT_MODEL_SPHERE, k, 0, 0, (C.c_float * 3)(*[float(v) for v in c]), m["radius"] * scale))
            prim += 1
    assert prim <= MAX_PRIMS, (family, instance, prim)
    ext = extent * scale
    lights = [sb._light(pta, pta.PT_LIGHT_POINT, place(centre + extent * np.array([0.15, 0.9, 0.25])), 25.0 * ext * ext * np.array([1.0, 0.95, 0.9])),
              sb._light(pta, pta.PT_LIGHT_DIRECTIONAL, 3.0 * (R @ sb._unit([-0.3, -0.9, -0.25])), (0.9, 1.0, 1.1))]
    eye, target = place(centre + extent * np.array([0.35, 0.55, 0.8])), place(centre)
    f = sb._unit(target - eye)
    r = sb._unit(np.cross(f, [0.0, 1.0, 0.0]))
    u = np.cross(r, f)
    cols = [list(r) + [0.0], list(u) + [0.0], list(-f) + [0.0], list(eye) + [1.0]]
    camera = pta.Camera((C.c_float * 16)(*[v for col in cols for v in col]), 0.9, 1000.0 * ext, 1e-3 * ext)
    built = sb.BuiltScene(pta, np.array(tris, np.float32).reshape(-1, 24), out_models, mats, [], np.zeros(0, np.uint8), lights,
                          camera, BACKGROUND)
    built.n_prims = prim
    return built, floors


def primitives(built):
    """The primitives of a BuiltScene in primitive order, as float32 the way the description holds them: dict(is_sphere [n],
    tri [n, 3, 3] positions, nrm [n, 3, 3] vertex normals, centre [n, 3], radius [n]) - the rows of the other kind are 0."""
    d = built.desc.contents
    rec = np.ctypeslib.as_array(d.triangles, (int(d.n_triangles) * 24,)).reshape(-1, 3, 8)
    kinds, tri, nrm, centre, radius = [], [], [], [], []
    z33 = np.zeros((1, 3, 3), np.float32)
    for m in range(int(d.n_models)):
        mo = d.models[m]
        if mo.kind == 0:
            r = rec[mo.tri_first:mo.tri_first + mo.tri_count]
            kinds.append(np.zeros(len(r), bool))
            tri.append(r[:, :, :3])
            nrm.append(r[:, :, 3:6])
            centre.append(np.zeros((len(r), 3), np.float32))
            radius.append(np.zeros(len(r), np.float32))
        else:
            kinds.append(np.ones(1, bool))
            tri.append(z33)
            nrm.append(z33)
            centre.append(np.array([[mo.center[0], mo.center[1], mo.center[2]]], np.float32))
            radius.append(np.array([mo.radius], np.float32))
    return dict(is_sphere=np.concatenate(kinds), tri=np.concatenate(tri).astype(np.float32), nrm=np.concatenate(nrm).astype(np.float32),
                centre=np.concatenate(centre), radius=np.concatenate(radius))
