"""Scenes for the shading tests, built in Python straight into a pt_scene_desc (ctypes arrays): no loader and no PNG
between the float64 model (tests/shading_model.py) and the kernels.  `cases()` is the feature matrix of
tests/test_shading_model.py and tests/test_shading_matrix.py."""
import ctypes as C
from collections import namedtuple

import numpy as np

import __graft_entry__ as entry

TEX_SIZES = ((1, 1), (3, 5), (64, 64), (257, 129))   # (width, height)
TEX_KINDS = ("albedo", "emissive", "opacity", "metalness", "roughness", "normal")
TEX_CHANNELS = {"albedo": 3, "emissive": 3, "opacity": 1, "metalness": 1, "roughness": 1, "normal": 3}
MATERIALS = ("box", "floor", "wall", "panel", "ball", "sheet")
INF = float("inf")


class BuiltScene:
    """What pta.GpuScene, pta.Prep and oracle.OracleScene take (.desc), with the arrays kept alive."""

    def __init__(self, pta, tris, models, materials, textures, texels, lights, camera, background):
        d = pta.SceneDesc()
        t = np.ascontiguousarray(tris, np.float32).reshape(-1)
        self._tris = t
        self._texels = np.ascontiguousarray(texels, np.uint8)
        self._models, _ = pta._table(pta.Model, models, None)
        self._materials, _ = pta._table(pta.Material, materials, None)
        self._textures, _ = pta._table(pta.Texture, textures, None)
        self._lights, _ = pta._table(pta.Light, lights, None)
        d.n_models, d.n_materials, d.n_textures, d.n_lights = len(models), len(materials), len(textures), len(lights)
        d.n_triangles, d.n_texel_bytes = t.size // 24, self._texels.size
        d.models = C.cast(self._models, C.POINTER(pta.Model))
        d.materials = C.cast(self._materials, C.POINTER(pta.Material))
        d.textures = C.cast(self._textures, C.POINTER(pta.Texture))
        d.lights = C.cast(self._lights, C.POINTER(pta.Light))
        d.triangles = t.ctypes.data_as(C.POINTER(C.c_float))
        d.texels = self._texels.ctypes.data_as(C.POINTER(C.c_uint8))
        d.camera = camera
        d.background = (C.c_float * 3)(*background)
        self._desc = d
        self.desc = C.pointer(d)
        self.materials, self.lights, self.models = list(materials), list(lights), list(models)

    @property
    def translucent(self):
        """pt_scene_info.has_translucent: a model whose material has an opacity other than 1 or an opacity texture."""
        used = [self.materials[m.material] for m in self.models]
        return any(m.opacity != 1.0 or m.tex_opacity >= 0 for m in used)

    @property
    def n_triangles(self):
        return int(self._desc.n_triangles)

    @property
    def n_lights(self):
        return int(self._desc.n_lights)


# ---------------------------------------------------------------------------------------------------------------------
# textures: procedural, seeded; the two larger sizes hold every byte value in every channel
# ---------------------------------------------------------------------------------------------------------------------
def make_textures(pta, seed=7):
    """(list of pta.Texture, texel bytes, {(channels, size index): texture index})."""
    rng = np.random.default_rng(seed)
    tex, blobs, index, off = [], [], {}, 0
    for ch in (1, 3):
        for si, (w, h) in enumerate(TEX_SIZES):
            px = rng.integers(0, 256, size=(h * w, ch), dtype=np.uint8)
            if w * h >= 256:
                for c in range(ch):
                    px[rng.permutation(h * w)[:256], c] = rng.permutation(256).astype(np.uint8)
            index[(ch, si)] = len(tex)
            tex.append(pta.Texture(off, w, h, ch, 0))
            blobs.append(px.reshape(-1))
            off += px.size
    return tex, np.concatenate(blobs), index


# ---------------------------------------------------------------------------------------------------------------------
# geometry
# ---------------------------------------------------------------------------------------------------------------------
def _quad(p0, e1, e2, normals, uv0, du1, du2):
    """Two triangles p0, p0+e1, p0+e1+e2 / p0, p0+e1+e2, p0+e2 with per-corner normals and an affine UV map."""
    p0, e1, e2 = (np.asarray(v, np.float64) for v in (p0, e1, e2))
    uv0, du1, du2 = (np.asarray(v, np.float64) for v in (uv0, du1, du2))
    P = [p0, p0 + e1, p0 + e1 + e2, p0 + e2]
    T = [uv0, uv0 + du1, uv0 + du1 + du2, uv0 + du2]
    out = []
    for idx in ((0, 1, 2), (0, 2, 3)):
        out.append(np.concatenate([np.concatenate([P[i], normals[i], T[i]]) for i in idx]))
    return out


def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v)


def _panel():
    """The same triangle wound both ways side by side - one of the two is seen from its back; normals of length 0.5, 4 and 1."""
    a, b, c = np.array([-1.9, 0.1, 0.2]), np.array([-1.2, 0.15, -0.9]), np.array([-1.6, 1.4, -0.3])
    npn = [0.5 * _unit([1, 0.1, 0.6]), 4.0 * _unit([1, -0.1, 0.5]), _unit([0.9, 0.2, 0.7])]
    tp = [np.array([0.11, 0.07]), np.array([2.3, -0.4]), np.array([0.9, 1.8])]
    sh = np.array([0.0, 0.0, 1.25])
    return [np.concatenate([np.concatenate([p, n, t]) for p, n, t in zip((a, b, c), npn, tp)]),
            np.concatenate([np.concatenate([p + sh, n, t]) for p, n, t in zip((a, c, b), (npn[0], npn[2], npn[1]),
                                                                            (tp[0], tp[2], tp[1]))])]


def _terrace():
    """The groups of `terrace`: what the escape masks (csrc/pt_escape.h) can answer, next to what they cannot.
      floor  the ground y = 0 over [-2, 2] x [-2, 1.6] as 8 x 8 quads: small triangles, so that the origin set of most of them
             is clear of everything that rises above the plane; vertex normals of length 1, tilted by up to 2 degrees (the
             shaded origin sits 1e-5 x normal above the surface: inside [PT_ESC_H_LO, PT_ESC_H_HI])
      box    a convex box floating 0.9 above the ground, normals outward and exactly axial: a flat top whose neighbours fall away
      wall   a slab of 0.5 x 0.5 floating at y = 1.5 - high enough that neither the ground nor the box nor the ball counts as
             "near and below" (r_near = 2 x the origin set's radius), so nearly its whole upper hemisphere is clear - with vertex
             normals of length 1, 1, 4 and 0.5: where the interpolated normal is longer than the light grids' margin its paths
             go through the shadow queue under a live light, and are ended by the masks under none
      panel  the panel of `open`: vertex normals of length 0.5 and 4, standing on the ground - the ground triangles next to it
             are left unexamined, as are those under the ball (a sphere has no mask)"""
    g = {"floor": [], "box": []}
    nx, nz, dx, dz = 8, 8, 0.5, 0.45
    normal = lambda x, z: _unit([0.035 * np.sin(1.7 * x + 0.3), 1.0, 0.035 * np.cos(2.1 * z)])
    for i in range(nx):
        for j in range(nz):
            x, z = -2.0 + i * dx, 1.6 - j * dz
            n = [normal(x, z), normal(x + dx, z), normal(x + dx, z - dz), normal(x, z - dz)]
            uv0 = (-2.5 + 1.3 * (x + 2.0) + 0.23 * (1.6 - z), -2.5 + 0.2 * (x + 2.0) + 1.45 * (1.6 - z))
            g["floor"] += _quad((x, 0.0, z), (dx, 0, 0), (0, 0, -dz), n, uv0, (1.3 * dx, 0.2 * dx), (0.23 * dz, 1.45 * dz))
    lo, hi = np.array([-1.1, 0.9, -0.1]), np.array([-0.6, 1.3, 0.4])
    s = hi - lo
    for axis in range(3):
        a, b = (axis + 1) % 3, (axis + 2) % 3
        for side in (0, 1):
            p0 = lo.copy()
            e1, e2, n = np.zeros(3), np.zeros(3), np.zeros(3)
            e1[a], e2[b] = s[a], s[b]
            if side:
                p0[axis] = hi[axis]
            else:
                e1, e2 = e2, e1
            n[axis] = 1.0 if side else -1.0
            g["box"] += _quad(p0, e1, e2, [n] * 4, (0.03, 0.02), (0.9, 0.0), (0.0, 0.9))
    ns = [_unit([0.03, 1, 0.02]), _unit([-0.05, 1, 0.0]), 4.0 * _unit([0.0, 1, -0.04]), 0.5 * _unit([0.04, 1, 0.04])]
    g["wall"] = _quad((0.5, 1.5, 1.0), (0.5, 0, 0), (0, 0, -0.5), ns, (1.7, 0.13), (-2.3, 0.21), (0.17, 1.9))
    g["panel"] = _panel()
    return g


GEOMETRIES = ("full", "open", "boxed", "spheres", "room")   # room: the closed box and the ball
# not part of the matrix (cases()): the geometry whose escape masks prove misses (tests/test_masked_sequences.py)
MASKED_GEOMETRIES = ("terrace",)


def make_geometry(pta, geometry):
    """(triangles [n, 24], models): model k uses material k of MATERIALS (spheres-only: the ball alone, material 4)."""
    groups = _terrace() if geometry == "terrace" else {}
    if geometry in ("full", "boxed", "room"):   # a closed box around it all, normals inward
        lo, hi = np.array([-3.1, -0.4, -3.3]), np.array([3.2, 4.3, 3.4])
        s = hi - lo
        q = []
        for axis in range(3):
            a, b = (axis + 1) % 3, (axis + 2) % 3
            for side in (0, 1):
                p0 = lo.copy()
                e1, e2, n = np.zeros(3), np.zeros(3), np.zeros(3)
                e1[a], e2[b] = s[a], s[b]
                if side:
                    p0[axis] = hi[axis]
                    e1, e2 = e2, e1
                n[axis] = -1.0 if side else 1.0
                q += _quad(p0, e1, e2, [n] * 4, (0.03, 0.02), (0.9, 0.0), (0.0, 0.9))
        groups["box"] = q
    if geometry not in ("spheres", "room", "terrace"):
        # floor: vertex normals of length 0.5 and 4, not parallel; UVs scaled and rotated over [-2.5, 3.5]
        nf = [0.5 * _unit([0.05, 1, 0.02]), 4.0 * _unit([-0.04, 1, 0.03]), 0.5 * _unit([0.02, 1, -0.06]), 4.0 * _unit([0, 1, 0.05])]
        groups["floor"] = _quad((-2.0, 0.0, 1.5), (4.0, 0, 0), (0, 0, -3.5), nf, (-2.5, -2.5), (5.2, 0.8), (0.8, 5.2))
        # back wall: mirrored UVs (negative UV determinant)
        nw = [_unit([0.03, 0.02, 1]), _unit([-0.05, 0.0, 1]), 4.0 * _unit([0.0, -0.04, 1]), 0.5 * _unit([0.04, 0.04, 1])]
        groups["wall"] = _quad((-2.0, 0.0, -2.0), (4.0, 0, 0), (0, 2.5, 0), nw, (1.7, 0.13), (-2.3, 0.21), (0.17, 1.9))
        groups["panel"] = _panel()
    if geometry == "full":   # a translucent sheet between the lights and the rest
        ns = [_unit([0, -1, 0])] * 4
        groups["sheet"] = _quad((-2.5, 2.2, 2.0), (5.0, 0, 0), (0, 0, -4.5), ns, (0.02, 0.04), (1.3, 0.0), (0.0, 1.1))
    tris, models = [], []
    for k, name in enumerate(MATERIALS):
        if name == "ball":
            models.append(pta.Model(pta.PT_MODEL_SPHERE, k, 0, 0, (C.c_float * 3)(0.7, 0.55, -0.3), 0.5))
        elif name in groups:
            models.append(pta.Model(pta.PT_MODEL_MESH, k, len(tris), len(groups[name]), (C.c_float * 3)(0, 0, 0), 0.0))
            tris += groups[name]
    return np.array(tris, np.float32).reshape(-1, 24), models


def make_camera(pta, eye=(0.137, 1.371, 2.613), target=(0.02, 0.61, -0.52), fov=0.93):
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    f = _unit(target - eye)
    r = _unit(np.cross(f, [0.0, 1.0, 0.0]))
    u = np.cross(r, f)
    cols = [list(r) + [0.0], list(u) + [0.0], list(-f) + [0.0], list(eye) + [1.0]]
    return pta.Camera((C.c_float * 16)(*[v for col in cols for v in col]), fov, 100.0, 0.1)


# ---------------------------------------------------------------------------------------------------------------------
# lights
# ---------------------------------------------------------------------------------------------------------------------
def _light(pta, kind, vec, color):
    return pta.Light(kind, (C.c_float * 3)(*[float(v) for v in vec]), (C.c_float * 3)(*[float(v) for v in color]), 0.1)


LIGHT_SETS = ("none", "point", "dir_short", "dir_long", "point_dir", "five", "huge", "near")
# the ball's centre is (0.7, 0.55, -0.3); the floor is y = 0; the wall z = -2; the sheet y = 2.2
_FLOOR_SPOT = (0.31, 0.0, 0.42)


def make_lights(pta, name):
    P, D = pta.PT_LIGHT_POINT, pta.PT_LIGHT_DIRECTIONAL
    up = 0.1 * _unit([0.21, 0.95, 0.12])        # length 0.1, shining upwards: every floor it meets is unlit (moot)
    down = 10.0 * _unit([-0.3, -0.9, -0.25])    # length 10
    point = _light(pta, P, (0.4, 3.3, 0.9), (160.0, 150.0, 140.0))
    sets = {
        "none": [],
        "point": [point],
        "dir_short": [_light(pta, D, up, (2.0, 1.5, 1.0))],
        "dir_long": [_light(pta, D, down, (0.9, 1.0, 1.1))],
        "point_dir": [point, _light(pta, D, down, (0.5, 0.6, 0.7))],
        "five": [point, _light(pta, D, down, (0.6, 0.0, 0.8)),             # one zero component
                 _light(pta, P, (-1.0, 3.0, 0.2), (0.0, 0.0, 0.0)),         # colour 0
                 _light(pta, D, up, (1.0, 1.2, 0.8)),
                 _light(pta, P, (0.72, 0.5, -0.33), (3.0, 2.0, 1.0))],      # inside the sphere
        "huge": [_light(pta, P, (0.4, 3.3, 0.9), (9e29, 9e29, 9e29)), _light(pta, D, down, (1.1e30, 1.0, 1.0)),
                 _light(pta, P, (-1.2, 3.1, 0.3), (3e38, 3e38, 3e38)), _light(pta, D, _unit([0.2, -1, 0.1]), (INF, 1.0, INF)),
                 _light(pta, D, up, (0.5, 0.5, 0.5))],
        "near": [_light(pta, P, (_FLOOR_SPOT[0], 5e-4, _FLOOR_SPOT[2]), (1e-3, 1e-3, 2e-3)),
                 _light(pta, P, (-0.6, 2e-3, 0.7), (1e-3, 2e-3, 1e-3)),
                 _light(pta, P, (0.3, 1.1, -2.6), (40.0, 40.0, 40.0)),      # behind the (emissive) wall
                 _light(pta, D, up, (0.7, 0.7, 0.7))],
    }
    return sets[name]


# The 1e-3 guard of the kernels' skip (a point light nearer than that to the shaded point is cast even where its BRDF term is
# exactly 0): a camera of 2.8 mrad looks at one spot of the closed box's floor (y = -0.4, normals exactly (0, 1, 0)) and the
# light sits 5e-4 BELOW that spot, outside the box - n.l < 0 at every hit, so the term is 0 on both sides of 1e-3.
GUARD_SPOT = (0.31, -0.4, 0.42)
GUARD_FOV = 2.84e-3


def guard_scene(pta, with_near, with_other):
    """The `room` geometry under (optionally) a directional light and (optionally) the near light; the camera on the spot."""
    case = Case("near-guard", "room", "none", "none", "opaque", 0, "FILMIC", 0, True)
    lights = []
    if with_other:
        lights.append(_light(pta, pta.PT_LIGHT_DIRECTIONAL, 10.0 * _unit([-0.3, -0.9, -0.25]), (0.9, 1.0, 1.1)))
    if with_near:
        lights.append(_light(pta, pta.PT_LIGHT_POINT, (GUARD_SPOT[0], GUARD_SPOT[1] - 5e-4, GUARD_SPOT[2]), (1e-3, 1e-3, 2e-3)))
    return case, build(case, lights=lights, pta=pta, camera=make_camera(pta, target=GUARD_SPOT, fov=GUARD_FOV))


def tame_subset(pta, lights):
    """The lights the kernels may skip when their BRDF term is 0: every colour component finite and below 1e30."""
    return [l for l in lights if all(abs(c) < 1e30 for c in l.color)]


# ---------------------------------------------------------------------------------------------------------------------
# materials
# ---------------------------------------------------------------------------------------------------------------------
FACTOR_SETS = ("opaque", "mirror", "alpha", "edges", "glow", "black")


def _factors(name):
    """{material: (albedo, emissive, opacity, metalness, roughness)}."""
    base = {"box": ((0.7, 0.7, 0.75), (0, 0, 0), 1.0, 0.0, 1.0), "floor": ((0.8, 0.7, 0.6), (0, 0, 0), 1.0, 0.0, 0.05),
            "wall": ((0.9, 0.85, 0.3), (0, 0, 0), 1.0, 1.0, 1.0), "panel": ((0.3, 0.8, 0.4), (0, 0, 0), 1.0, 0.0, 1.0),
            "ball": ((1.0, 1.0, 1.0), (0, 0, 0), 1.0, 1.0, 0.0), "sheet": ((0.5, 0.6, 0.9), (0, 0, 0), 0.5, 0.0, 0.05)}
    m = {k: list(v) for k, v in base.items()}
    if name == "mirror":   # metal everywhere, brighter than physical (the Smith term alone costs a quarter per bounce and the
        for k in m:        # roulette follows the throughput): most paths keep going through a closed box
            m[k][0], m[k][3], m[k][4] = (2.0, 1.9, 1.8), 1.0, 0.05
        m["ball"][4], m["wall"][4], m["box"][4] = 0.0, 1.0, 0.2   # (box: a2 above the NDF's cancellation zone)
    elif name == "alpha":
        m["floor"][2], m["wall"][2], m["panel"][2], m["ball"][2], m["box"][2] = 0.5, 1.5, 0.0, 0.5, 1.0
    elif name == "edges":
        m["floor"][2], m["wall"][2], m["panel"][2], m["ball"][2] = 0.0011, 0.001, 0.5, 1.5
        m["floor"][4] = 0.0
    elif name == "glow":
        m["wall"][1], m["panel"][1], m["ball"][1] = (1e4, 1e4, 1e4), (0.5, 0.25, 1.0), (1e4, 0.0, 2.0)
    elif name == "black":
        m["floor"][0], m["ball"][0], m["wall"][0] = (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)
        m["floor"][4], m["box"][3] = 1.0, 1.0
    return m


def make_materials(pta, tex_index, tex_kind, factor_set, size_shift=0):
    """The material table: tex_kind is "none", "all" or one of TEX_KINDS (that kind alone).  Every material carries the
    textures, the ball's too: a sphere must ignore them (MaterialSample::simple)."""
    f = _factors(factor_set)
    out = []
    for k, name in enumerate(MATERIALS):
        albedo, emissive, opacity, metal, rough = f[name]
        if tex_kind in ("emissive", "all") and not any(emissive):
            emissive = (0.6, 0.5, 0.4)   # a texture scales the factor: without one it would stay dark
        idx = {}
        for j, kind in enumerate(TEX_KINDS):
            on = tex_kind == "all" or tex_kind == kind
            idx[kind] = tex_index[(TEX_CHANNELS[kind], (k + j + size_shift) % len(TEX_SIZES))] if on else -1
        out.append(pta.Material((C.c_float * 3)(*albedo), (C.c_float * 3)(*emissive), opacity, metal, rough, 1.5,
                                idx["albedo"], idx["emissive"], idx["opacity"], idx["metalness"], idx["roughness"],
                                idx["normal"]))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the matrix
# ---------------------------------------------------------------------------------------------------------------------
Case = namedtuple("Case", "name geometry tex_kind light_set factor_set bounces tonemap size_shift moot")
TEX_AXIS = ("none",) + TEX_KINDS + ("all",)
BOUNCES = (0, 1, 4, 8)
TONEMAPS = ("REINHARD", "FILMIC", "ACES")


def cases():
    """Every (texture kind, light set) pair once, the other axes cycled through them so that every value of every axis
    occurs; then the named scenes the pairs do not reach and the deep-bounce scenes in the closed box."""
    out, k = [], 0
    for ti, tk in enumerate(TEX_AXIS):
        for li, ls in enumerate(LIGHT_SETS):
            geometry = ("full", "open", "boxed")[k % 3]
            fs = FACTOR_SETS[(ti + 2 * li) % len(FACTOR_SETS)]
            if ls == "near" and tk in ("none", "albedo"):
                fs = "glow"    # a light behind an emissive surface
            moot = ls in ("dir_short", "five", "huge", "near") and fs not in ("glow",) and tk not in ("emissive", "all")
            out.append(Case(f"{tk}-{ls}", geometry, tk, ls, fs, BOUNCES[(ti + li) % 4], TONEMAPS[k % 3], k, moot))
            k += 1
    out.append(Case("spheres-dir", "spheres", "none", "dir_long", "opaque", 1, "ACES", 0, False))
    out.append(Case("spheres-none", "spheres", "all", "none", "glow", 4, "REINHARD", 1, False))
    out.append(Case("opaque-but-opacity-texture", "boxed", "opacity", "point", "opaque", 4, "FILMIC", 2, False))
    for b in (1, 4, 8):   # the closed metal box: most paths are alive at the last bounce
        out.append(Case(f"deep-{b}", "room", "none", "point_dir", "mirror", b, TONEMAPS[b % 3], 3, False))
    # (a random normal map turns half of the normals below the horizon and ends most paths at once: depth 1 is what it reaches)
    out.append(Case("mirror-box-normal", "boxed", "normal", "point", "mirror", 1, "ACES", 1, False))
    return out


def case_by_name(name):
    return next(c for c in cases() if c.name == name)


_TEX = {}


def build(case, lights=None, materials=None, pta=None, camera=None):
    """The BuiltScene of a case (lights / materials / camera: what replaces the case's own)."""
    pta = pta or entry.load_package()
    if "t" not in _TEX:
        _TEX["t"] = make_textures(pta)
    tex, texels, tex_index = _TEX["t"]
    tris, models = make_geometry(pta, case.geometry)
    mats = materials if materials is not None else make_materials(pta, tex_index, case.tex_kind, case.factor_set, case.size_shift)
    lts = lights if lights is not None else make_lights(pta, case.light_set)
    bg = (0.25, 0.3, 0.45)
    return BuiltScene(pta, tris, models, mats, tex, texels, lts, camera or make_camera(pta), bg)


def case_materials(case, pta=None):
    pta = pta or entry.load_package()
    if "t" not in _TEX:
        _TEX["t"] = make_textures(pta)
    return make_materials(pta, _TEX["t"][2], case.tex_kind, case.factor_set, case.size_shift)


def profile(case, width, height, samples=1, bounces=None, tonemap=None, pta=None):
    pta = pta or entry.load_package()
    return pta.Profile.make(width, height, samples, case.bounces if bounces is None else bounces, tonemap or case.tonemap)
