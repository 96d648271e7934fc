"""The shading half of the reference renderer, restated in float64 from the Rust source alone
(src/renderer/{mod,hit,material_sample,tonemap,utils}.rs, src/renderer/brdf/{mod,cook_torrance}.rs,
src/scene/internal/{material,camera,model}.rs) - a second reading, independent of oracle/pt_oracle.cpp and of csrc/.

From the project it takes only what has anchors of its own: the sorted hit list of an f32 ray
(OracleScene(desc, PTO_BRUTE_FORCE).trace_all), the words of the random generator (oracle.rng_words) and the
pt_scene_desc itself.  Everything else is computed here, in Python floats (IEEE double).

Steered paths: the model predicts every ray ray_cast is called with, compares it with the ray the f32 pipeline really cast
(OracleScene.path_rays) and then goes on FROM THE f32 RAY, so that rounding differences do not add up along a path.  A path
reports its radiance, its largest ray disagreement and whether a discrete decision was too close to call (fragile).
"""
import math

import numpy as np

F32 = np.float32
PI = float(F32(math.pi))               # std::f32::consts::PI
NORMAL_BIAS = float(F32(0.00001))      # mod.rs:58
ROUGH_MIN = float(F32(0.0001))         # material_sample.rs:23,34
OPACITY_MIN = float(F32(0.001))        # mod.rs:201
THROUGHPUT_MIN = float(F32(0.00001))   # mod.rs:219
SPEC_DENOM_MIN = float(F32(0.0001))    # cook_torrance.rs:50
INV_GAMMA = float(F32(1.0) / F32(2.2))  # mod.rs:340-344
FLT_MAX = float(np.finfo(np.float32).max)
NAN, INF = float("nan"), float("inf")
TEXEL_EDGE = 1e-4
CLOSE = 1e-6
GGX_CANCEL = 1e-3      # eval_direct: |1 - ndh^2 (1 - a2)| below this: f32 keeps fewer than four digits of the NDF
SAMPLE_CANCEL = 1e-3   # the GGX sample: f32 moves theta by more than this (the mirror direction moves by twice that)


def f32_normalize(d):
    """cgmath's normalize of an f32 vector IN f32 (self * (1 / sqrt(x*x + y*y + z*z)), left to right), exactly.  The one
    place where the model emulates f32: a sample reflected onto -v (see ShadingModel.path)."""
    x, y, z = (F32(v) for v in d)
    with np.errstate(all="ignore"):
        s = F32(1.0) / np.sqrt(F32(F32(x * x) + F32(y * y)) + F32(z * z))
        return (float(F32(x * s)), float(F32(y * s)), float(F32(z * s)))


# ---- scalar helpers with the semantics of Rust's f32 methods ---------------------------------------------------------
def fmax(a, b):
    """f32::max: the other operand if one is NaN."""
    if a != a:
        return b
    if b != b:
        return a
    return a if a > b else b


def div(a, b):
    if b == 0.0:
        if a != a or a == 0.0:
            return NAN
        return math.copysign(INF, a) * math.copysign(1.0, b)
    if math.isinf(a) and math.isinf(b):
        return NAN
    return a / b


def sqrt(x):
    return math.sqrt(x) if x >= 0.0 else (NAN if x == x else NAN)


def acos(x):
    return math.acos(x) if -1.0 <= x <= 1.0 else NAN


def sin(x):
    return math.sin(x) if math.isfinite(x) else NAN


def cos(x):
    return math.cos(x) if math.isfinite(x) else NAN


def ovf(x):
    """The value as an f32 would hold it where that matters: beyond FLT_MAX it is infinite."""
    if x > FLT_MAX:
        return INF
    if x < -FLT_MAX:
        return -INF
    return x


def add(a, b):
    return (a[0] + b[0], a[1] + b[1], a[2] + b[2])


def sub(a, b):
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


def scale(a, s):
    return (a[0] * s, a[1] * s, a[2] * s)


def mul(a, b):
    return (a[0] * b[0], a[1] * b[1], a[2] * b[2])


def dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def length(a):
    return sqrt(dot(a, a))


def normalize(a):
    n = length(a)
    return (div(a[0], n), div(a[1], n), div(a[2], n))


def finite3(a):
    return all(math.isfinite(v) for v in a)


def gen_f32(word):
    """rand 0.8 Standard for f32: the top 24 bits of a word, scaled by 2^-24."""
    return (int(word) >> 8) * (1.0 / 16777216.0)


class Draws:
    def __init__(self, words):
        self.words, self.n = words, 0

    def next(self):
        v = gen_f32(self.words[self.n])
        self.n += 1
        return v


class PathResult:
    __slots__ = ("radiance", "ray_error", "fragile", "n_rays", "alive_at_last", "draws")

    def __init__(self):
        self.radiance, self.ray_error, self.fragile, self.n_rays, self.alive_at_last, self.draws = None, 0.0, None, 0, False, 0

    def flag(self, reason):
        if self.fragile is None:
            self.fragile = reason


class ShadingModel:
    def __init__(self, desc, oracle_scene, oracle, max_hits=48):
        d = desc.contents if hasattr(desc, "contents") else desc
        self.scene, self.oracle, self.max_hits = oracle_scene, oracle, max_hits
        nt = int(d.n_triangles)
        self.tris = (np.ctypeslib.as_array(d.triangles, (nt * 24,)).astype(np.float64).reshape(nt, 3, 8) if nt else
                     np.zeros((0, 3, 8)))
        self.tri_list = self.tris.tolist()
        self.texels = np.ctypeslib.as_array(d.texels, (int(d.n_texel_bytes),)).copy() if d.n_texel_bytes else np.zeros(0, np.uint8)
        self.textures = [(int(t.offset), int(t.width), int(t.height), int(t.channels)) for t in (d.textures[i] for i in range(d.n_textures))]
        self.materials = []
        for i in range(d.n_materials):
            m = d.materials[i]
            self.materials.append(dict(albedo=tuple(float(v) for v in m.albedo), emissive=tuple(float(v) for v in m.emissive),
                                       opacity=float(m.opacity), metalness=float(m.metalness), roughness=float(m.roughness),
                                       tex=dict(albedo=m.tex_albedo, emissive=m.tex_emissive, opacity=m.tex_opacity,
                                                metalness=m.tex_metalness, roughness=m.tex_roughness, normal=m.tex_normal)))
        self.models, self.prim_model, self.prim_tri = [], [], []
        for i in range(d.n_models):
            m = d.models[i]
            sphere = m.kind == 1
            self.models.append(dict(sphere=sphere, material=self.materials[m.material], center=tuple(float(v) for v in m.center),
                                    radius=float(m.radius)))
            if sphere:
                self.prim_model.append(i)
                self.prim_tri.append(-1)
            else:
                for t in range(m.tri_count):
                    self.prim_model.append(i)
                    self.prim_tri.append(m.tri_first + t)
        self.lights = [(int(l.kind), tuple(float(v) for v in l.vec), tuple(float(v) for v in l.color))
                       for l in (d.lights[i] for i in range(d.n_lights))]
        t = [float(v) for v in d.camera.transform]
        self.cam_cols = [tuple(t[4 * k:4 * k + 3]) for k in range(4)]
        self.fov = float(d.camera.fov)
        self.background = tuple(float(v) for v in d.background)

    # ---- camera (mod.rs:107-124) -------------------------------------------------------------------------------------
    def camera_ray(self, profile, pixel, draws):
        w, h = profile.width, profile.height
        x, y = pixel % w, pixel // w
        tan_half = math.tan(self.fov / 2.0)
        sx = ((x + draws.next()) / w * 2.0 - 1.0) * (tan_half * (w / h))   # mod.rs:114-116
        sy = (1.0 - (y + draws.next()) / h * 2.0) * tan_half              # mod.rs:118-120
        dcam = normalize((sx, sy, -1.0))                                   # mod.rs:122
        c = self.cam_cols                                                  # camera.rs:36-39: w = 0, the translation drops out
        d = tuple(c[0][k] * dcam[0] + c[1][k] * dcam[1] + c[2][k] * dcam[2] for k in range(3))
        return c[3], d                                                     # camera.rs:42-48

    # ---- hits (hit.rs:100-137, model.rs:26-63) ----------------------------------------------------------------------
    def hits_of(self, ray, records):
        o, d = ray
        out = []
        for rec in records:
            prim, flags, dist = int(rec["prim"]), int(rec["flags"]), float(rec["dist"])
            model = self.models[self.prim_model[prim]]
            if flags & 2:   # sphere: the entry hit's normal points outwards, the exit hit's inwards (model.rs:43-61)
                t = div(dist, length(d))   # dist is |hit_point - origin| (model.rs:46,58)
                pos = add(o, scale(d, t))
                n = normalize(sub(pos, model["center"]))
                if flags & 4:
                    n = scale(n, -1.0)
                out.append(dict(sphere=True, model=model, pos=pos, normal=n, dist=dist))
                continue
            v0, v1, v2 = self.tri_list[self.prim_tri[prim]]
            u, v = float(rec["u"]), float(rec["v"])
            w0 = 1.0 - u - v
            normal = tuple(w0 * v0[3 + k] + u * v1[3 + k] + v * v2[3 + k] for k in range(3))               # hit.rs:108-110
            duv1, duv2 = (v1[6] - v0[6], v1[7] - v0[7]), (v2[6] - v0[6], v2[7] - v0[7])
            uv = (v0[6] + u * duv1[0] + v * duv2[0], v0[7] + u * duv1[1] + v * duv2[1])                    # hit.rs:111-113
            e1, e2 = tuple(v1[k] - v0[k] for k in range(3)), tuple(v2[k] - v0[k] for k in range(3))
            f = div(1.0, duv1[0] * duv2[1] - duv2[0] * duv1[1])                                             # hit.rs:121
            tangent = normalize(tuple(f * (duv2[1] * e1[k] - duv1[1] * e2[k]) for k in range(3)))           # hit.rs:122-127
            pos = add(o, scale(d, dist))                                                                    # triangle.rs:77
            out.append(dict(sphere=False, model=model, pos=pos, normal=normal, uv=uv, tangent=tangent, back=bool(flags & 1),
                            dist=dist))
        return out

    # ---- textures and materials (material.rs:115-218, material_sample.rs) -----------------------------------------
    def get_pixel(self, tex, uv, res):
        off, w, h, ch = self.textures[tex]
        cx, cy = uv[0] * w, uv[1] * h                          # material.rs:121-124
        for c in (cx, cy):
            if not math.isfinite(c) or abs(c - round(c)) < TEXEL_EDGE:
                res.flag("texel border")
        ix = int(cx) if math.isfinite(cx) else 0               # `as i64` truncates toward zero (NaN -> 0)
        iy = int(cy) if math.isfinite(cy) else 0
        x, y = ix % w, iy % h                                  # rem_euclid; Python's % of a positive modulus is the same
        p = off + (y * w + x) * ch
        return self.texels[p:p + ch]

    def material_sample(self, material, hit, res):
        """hit decides between MaterialSample::simple and ::new and gives the uv (hit.rs:84-91)."""
        m, t = material, material["tex"]
        if hit["sphere"]:
            albedo, emissive, opacity, metal, rough = m["albedo"], m["emissive"], m["opacity"], m["metalness"], m["roughness"]
        else:
            uv = hit["uv"]
            albedo, emissive, opacity, metal, rough = m["albedo"], m["emissive"], m["opacity"], m["metalness"], m["roughness"]
            if t["albedo"] >= 0:      # sRGB -> linear on the albedo only (material.rs:137-142)
                p = self.get_pixel(t["albedo"], uv, res)
                albedo = tuple(math.pow(float(p[k]) / 255.0, float(F32(2.2))) * albedo[k] for k in range(3))
            if t["emissive"] >= 0:    # material.rs:189-197
                p = self.get_pixel(t["emissive"], uv, res)
                emissive = tuple(float(p[k]) / 255.0 * emissive[k] for k in range(3))
            if t["opacity"] >= 0:     # material.rs:207-211
                opacity = float(self.get_pixel(t["opacity"], uv, res)[0]) / 255.0 * opacity
            if t["metalness"] >= 0:   # material.rs:152-156
                metal = float(self.get_pixel(t["metalness"], uv, res)[0]) / 255.0 * metal
            if t["roughness"] >= 0:   # material.rs:165-169
                rough = float(self.get_pixel(t["roughness"], uv, res)[0]) / 255.0 * rough
        return dict(albedo=albedo, emissive=emissive, opacity=opacity, metalness=metal, roughness=fmax(rough, ROUGH_MIN))

    def shading_normal(self, hit, res):
        """hit.rs:55-82."""
        if hit["sphere"]:
            return hit["normal"]
        n = hit["normal"]
        tex = hit["model"]["material"]["tex"]["normal"]
        if tex >= 0:
            p = self.get_pixel(tex, hit["uv"], res)
            nm = tuple(float(p[k]) / 127.5 - 1.0 for k in range(3))                    # material.rs:181-185
            tg = hit["tangent"]
            bt = cross(n, tg)                                                           # hit.rs:66
            n = normalize(add(add(scale(tg, nm[0]), scale(bt, nm[1])), scale(n, nm[2])))  # hit.rs:67-68
        return scale(n, -1.0) if hit["back"] else n                                      # hit.rs:74-78

    # ---- Cook-Torrance (cook_torrance.rs) -------------------------------------------------------------------------
    @staticmethod
    def f0_of(ms):
        m = ms["metalness"]
        return tuple(0.04 * (1.0 - m) + ms["albedo"][k] * m for k in range(3))   # cook_torrance.rs:180-182

    @staticmethod
    def fresnel(f0, cos_theta):
        p = (1.0 - cos_theta) ** 5
        return tuple(f0[k] + (1.0 - f0[k]) * p for k in range(3))                # cook_torrance.rs:143-147

    @staticmethod
    def geometry_smith(rough, n, v, l):
        k = (rough + 1.0) ** 2 / 8.0                                            # cook_torrance.rs:161
        ndv, ndl = fmax(dot(n, v), 0.0), fmax(dot(n, l), 0.0)
        return div(ndv, ndv * (1.0 - k) + k) * div(ndl, ndl * (1.0 - k) + k)    # cook_torrance.rs:149-164

    @staticmethod
    def diffuse(ms, ks, n, l):
        c = fmax(dot(n, l), 0.0)                                                 # cook_torrance.rs:113-116
        return tuple((1.0 - ks[k]) * (1.0 - ms["metalness"]) * ms["albedo"][k] / PI * c for k in range(3))

    def eval_direct(self, ms, n, v, l, res):
        h = normalize(add(v, l))                                                 # cook_torrance.rs:40
        a = ms["roughness"] * ms["roughness"]
        a2 = a * a
        ndh = fmax(dot(n, h), 0.0)
        den = ndh * ndh * (a2 - 1.0) + 1.0
        if abs(den) < GGX_CANCEL * fmax(1.0, ndh * ndh):
            res.flag("GGX denominator cancels")   # 1 - ndh^2 (1 - a2) next to 0: f32 keeps few digits of it
        d = div(a2, PI * den * den)                                              # cook_torrance.rs:167-177
        f = self.fresnel(self.f0_of(ms), fmax(dot(h, v), 0.0))
        g = self.geometry_smith(ms["roughness"], n, v, l)
        ndl = fmax(dot(n, l), 0.0)
        denom = fmax(4.0 * fmax(dot(n, v), 0.0) * ndl, SPEC_DENOM_MIN)           # cook_torrance.rs:47-50
        dif = self.diffuse(ms, f, n, l)
        return tuple(dif[k] + div(d * f[k] * g, denom) * ndl + ms["emissive"][k] for k in range(3))   # :57: + emissive

    def microfacet(self, ms, n, draws, res):
        a = ms["roughness"] * ms["roughness"]
        a2 = a * a
        r1, r2 = draws.next(), draws.next()                                      # cook_torrance.rs:123-124
        den = r1 * (a2 - 1.0) + 1.0
        theta = acos(sqrt(div(1.0 - r1, den)))                                   # :128
        # Next to r1 = 1 with a small a2 the denominator cancels down to a2, of which f32 keeps few digits or none
        # (a2 < 3e-8: a2 - 1 is -1 and theta is 0 whatever r1).  How far that moves theta is found by doing the four
        # operations in f32 as well - only to flag the sample, never for its value.
        with np.errstate(all="ignore"):
            a32 = F32(ms["roughness"]) * F32(ms["roughness"])
            ratio32 = float((F32(1.0) - F32(r1)) / (F32(r1) * (a32 * a32 - F32(1.0)) + F32(1.0)))
        if not abs(acos(sqrt(ratio32)) - theta) < SAMPLE_CANCEL:
            res.flag("GGX sample denominator cancels")
        phi = 2.0 * PI * r2                                                      # :130
        st = sin(theta)
        local = normalize((st * cos(phi), cos(theta), st * sin(phi)))            # :133-137
        if abs(abs(n[0]) - abs(n[1])) < CLOSE * length(n) and not (n[0] == 0.0 and n[1] == 0.0):   # (0 = 0 is exact in f32 too)
            res.flag("|n.x| next to |n.y| in transform_to_world")
        return normalize(self.transform_to_world(local, n))                      # :139-140

    @staticmethod
    def transform_to_world(vec, n):
        """brdf/mod.rs:35-48."""
        if abs(n[0]) > abs(n[1]):
            s = sqrt(n[0] * n[0] + n[2] * n[2])
            nt = (div(n[2], s), div(0.0, s), div(-n[0], s))
        else:
            s = sqrt(n[1] * n[1] + n[2] * n[2])
            nt = (div(0.0, s), div(-n[2], s), div(n[1], s))
        nb = cross(n, nt)
        return tuple(vec[0] * nb[k] + vec[1] * n[k] + vec[2] * nt[k] for k in range(3))

    def eval_indirect(self, ms, n, v, l, wm, res):
        h = normalize(add(v, l))                                                 # cook_torrance.rs:66
        f = self.fresnel(self.f0_of(ms), fmax(dot(h, v), 0.0))
        g = self.geometry_smith(ms["roughness"], n, v, l)
        ndl = dot(n, l)
        if abs(ndl) < CLOSE * (length(n) + 1e-300):
            res.flag("n.l next to 0")
        if ndl > 0.0:                                                            # :71-80
            weight = div(abs(dot(v, wm)), abs(dot(v, n)) * abs(dot(wm, n)))
            spec = tuple(f[k] * g * weight for k in range(3))
        else:
            spec = (0.0, 0.0, 0.0)
        dif = self.diffuse(ms, f, n, l)
        return tuple(dif[k] + spec[k] for k in range(3))

    # ---- lights (mod.rs:281-333) ----------------------------------------------------------------------------------
    def shadow_ray(self, light, hit, res):
        kind, vec, _ = light
        origin = add(hit["pos"], scale(hit["normal"], NORMAL_BIAS))              # mod.rs:284-285, 310-311: the unflipped hit normal
        if kind == 1:
            return origin, scale(vec, -1.0), vec, None                           # the direction as given, not normalised
        dvec = sub(hit["pos"], vec)                                              # mod.rs:306-308
        dist = length(dvec)
        if dist <= 1e-6 * fmax(1.0, length(vec)):
            res.flag("point light at the hit point")   # f32 rounds the hit to the light itself: 0 / 0
        direction = normalize(dvec)
        return origin, scale(direction, -1.0), direction, dist

    def light_radiance(self, light, hit, direction_dist, shadow_hits, res):
        kind, vec, color = light
        if kind == 1:
            c = color
            for sh in shadow_hits:                                               # mod.rs:291-297: the occluder's own sample
                op = self.material_sample(sh["model"]["material"], sh, res)["opacity"]
                c = scale(c, 1.0 - op)
                if c[0] + c[1] + c[2] == 0.0:
                    break
            return c
        dist = direction_dist
        diss = 4.0 * PI * dist * dist                                            # mod.rs:315
        c = tuple(ovf(div(color[k], diss)) for k in range(3))                    # mod.rs:318
        for sh in shadow_hits:
            gap = length(sub(sh["pos"], hit["pos"]))                             # mod.rs:320
            if abs(gap - dist) <= 1e-5 * dist:
                res.flag("occluder at the light's distance")
            if gap > dist:
                break
            # mod.rs:324: the OCCLUDER's material, sampled at the SHADED hit's kind and uv
            op = self.material_sample(sh["model"]["material"], hit, res)["opacity"]
            c = scale(c, 1.0 - op)
            if c[0] + c[1] + c[2] == 0.0:
                break
        return c

    # ---- one path (mod.rs:172-278) --------------------------------------------------------------------------------
    def path(self, profile, pixel, f32_rays=None, hit_records=None, n_words=256):
        """The radiance of sample 1 of `pixel` for a profile with samples == 1.  f32_rays: OracleScene.path_rays of it
        (fetched when None); hit_records: per f32 ray the (records, count) of trace_all (traced when None)."""
        res = PathResult()
        if f32_rays is None:
            f32_rays = self.scene.path_rays(profile, pixel, 1)
        seed = 1 + pixel * profile.samples                                       # mod.rs:110-112
        draws = Draws(self.oracle.rng_words(np.array([seed], np.uint64), n_words)[0])
        cursor = [0]

        def cast(origin, direction):
            """ray_cast: compare the predicted ray with the f32 one, go on from the f32 one."""
            k = cursor[0]
            cursor[0] += 1
            if k >= len(f32_rays):
                res.flag("more rays than the f32 path")
                return None, None
            r = [float(v) for v in f32_rays[k]]
            fo, fd = tuple(r[:3]), tuple(r[3:])
            if finite3(origin) and finite3(direction) and finite3(fo) and finite3(fd):
                eo = max(abs(a - b) for a, b in zip(origin, fo)) / max(1.0, max(abs(v) for v in fo))
                ed = max(abs(a - b) for a, b in zip(direction, fd)) / max(1.0, max(abs(v) for v in fd))
                res.ray_error = max(res.ray_error, eo, ed)
            else:
                same = all((a != a and b != b) or a == b for a, b in zip(origin + direction, fo + fd))
                if not same:
                    res.ray_error = INF
            if hit_records is not None:
                recs, n = hit_records[k]
            else:
                recs, n = self.scene.trace_all(np.array(r, np.float32), self.max_hits)
                recs, n = recs[0], int(n[0])
            if n >= self.max_hits:
                res.flag("hit list truncated")
            return (fo, fd), self.hits_of((fo, fd), recs[:n])

        color, thr = (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)
        ray_o, ray_d = self.camera_ray(profile, pixel, draws)
        bounces = profile.bounces
        for bounce in range(bounces + 1):
            ray, hits = cast(ray_o, ray_d)
            if ray is None:
                break
            if not hits:
                color = add(color, mul(thr, self.background))                    # mod.rs:184-186
                break
            surf = None
            for hit in hits:                                                     # mod.rs:189-205
                ms = self.material_sample(hit["model"]["material"], hit, res)
                n = self.shading_normal(hit, res)
                surf = (hit, ms, n)
                op = ms["opacity"]
                if hit["model"]["material"]["tex"]["opacity"] >= 0 and not hit["sphere"] and (abs(op - 1.0) < CLOSE or abs(op - OPACITY_MIN) < CLOSE * OPACITY_MIN):
                    res.flag("opacity at a threshold")
                if op >= 1.0:
                    break
                if op > OPACITY_MIN:
                    r = draws.next()
                    if abs(r - op) < CLOSE:
                        res.flag("alpha draw next to the opacity")
                    if r < op:
                        break
            hit, ms, n = surf
            if bounce == bounces:
                res.alive_at_last = True
            view = scale(ray[1], -1.0)                                           # mod.rs:207
            color = add(color, mul(thr, ms["emissive"]))                         # mod.rs:245
            for light in self.lights:                                            # mod.rs:248-262
                so, sd, ldir, dist = self.shadow_ray(light, hit, res)
                sray, shits = cast(so, sd)
                if sray is None:
                    break
                rad = self.light_radiance(light, hit, dist, shits, res)
                if rad[0] == 0.0 and rad[1] == 0.0 and rad[2] == 0.0:
                    continue
                b = self.eval_direct(ms, n, view, scale(ldir, -1.0), res)
                color = tuple(ovf(color[k] + ovf(ovf(thr[k] * b[k]) * rad[k])) for k in range(3))
            if bounce < bounces:                                                 # mod.rs:265-275
                wm = self.microfacet(ms, n, draws, res)
                vm = dot(view, wm)
                if abs(vm) < CLOSE:
                    res.flag("v.m next to 0")
                if vm > 0.0:
                    ray_d = normalize(sub(scale(wm, 2.0 * vm), view))             # utils.rs:34-36, cook_torrance.rs:30-31
                else:
                    # max(v.m, 0) = 0: the reflection is -v, the f32 ray direction itself, and what eval_indirect sees as
                    # its halfway vector is the rounding of normalize(-v) against v - zero (NaN: Fresnel 1, the path
                    # dies) or a few ulps.  No float64 value stands for that, so this one normalize is done in f32.
                    ray_d = f32_normalize(ray[1])
                ray_o = add(hit["pos"], scale(hit["normal"], NORMAL_BIAS))
                # (the throughput is judged on the direction the f32 path really took: peek at the next f32 ray)
                k = cursor[0]
                ldir = tuple(float(v) for v in f32_rays[k][3:]) if k < len(f32_rays) else ray_d
                thr = mul(thr, self.eval_indirect(ms, n, view, ldir, wm, res))    # pdf() == 1
            m2 = dot(thr, thr)
            if abs(m2 - THROUGHPUT_MIN) < 1e-5 * THROUGHPUT_MIN:
                res.flag("throughput at its cut")
            if m2 < THROUGHPUT_MIN:                                              # mod.rs:219-221
                break
            if bounce > 3:                                                       # mod.rs:223-225, utils.rs:23-31
                p = fmax(fmax(thr[0], thr[1]), thr[2])
                thr = scale(thr, div(1.0, p))
                r = draws.next()
                if abs(r - p) < CLOSE:
                    res.flag("roulette draw next to its probability")
                if r > p:
                    break
        if cursor[0] != len(f32_rays):
            res.flag("ray sequences differ in length")
        res.radiance, res.n_rays, res.draws = color, cursor[0], draws.n
        return res

    def image(self, profile, pixels=None):
        """Every pixel's PathResult; the f32 rays are fetched per pixel and traced in one batch."""
        assert profile.samples == 1
        pixels = range(profile.width * profile.height) if pixels is None else pixels
        rays = [self.scene.path_rays(profile, p, 1) for p in pixels]
        flat = np.concatenate(rays) if rays else np.zeros((0, 6), np.float32)
        ok = np.isfinite(flat).all(axis=1)
        recs, counts = self.scene.trace_all(np.where(ok[:, None], flat, 0).astype(np.float32), self.max_hits)
        counts = np.where(ok, counts, 0)
        out, at = [], 0
        for p, r in zip(pixels, rays):
            hr = [(recs[at + k], int(counts[at + k])) for k in range(len(r))]
            at += len(r)
            out.append(self.path(profile, p, r, hr))
        return out, rays


# ---- post-processing (mod.rs:335-353, tonemap.rs) -------------------------------------------------------------------
def tonemap(op, c):
    if op == 0:     # tonemap.rs:23-25
        return div(c, ovf(c + 1.0))
    if op == 1:     # tonemap.rs:27-38
        c = fmax(c - float(F32(0.004)), 0.0)
        num = ovf(c * ovf(ovf(float(F32(6.2)) * c) + 0.5))
        den = ovf(ovf(c * ovf(ovf(float(F32(6.2)) * c) + float(F32(1.7)))) + float(F32(0.06)))
        return div(num, den)
    a, b, cc, d, e = (float(F32(v)) for v in (2.51, 0.03, 2.43, 0.59, 0.14))   # tonemap.rs:40-54
    num = ovf(c * ovf(ovf(a * c) + b))
    den = ovf(ovf(c * ovf(ovf(cc * c) + d)) + e)
    r = div(num, den)
    if r != r:
        return r    # f32::clamp keeps NaN
    return min(max(r, 0.0), 1.0)


def post_value(op, radiance):
    """The value `as u8` is applied to."""
    t = tonemap(op, radiance)
    if t == -INF:
        g = INF            # powf(-inf, y) is +inf for a positive y that is no odd integer (Reinhard at -1: -1 / 0)
    elif t != t or t < 0.0:
        g = NAN            # powf of a finite negative base with a fractional exponent
    elif t == 0.0:
        g = 0.0
    elif math.isinf(t):
        g = INF
    else:
        g = math.pow(t, INV_GAMMA)
    return g * 255.0


def as_u8(x):
    """Rust's float -> u8 cast: NaN -> 0, saturating, truncating."""
    if x != x:
        return 0
    if x <= 0.0:
        return 0
    if x >= 255.0:
        return 255
    return int(x)


def post_process(op, samples, accum):
    """(u8 [n, 3], near [n, 3] bool: the value before the cast is within 1e-4 of an integer)."""
    accum = np.asarray(accum, np.float64).reshape(-1, 3)
    out, near = np.zeros(accum.shape, np.uint8), np.zeros(accum.shape, bool)
    for i in range(accum.shape[0]):
        for k in range(3):
            x = post_value(op, div(float(accum[i, k]), float(samples)))
            out[i, k] = as_u8(x)
            near[i, k] = math.isfinite(x) and abs(x - round(x)) < 1e-4
    return out, near


# ---- comparing a rendered accumulator with the model ---------------------------------------------------------------------
DIRECT_SIZE = (64, 48)    # the direct tier: every case at bounces 0
PATH_SIZE = (64, 48)      # the whole-path tiers: the cases of bounces 1 / 4 / 8 (scalar Python per path)
ATOL_SHARE = 1e-7         # atol = this share of the case's largest finite radiance
RTOL_FACTOR = 4.0         # rtol = this factor x the recorded largest deviation of the tier
DIRECT_CEILING, RAY_CEILING = 1e-3, 5e-3
FRAGILE_CAP = {"direct": 0.01, "paths": 0.02}


def tier_of(bounces):
    return "direct" if bounces == 0 else f"paths{bounces}"


def compare(accum, results):
    """accum [n, 3] (one sample per pixel) against the model's PathResults.  Returns (excess [n, 3], atol, kind_mismatch,
    fragile [n]): excess = (|a - m| - atol)+ / |m| per finite pixel and channel, 0 where both are non-finite of the same kind
    and on fragile pixels; kind_mismatch counts the channels of non-fragile pixels whose kinds differ (NaN, +inf, -inf)."""
    a = np.asarray(accum, np.float64).reshape(-1, 3)
    m = np.array([r.radiance for r in results], np.float64).reshape(-1, 3)
    fragile = np.array([r.fragile is not None for r in results], bool)
    fin = np.isfinite(m)
    atol = ATOL_SHARE * (np.abs(m[fin]).max() if fin.any() else 0.0)
    both = fin & np.isfinite(a)
    with np.errstate(all="ignore"):
        over = np.maximum(np.abs(a - m) - atol, 0.0)
        excess = np.where(over > 0, over / np.abs(m), 0.0)
    excess = np.where(both, excess, 0.0)
    same_kind = both | (np.isnan(a) & np.isnan(m)) | (np.isinf(a) & np.isinf(m) & (np.sign(a) == np.sign(m)))
    kind_mismatch = int((~same_kind & ~fragile[:, None]).sum())
    excess[fragile] = 0.0
    return excess, atol, kind_mismatch, fragile


def rays_finite(oracle_scene, profile):
    """Every ray of every path of the frame is finite (checked on the CPU before a case goes to a GPU)."""
    for s in range(1, profile.samples + 1):
        for p in range(profile.width * profile.height):
            if not np.isfinite(oracle_scene.path_rays(profile, p, s)).all():
                return False
    return True


# ---- the model over the matrix, once per session ------------------------------------------------------------------------
def model_job(job):
    """(case name, bounces) -> what the tests need of the model's frame at that depth, plain arrays (runs in a worker
    process: CPU only, the oracle and the model)."""
    import __graft_entry__ as entry
    import scene_builder as sb
    name, bounces = job
    oracle = entry.load_oracle()
    case = sb.case_by_name(name)
    scene = sb.build(case)
    o = oracle.OracleScene(scene.desc, oracle.PTO_BRUTE_FORCE)
    w, h = DIRECT_SIZE if bounces == 0 else PATH_SIZE
    prof = sb.profile(case, w, h, 1, bounces=bounces)
    _, acc, stats = o.render(prof)
    results, rays = ShadingModel(scene.desc, o, oracle).image(prof)
    return dict(job=job, results=[(r.radiance, r.ray_error, r.fragile, r.alive_at_last) for r in results], oracle_accum=acc,
                numeric_errors=stats["numeric_errors"], rays_finite=all(bool(np.isfinite(r).all()) for r in rays))


class Frame:
    """A model_job's answer with the PathResults rebuilt."""

    def __init__(self, d):
        self.results = []
        for radiance, ray_error, fragile, alive in d["results"]:
            r = PathResult()
            r.radiance, r.ray_error, r.fragile, r.alive_at_last = radiance, ray_error, fragile, alive
            self.results.append(r)
        self.oracle_accum, self.numeric_errors, self.rays_finite = d["oracle_accum"], d["numeric_errors"], d["rays_finite"]


def run_jobs(jobs, workers=8):
    """{job: Frame} - in fresh worker processes (spawned: they must not inherit a GPU context)."""
    import multiprocessing
    from concurrent.futures import ProcessPoolExecutor
    jobs = list(jobs)
    with ProcessPoolExecutor(min(workers, max(1, len(jobs))), mp_context=multiprocessing.get_context("spawn")) as pool:
        return {d["job"]: Frame(d) for d in pool.map(model_job, jobs)}
