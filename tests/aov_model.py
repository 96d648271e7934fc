"""Sample-coherent AOVs (include/ptgpu.h pt_render_aov) restated without csrc/.

  reduce_records   the pixel record's sums: blocks of 64 sample numbers, the pairwise tree with its zero additions done literally
  guides_of        pt_aov_guides
  records_f64      the per-sample records in float64 from tests/shading_model.py (camera_ray / hits_of / material_sample /
                   shading_normal) over the oracle's f32 camera ray (primary_ray), its brute-force hit list (trace_all) and
                   the generator's words (rng_words); the alpha walk is done here, and a sample is flagged fragile when one of
                   its discrete decisions is too close to call
  records_f32      the same features in numpy float32, one operation per step, written from SURVEY 8 a8/a9
  deviation        the per-field relative deviation the tolerance fixture (tools/measure_aov_deviation.py) records and the
                   GPU test (tests/test_aov_gpu.py) bounds
  cases / build    the scenes both the CPU condition (at most 1 % fragile samples) and the GPU test use
"""
import ctypes as C
import math

import numpy as np

import scene_builder as sb
import shading_model as sm

f32 = np.float32
FLOATS = 16
FRAGILE_CAP = 0.01
SAMPLE_SIZE, SAMPLES = (16, 12), 3            # the frames of the per-sample comparison
MAX_HITS = 64                                  # trace_all's list: longer than the 25 entries of the pane stack
LUM = tuple(float(f32(v)) for v in (0.2126, 0.7152, 0.0722))
FIELDS = {"normal": slice(0, 3), "albedo": slice(4, 7), "position": slice(8, 11), "roughness": slice(11, 12),
          "metalness": slice(12, 13), "emissive_lum": slice(13, 14)}


# ---------------------------------------------------------------------------------------------------- the pixel record
def tree64(block):
    """x[j] = x[2j] + x[2j+1], six levels, over axis 0 of a [64, ...] float32 array."""
    x = np.asarray(block, f32)
    assert x.shape[0] == 64
    while x.shape[0] > 1:
        x = (x[0::2] + x[1::2]).astype(f32)
    return x[0]


def reduce_records(records):
    """[N, n, 16] float32 sample records -> [n, 16] float32 pixel records."""
    r = np.ascontiguousarray(records, f32)
    n_samples, n = r.shape[0], r.shape[1]
    out = np.zeros((n, FLOATS), f32)
    total = None
    with np.errstate(all="ignore"):
        for base in range(0, n_samples, 64):
            block = np.zeros((64, n, 14), f32)            # a missing sample is +0.0f
            part = r[base:base + 64, :, :14]
            block[:part.shape[0]] = part
            s = tree64(block)
            total = s if total is None else (total + s).astype(f32)
    out[:, :14] = total
    prim = r[:, :, 14].view(np.int32)
    covered = r[:, :, 15] > 0
    first = np.where(covered.any(axis=0), covered.argmax(axis=0), 0)
    first_prim = np.where(covered.any(axis=0), prim[first, np.arange(n)], -1).astype(np.int32)
    out[:, 14] = first_prim.view(f32)
    out[:, 15] = (covered & (prim == first_prim[None, :])).sum(axis=0).astype(f32)
    return out


def guides_of(aov, samples):
    """pt_aov_guides: [n, 16] pixel records of a frame of `samples` samples -> [n, 8] guides."""
    r = np.ascontiguousarray(aov, f32).reshape(-1, FLOATS)
    fn = f32(samples)
    cov = r[:, 7]
    valid = (cov > 0) & ((cov + cov).astype(f32) >= fn)
    g = np.zeros((len(r), 8), f32)
    with np.errstate(all="ignore"):
        g[:, 0:3] = np.where(valid[:, None], r[:, 0:3], f32(0))
        g[:, 3] = np.where(valid, (r[:, 3] / cov).astype(f32), f32(-1.0))
        g[:, 4:7] = np.where(valid[:, None], (r[:, 4:7] / fn).astype(f32), f32(0))
    g[:, 7] = np.where(valid, r[:, 14].view(np.int32), -1).astype(np.int32).view(f32)
    return g


# ---------------------------------------------------------------------------------------------------- float64 records
class SampleRecords:
    """values [N, n, 16] float64 (float 14 unused), prim [N, n] int32 (-1: no surface), dist [N, n] float32 (the selected list
    entry's, bit for bit), fragile [N, n] bool, hit [N, n]: the selected entry (oracle.HIT_DTYPE), rays [N, n, 6] float32."""

    def __init__(self, n_samples, n, hit_dtype):
        self.values = np.zeros((n_samples, n, FLOATS))
        self.prim = np.full((n_samples, n), -1, np.int32)
        self.dist = np.zeros((n_samples, n), f32)
        self.fragile = np.zeros((n_samples, n), bool)
        self.hit = np.zeros((n_samples, n), hit_dtype)
        self.rays = np.zeros((n_samples, n, 6), f32)
        self.textured = np.zeros((n_samples, n), bool)   # the surface's material reads a texture for albedo / roughness / metalness


def records_f64(model, profile, pixels=None, first_entry=False):
    """The record of every sample of the given global pixels (default: all) of the frame `profile`."""
    oracle, scene = model.oracle, model.scene
    n_samples = profile.samples
    pixels = list(range(profile.width * profile.height)) if pixels is None else list(pixels)
    out = SampleRecords(n_samples, len(pixels), oracle.HIT_DTYPE)
    for k, pixel in enumerate(pixels):
        for s in range(1, n_samples + 1):
            out.rays[s - 1, k] = scene.primary_ray(profile, pixel, s)
    flat = out.rays.reshape(-1, 6)
    ok = np.isfinite(flat).all(axis=1)
    recs, counts = scene.trace_all(np.where(ok[:, None], flat, 0).astype(f32), MAX_HITS)
    counts = np.where(ok, counts, 0)
    seeds = np.array([s + pixel * n_samples for s in range(1, n_samples + 1) for pixel in pixels], np.uint64)
    words = oracle.rng_words(seeds, 80)
    for at in range(len(flat)):
        s0, k = divmod(at, len(pixels))
        res = sm.PathResult()
        draws = sm.Draws(words[at])
        o64, d64 = model.camera_ray(profile, pixels[k], draws)     # (draws 0 and 1; the walk goes on from the f32 ray)
        r = [float(v) for v in flat[at]]
        fo, fd = tuple(r[:3]), tuple(r[3:])
        if not ok[at] or max(abs(a - b) for a, b in zip(o64 + d64, fo + fd)) > 1e-5 * max(1.0, max(abs(v) for v in fo + fd)):
            res.flag("camera ray")
        n = int(counts[at])
        if n >= MAX_HITS:
            res.flag("hit list truncated")
        hits = model.hits_of((fo, fd), recs[at][:n])
        chosen = None
        for j, hit in enumerate(hits):                               # mod.rs:189-205
            ms = model.material_sample(hit["model"]["material"], hit, res)
            chosen = (j, hit, ms)
            if first_entry:
                break
            op = ms["opacity"]
            if hit["model"]["material"]["tex"]["opacity"] >= 0 and not hit["sphere"] and (
                    abs(op - 1.0) < sm.CLOSE or abs(op - sm.OPACITY_MIN) < sm.CLOSE * sm.OPACITY_MIN):
                res.flag("opacity at a threshold")
            if op >= 1.0:
                break
            if op > sm.OPACITY_MIN:
                u = draws.next()
                if abs(u - op) < sm.CLOSE:
                    res.flag("alpha draw next to the opacity")
                if u < op:
                    break
        if chosen is not None:
            j, hit, ms = chosen
            nrm = model.shading_normal(hit, res)
            nn = sm.dot(nrm, nrm)
            unit = sm.scale(nrm, 1.0 / math.sqrt(nn)) if 0.0 < nn < math.inf else (0.0, 0.0, 0.0)
            e = ms["emissive"]
            v = out.values[s0, k]
            v[0:3], v[3], v[4:7], v[7] = unit, float(recs[at][j]["dist"]), ms["albedo"], 1.0
            v[8:11], v[11], v[12] = hit["pos"], ms["roughness"], ms["metalness"]
            v[13] = (LUM[0] * e[0] + LUM[1] * e[1]) + LUM[2] * e[2]
            v[15] = 1.0
            out.prim[s0, k] = int(recs[at][j]["prim"])
            out.dist[s0, k] = recs[at][j]["dist"]
            out.hit[s0, k] = recs[at][j]
            t = hit["model"]["material"]["tex"]
            out.textured[s0, k] = not hit["sphere"] and (t["albedo"] >= 0 or t["roughness"] >= 0 or t["metalness"] >= 0)
        out.fragile[s0, k] = res.fragile is not None
    return out


def rounded(rec):
    """records_f64's values rounded to float32, in the layout of pt_render_aov_samples ([N, n, 16], the primitive in float 14)."""
    out = rec.values.astype(f32)
    out[..., 14] = rec.prim.view(f32)
    return out


# ---------------------------------------------------------------------------------------------------- float32 records
def _v3(a):
    return np.array(a, f32)


def _dot32(a, b):
    return f32(f32(a[0] * b[0] + a[1] * b[1]) + a[2] * b[2])


def _norm32(a):
    return (a * (f32(1.0) / np.sqrt(_dot32(a, a)))).astype(f32)


def _cross32(a, b):
    return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]], f32)


def _texel32(model, tex, uv):
    off, w, h, ch = model.textures[tex]
    out = []
    for c, n in ((f32(uv[0] * f32(w)), w), (f32(uv[1] * f32(h)), h)):
        out.append((int(c) if math.isfinite(float(c)) else 0) % n)   # trunc_i64, rem_euclid
    p = off + (out[1] * w + out[0]) * ch
    return model.texels[p:p + ch]


def records_f32(model, rec):
    """[N, n, 16] float32: the features of records_f64's selected list entries (rec.hit over rec.rays) in float32, every step
    one operation in the order of SURVEY 8 a8 (Hit::new_triangle, get_normal) and a9 (MaterialSample, Material::get_*)."""
    out = np.zeros(rec.values.shape, f32)
    with np.errstate(all="ignore"):
        for idx in np.ndindex(rec.prim.shape):
            prim = int(rec.prim[idx])
            if prim < 0:
                continue
            h, ray = rec.hit[idx], rec.rays[idx]
            o, d = ray[:3], ray[3:]
            mdl = model.models[model.prim_model[prim]]
            m, t = mdl["material"], mdl["material"]["tex"]
            albedo, emissive = _v3(m["albedo"]), _v3(m["emissive"])
            rough, metal = f32(m["roughness"]), f32(m["metalness"])
            if int(h["flags"]) & 2:                                    # a6: the sphere arm; a9: MaterialSample::simple
                c = _v3(mdl["center"])
                # a6: a = d.d, b = 2 (o - c).d, c = |o - c|^2 - r^2; t = (-b -+ sqrt(b^2 - 4ac)) / (2a); p = o + d * t (the hit
                # record carries dist = |p - o|, not t: the float64 model goes back through dist / |d|)
                rc, rad = (o - c).astype(f32), f32(mdl["radius"])
                qa, qb = _dot32(d, d), f32(f32(2.0) * _dot32(rc, d))
                qc = f32(_dot32(rc, rc) - f32(rad * rad))
                root = np.sqrt(f32(f32(qb * qb) - f32(f32(f32(4.0) * qa) * qc)))
                tpar = f32(f32(-qb + root) / f32(f32(2.0) * qa)) if int(h["flags"]) & 4 else f32(f32(-qb - root) / f32(f32(2.0) * qa))
                p = (o + d * tpar).astype(f32)
                n = _norm32((p - c).astype(f32))
                if int(h["flags"]) & 4:
                    n = -n
                pos = p
            else:
                v0, v1, v2 = (np.array(v, f32) for v in model.tri_list[model.prim_tri[prim]])
                u, v = f32(h["u"]), f32(h["v"])
                n = (((f32(1.0) - u - v) * v0[3:6] + u * v1[3:6]) + v * v2[3:6]).astype(f32)
                uv = ((v0[6:8] + u * (v1[6:8] - v0[6:8])) + v * (v2[6:8] - v0[6:8])).astype(f32)
                pos = (o + d * f32(h["dist"])).astype(f32)
                if t["normal"] >= 0:
                    e1, e2 = (v1[0:3] - v0[0:3]).astype(f32), (v2[0:3] - v0[0:3]).astype(f32)
                    d1, d2 = (v1[6:8] - v0[6:8]).astype(f32), (v2[6:8] - v0[6:8]).astype(f32)
                    f = f32(1.0) / f32(d1[0] * d2[1] - d2[0] * d1[1])
                    tg = _norm32((f * (d2[1] * e1 - d1[1] * e2)).astype(f32))
                    px = _texel32(model, t["normal"], uv)
                    nm = np.array([f32(px[k]) / f32(127.5) - f32(1.0) for k in range(3)], f32)
                    bt = _cross32(n, tg)
                    n = _norm32(((tg * nm[0] + bt * nm[1]) + n * nm[2]).astype(f32))
                if int(h["flags"]) & 1:
                    n = -n
                if t["albedo"] >= 0:
                    px = _texel32(model, t["albedo"], uv)
                    albedo = (np.power(px[:3].astype(f32) / f32(255.0), f32(2.2)).astype(f32) * albedo).astype(f32)
                if t["emissive"] >= 0:
                    px = _texel32(model, t["emissive"], uv)
                    emissive = ((px[:3].astype(f32) / f32(255.0)) * emissive).astype(f32)
                if t["metalness"] >= 0:
                    metal = f32(f32(_texel32(model, t["metalness"], uv)[0]) / f32(255.0) * metal)
                if t["roughness"] >= 0:
                    rough = f32(f32(_texel32(model, t["roughness"], uv)[0]) / f32(255.0) * rough)
            rough = max(rough, f32(0.0001))
            nn = _dot32(n, n)
            unit = (n * (f32(1.0) / np.sqrt(nn))).astype(f32) if 0.0 < nn < np.inf else np.zeros(3, f32)
            r = out[idx]
            r[0:3], r[3], r[4:7], r[7], r[8:11], r[11], r[12] = unit, h["dist"], albedo, 1.0, pos, rough, metal
            r[13] = f32(f32(f32(0.2126) * emissive[0] + f32(0.7152) * emissive[1]) + f32(0.0722) * emissive[2])
            r[14] = np.int32(prim).view(f32)
            r[15] = 1.0
    return out


# ---------------------------------------------------------------------------------------------------- the comparison
def deviation(got, rec, origin):
    """{field: [N, n] float64}: the deviation of float32 records `got` [N, n, 16] from records_f64's, relative to the field's
    own size - the normal is a unit vector: its largest component difference; albedo: over its largest component; the
    position: over the larger of the position's and the ray origin's largest coordinate (it is o + d * dist: the rounding
    is that of its terms); the scalars: over their own value.  Where the reference field is exactly 0 only 0 deviates by 0
    (anything else: inf).  Samples without a surface deviate by 0 when `got` is all zero there, else by inf."""
    want = rec.values
    got = np.asarray(got, np.float64)
    o = float(np.abs(np.asarray(origin, np.float64)).max())
    out = {}
    with np.errstate(all="ignore"):
        for name, sl in FIELDS.items():
            diff = np.abs(got[..., sl] - want[..., sl]).max(axis=-1)
            if name == "normal":
                scale = np.ones(diff.shape)
            elif name == "position":
                scale = np.maximum(np.abs(want[..., sl]).max(axis=-1), o)
            else:
                scale = np.abs(want[..., sl]).max(axis=-1)
            dev = np.where(diff == 0, 0.0, np.where(scale > 0, diff / scale, np.inf))
            out[name] = np.where(np.isnan(dev), np.inf, dev)
    return out


# ---------------------------------------------------------------------------------------------------- the cases
BUILT_CASES = ("all-point", "none-point_dir", "albedo-none", "normal-point")   # scene_builder: every texture kind and the
# sphere (translucent, an opacity texture); untextured and translucent; opaque with an albedo texture; a normal map alone
GOLDEN_CASES = ("alpha_transparency",)
PANES = "pane-stack"
CASES = BUILT_CASES + GOLDEN_CASES + (PANES,)
N_PANES, PANE_OPACITY = 24, 0.05


def pane_stack(pta):
    """24 panes of opacity 0.05, 0.05 apart, in front of an opaque wall: nine walks in ten look at more than the 14 entries
    the first ChaCha block has draws for, and three in ten (0.95^24) skip every pane and stop at the wall; without the wall
    behind the upper half of the panes a walk that skips them all keeps the last one."""
    tris, models, mats = [], [], []
    n1 = [np.array([0.0, 0.0, 1.0])] * 4
    for k in range(N_PANES):
        q = sb._quad((-1.5, -1.0, -0.05 * k), (3.0, 0, 0), (0, 2.0, 0), n1, (0.0, 0.0), (1.0, 0.0), (0.0, 1.0))
        models.append(pta.Model(pta.PT_MODEL_MESH, k, len(tris), len(q), (C.c_float * 3)(0, 0, 0), 0.0))
        tris += q
        g = 0.2 + 0.03 * k
        mats.append(pta.Material((C.c_float * 3)(g, 1.0 - g, 0.5), (C.c_float * 3)(0.01 * k, 0.0, 0.02), PANE_OPACITY, 0.1, 0.3 + 0.02 * k,
                                 1.5, -1, -1, -1, -1, -1, -1))
    q = sb._quad((-1.5, -1.0, -2.0), (3.0, 0, 0), (0, 1.0, 0), n1, (0.0, 0.0), (1.0, 0.0), (0.0, 1.0))
    models.append(pta.Model(pta.PT_MODEL_MESH, N_PANES, len(tris), len(q), (C.c_float * 3)(0, 0, 0), 0.0))
    tris += q
    mats.append(pta.Material((C.c_float * 3)(0.9, 0.8, 0.7), (C.c_float * 3)(0.3, 0.2, 0.1), 1.0, 0.0, 1.0, 1.5, -1, -1, -1, -1, -1, -1))
    camera = sb.make_camera(pta, eye=(0.11, 0.07, 2.2), target=(0.02, -0.03, -1.0), fov=0.8)
    return sb.BuiltScene(pta, np.array(tris, f32).reshape(-1, 24), models, mats, [], np.zeros(1, np.uint8), [], camera,
                         (0.25, 0.3, 0.45))


def build(name, pta, scene_cache=None):
    """(what GpuScene / OracleScene take: an object with .desc, its camera)."""
    if name == PANES:
        s = pane_stack(pta)
        return s, s.desc.contents.camera
    if name in GOLDEN_CASES:
        from conftest import SCENES
        s = scene_cache(name) if scene_cache else pta.HostScene.load_isf(SCENES / name / "scene.isf")
        return s, s.camera
    s = sb.build(sb.case_by_name(name), pta=pta)
    return s, s.desc.contents.camera


def sample_profile(pta, width=SAMPLE_SIZE[0], height=SAMPLE_SIZE[1], samples=SAMPLES):
    return pta.Profile.make(width, height, samples, 0, "FILMIC")


def model_of(name, pta, oracle, scene_cache=None):
    scene, camera = build(name, pta, scene_cache)
    osc = oracle.OracleScene(scene.desc, oracle.PTO_BRUTE_FORCE, keepalive=scene)
    return sm.ShadingModel(scene.desc, osc, oracle, max_hits=MAX_HITS), scene, camera


def origin_of(camera):
    return [float(v) for v in list(camera.transform)[12:15]]
