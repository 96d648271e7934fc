"""A numpy float32 restatement of the a-trous filter of include/ptgpu.h (pt_denoise) and of the camera ray.

Written from the specification, not from the kernels: every line below is ONE IEEE f32 operation on whole-image arrays
(numpy rounds each f32 operation once, there is no contraction), taps are visited in the specified order (dy outer, dx
inner), so the device result can be held to this model bit for bit.  Nothing here calls a transcendental function; the one
the camera needs (tan of half the field of view) comes from libm's tanf, as the library's host code takes it.
"""
import ctypes
import ctypes.util

import numpy as np

f32 = np.float32
NO_DEMODULATE = 1
H_KERNEL = (f32(0.375), f32(0.25), f32(0.0625))

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.tanf.restype = ctypes.c_float
_libm.tanf.argtypes = [ctypes.c_float]


def tanf(x):
    return f32(_libm.tanf(float(f32(x))))


# ------------------------------------------------------------------------------------------------ vector helpers (pt_math.h)
def dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def normalize3(a):
    inv = f32(1.0) / np.sqrt(dot3(a, a))
    return a * inv[..., None]


# ------------------------------------------------------------------------------------------------ the camera ray
def primary_screen(x, y, width, height, r1, r2, tan_half_fov):
    """The jittered screen position of pixel (x, y): arrays of equal shape, r1 / r2 float32."""
    wf, hf = f32(width), f32(height)
    ratio = wf / hf
    sx = np.asarray(x).astype(f32) + np.asarray(r1, f32)
    sx = sx / wf
    sx = sx * f32(2.0)
    sx = sx - f32(1.0)
    sx = sx * (f32(tan_half_fov) * ratio)
    sy = np.asarray(y).astype(f32) + np.asarray(r2, f32)
    sy = sy / hf
    sy = sy * f32(2.0)
    sy = f32(1.0) - sy
    sy = sy * f32(tan_half_fov)
    return sx, sy


def primary_from_screen(transform, sx, sy):
    """(origin [.., 3], direction [.., 3]) of the ray through a screen position; transform: 16 floats, column k at 4k."""
    t = np.asarray(transform, f32)
    c0, c1, c2, c3 = t[0:3], t[4:7], t[8:11], t[12:15]
    v = np.stack([sx, sy, np.full_like(sx, f32(-1.0))], axis=-1)
    d = normalize3(v)
    w = ((c0 * d[..., 0:1] + c1 * d[..., 1:2]) + c2 * d[..., 2:3]) + c3 * f32(0.0)
    o = np.broadcast_to(c3, w.shape).copy()
    return o, w


def primary_rays(camera, width, height, r1=0.5, r2=0.5, pixels=None):
    """[n, 6] float32 rays (origin3, direction3) of the given pixel indices i = x + y*W (default: all), camera with
    .transform (16 floats) and .fov."""
    i = np.arange(width * height) if pixels is None else np.asarray(pixels)
    x, y = i % width, i // width
    tan_half = tanf(f32(camera.fov) / f32(2.0))
    r1 = np.broadcast_to(np.asarray(r1, f32), x.shape)
    r2 = np.broadcast_to(np.asarray(r2, f32), x.shape)
    sx, sy = primary_screen(x, y, width, height, r1, r2, tan_half)
    o, d = primary_from_screen(list(camera.transform), sx, sy)
    return np.concatenate([o, d], axis=-1).astype(f32)


# ------------------------------------------------------------------------------------------------ the filter
def wexp(e):
    r = np.fmax(f32(0.0), f32(1.0) - e * f32(0.125))
    r = r * r
    r = r * r
    r = r * r
    return r


def _slope(z, valid, axis):
    """min of the two one-sided |differences| over the valid in-image neighbours along `axis`; one: that one; none: 0."""
    zm, zp = np.roll(z, 1, axis), np.roll(z, -1, axis)
    vm, vp = np.roll(valid, 1, axis), np.roll(valid, -1, axis)
    idx = np.arange(z.shape[axis]).reshape((-1, 1) if axis == 0 else (1, -1))
    vm = vm & (idx > 0)
    vp = vp & (idx < z.shape[axis] - 1)
    dm = np.abs(z - zm)
    dp = np.abs(zp - z)
    return np.where(vm & vp, np.fmin(dp, dm), np.where(vp, dp, np.where(vm, dm, f32(0.0)))).astype(f32)


def _shifted(a, ox, oy, fill):
    """b[y, x] = a[y + oy, x + ox] where that is inside the image, else fill."""
    h, w = a.shape[:2]
    out = np.full_like(a, fill)
    ys0, ys1 = max(0, -oy), min(h, h - oy)
    xs0, xs1 = max(0, -ox), min(w, w - ox)
    if ys0 < ys1 and xs0 < xs1:
        out[ys0:ys1, xs0:xs1] = a[ys0 + oy:ys1 + oy, xs0 + ox:xs1 + ox]
    return out


def denoise(width, height, samples, accum, guides, iterations, sigma_color, sigma_depth, normal_power_log2, flags=0):
    """out_color [H*W, 3] float32 of pt_denoise."""
    with np.errstate(all="ignore"):
        acc_in = np.asarray(accum, f32).reshape(height, width, 3)
        g = np.asarray(guides, f32).reshape(height, width, 8)
        c = acc_in / f32(samples)
        if iterations == 0:
            return c.reshape(-1, 3).copy()
        n, z, albedo = g[..., 0:3], g[..., 3], g[..., 4:7]
        valid = z >= f32(0.0)
        nn = dot3(n, n)
        u = np.where(((nn > 0) & np.isfinite(nn))[..., None], normalize3(n), f32(0.0)).astype(f32)
        demod = not (flags & NO_DEMODULATE)
        d = albedo + f32(0.01) if demod else np.ones_like(albedo)
        x = c / d if demod else c.copy()
        gx = _slope(z, valid, 1)
        gy = _slope(z, valid, 0)
        sigma_color, sigma_depth = f32(sigma_color), f32(sigma_depth)
        zterm = f32(1e-4) * z
        for i in range(iterations):
            s = 1 << i
            sc = sigma_color * f32(2.0 ** -i)
            sc2 = sc * sc
            acc = np.zeros_like(x)
            wsum = np.zeros_like(z)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    k = H_KERNEL[abs(dx)] * H_KERNEL[abs(dy)]
                    ox, oy = s * dx, s * dy
                    vq = _shifted(valid, ox, oy, False)
                    xq = _shifted(x, ox, oy, f32(0.0))
                    if dx == 0 and dy == 0:
                        w = np.full_like(z, k)
                    else:
                        uq = _shifted(u, ox, oy, f32(0.0))
                        zq = _shifted(z, ox, oy, f32(0.0))
                        wn = np.fmax(f32(0.0), dot3(u, uq))
                        for _ in range(normal_power_log2):
                            wn = wn * wn
                        den = gx * f32(s * abs(dx)) + gy * f32(s * abs(dy))
                        den = sigma_depth * den
                        den = den + zterm
                        wz = wexp(np.abs(z - zq) / den)
                        w = (k * wn) * wz
                        if sigma_color != 0:
                            dl = x - xq
                            w = w * wexp(dot3(dl, dl) / sc2)
                        else:
                            w = w * f32(1.0)
                    take = valid & vq
                    acc = np.where(take[..., None], acc + xq * w[..., None], acc)
                    wsum = np.where(take, wsum + w, wsum)
            x = np.where(valid[..., None], acc / wsum[..., None], x).astype(f32)
        out = x * d if demod else x
        out = np.where(valid[..., None], out, c).astype(f32)
        return out.reshape(-1, 3).copy()


def denoise_with(params, width, height, samples, accum, guides):
    """denoise() with the fields of a pt_denoise_params structure."""
    return denoise(width, height, samples, accum, guides, int(params.iterations), params.sigma_color, params.sigma_depth,
                   int(params.normal_power_log2), int(params.flags))


# ------------------------------------------------------------------------------------------------ guides without a GPU
def guides_from_oracle(osc, camera, width, height):
    """A CPU stand-in for pt_render_guides, for the quality measurements (tools/measure_denoise_gain.py and its test):
    depth and primitive index are the oracle's first ray_cast entry of the restated pixel-centre rays (exact); normal and
    albedo are dequantised from the oracle's u8 debug planes - it has no float planes - so they are NOT the device's bits."""
    rays = primary_rays(camera, width, height)
    hits, counts = osc.trace_all(rays, 1)
    hit = counts > 0
    g = np.zeros((width * height, 8), f32)
    g[:, 3] = np.where(hit, hits["dist"][:, 0], f32(-1.0))
    g[:, 7] = np.where(hit, hits["prim"][:, 0], -1).astype(np.int32).view(f32)
    planes = osc.debug_render(width, height)
    if planes:
        g[:, 0:3] = np.where(hit[:, None], (planes["normal"].astype(f32) / f32(255.0) - f32(0.5)) * f32(2.0), f32(0.0))
        g[:, 4:7] = np.where(hit[:, None], planes["albedo"].astype(f32) / f32(255.0), f32(0.0))
    return g


# ------------------------------------------------------------------------------------------------ test inputs
def synthetic_inputs(width, height, seed):
    """Accumulator and guides with every feature the filter looks at: ~30 % invalid pixels, normals from a few clusters (some
    not unit length, one zero), sloped depth planes plus noise, albedo with zero channels."""
    rng = np.random.default_rng(seed)
    n = width * height
    y, x = np.divmod(np.arange(n), width)
    cluster = rng.integers(0, 5, n)
    normals = np.array([[0, 0, 1], [0, 2, 0], [0.6, 0, 0.8], [-0.3, 0.5, 0.2], [0, 0, 0]], f32)[cluster]
    normals = (normals + rng.normal(0, 0.02, (n, 3)).astype(f32) * (cluster[:, None] != 4)).astype(f32)
    slope = np.array([[0.1, 0.02], [0.0, 0.3], [-0.05, 0.0], [0.2, -0.1], [0.0, 0.0]], f32)[cluster]
    depth = (f32(20.0) + slope[:, 0] * x.astype(f32) + slope[:, 1] * y.astype(f32) + rng.normal(0, 0.01, n).astype(f32)).astype(f32)
    albedo = rng.random((n, 3)).astype(f32)
    albedo[rng.random((n, 3)) < 0.2] = 0
    invalid = rng.random(n) < 0.3
    g = np.zeros((n, 8), f32)
    g[:, 0:3], g[:, 3], g[:, 4:7] = normals, depth, albedo
    g[:, 7] = rng.integers(0, 1000, n).astype(np.int32).view(f32)
    g[invalid, 0:7] = 0
    g[invalid, 3] = -1
    g[invalid, 7] = np.array([-1], np.int32).view(f32)[0]
    samples = 4
    accum = (rng.random((n, 3)).astype(f32) * f32(3.0) * f32(samples)).astype(f32)
    accum[rng.random(n) < 0.02] *= f32(40.0)   # fireflies
    return samples, accum, g
