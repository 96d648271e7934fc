"""A numpy float32 restatement of the sample moments and the variance-guided a-trous filter of include/ptgpu.h
(pt_render_moments, pt_denoise_var).

Written from the specification like denoise_model.py, whose prep, tap weights and helpers it shares: every line is ONE IEEE
f32 operation on whole-image arrays, taps are visited in the specified order, so the device is held to it bit for bit.
"""
import numpy as np

import denoise_model as dm

f32 = np.float32
NO_DEMODULATE = dm.NO_DEMODULATE
G_KERNEL = (f32(0.25), f32(0.125), f32(0.0625))


def lum(a):
    return (f32(0.2126) * a[..., 0] + f32(0.7152) * a[..., 1]) + f32(0.0722) * a[..., 2]


def moments_of(planes):
    """planes [N, n, 3] float32, the samples of n pixels in order: (accum [n, 3], moments [n, 2]) as pt_render_moments builds
    them, one f32 operation per step."""
    planes = np.asarray(planes, f32)
    acc = np.zeros(planes.shape[1:], f32)
    m1 = np.zeros(planes.shape[1], f32)
    m2 = np.zeros(planes.shape[1], f32)
    with np.errstate(all="ignore"):
        for c in planes:
            L = lum(c)
            acc = acc + c
            m1 = m1 + L
            m2 = m2 + L * L
    return acc, np.stack([m1, m2], axis=1)


def moments_from_partial_sums(partials):
    """Moments from the oracle's accumulators after 1, 2, .. N sample passes ([N, n, 3]): sample k is taken as the DIFFERENCE of
    two partial sums, which is the sample only up to the rounding of those sums - for the quality measurements on the CPU,
    NOT the device's bits."""
    partials = np.asarray(partials, f32)
    planes = np.concatenate([partials[:1], partials[1:] - partials[:-1]], axis=0)
    return moments_of(planes)[1]


def variance_of_mean(samples, moments, lum_d=None):
    """prep's v for every pixel ([...] float32); lum_d: lum(d) of the demodulation, None with NO_DEMODULATE."""
    N = f32(samples)
    mu = moments[..., 0] / N
    e2 = moments[..., 1] / N
    s2 = np.fmax(f32(0.0), e2 - mu * mu)
    v = s2 / f32(samples - 1)
    if lum_d is not None:
        v = v / (lum_d * lum_d)
    return v


def denoise_var(width, height, samples, accum, moments, guides, iterations, sigma_color, sigma_depth, normal_power_log2, flags=0):
    """out_color [H*W, 3] float32 of pt_denoise_var."""
    with np.errstate(all="ignore"):
        acc_in = np.asarray(accum, f32).reshape(height, width, 3)
        mom = np.asarray(moments, f32).reshape(height, width, 2)
        g = np.asarray(guides, f32).reshape(height, width, 8)
        c = acc_in / f32(samples)
        if iterations == 0:
            return c.reshape(-1, 3).copy()
        n, z, albedo = g[..., 0:3], g[..., 3], g[..., 4:7]
        valid = z >= f32(0.0)
        nn = dm.dot3(n, n)
        u = np.where(((nn > 0) & np.isfinite(nn))[..., None], dm.normalize3(n), f32(0.0)).astype(f32)
        demod = not (flags & NO_DEMODULATE)
        d = albedo + f32(0.01) if demod else np.ones_like(albedo)
        x = c / d if demod else c.copy()
        v = variance_of_mean(samples, mom, lum(d) if demod else None)
        v = np.where(valid, v, f32(0.0)).astype(f32)
        gx = dm._slope(z, valid, 1)
        gy = dm._slope(z, valid, 0)
        sigma_color, sigma_depth = f32(sigma_color), f32(sigma_depth)
        zterm = f32(1e-4) * z
        for i in range(iterations):
            s = 1 << i
            b = np.zeros_like(z)
            bs = np.zeros_like(z)
            for dy in range(-1, 2):
                for dx in range(-1, 2):
                    gw = G_KERNEL[abs(dx) + abs(dy)]
                    vq_ok = dm._shifted(valid, dx, dy, False)
                    vq = dm._shifted(v, dx, dy, f32(0.0))
                    b = np.where(vq_ok, b + vq * gw, b)
                    bs = np.where(vq_ok, bs + gw, bs)
            vb = b / bs
            lden = sigma_color * np.sqrt(vb) + f32(1e-6)
            lp = lum(x)
            acc = np.zeros_like(x)
            wsum = np.zeros_like(z)
            vacc = np.zeros_like(z)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    k = dm.H_KERNEL[abs(dx)] * dm.H_KERNEL[abs(dy)]
                    ox, oy = s * dx, s * dy
                    vq_ok = dm._shifted(valid, ox, oy, False)
                    xq = dm._shifted(x, ox, oy, f32(0.0))
                    vq = dm._shifted(v, ox, oy, f32(0.0))
                    if dx == 0 and dy == 0:
                        w = np.full_like(z, k)
                    else:
                        uq = dm._shifted(u, ox, oy, f32(0.0))
                        zq = dm._shifted(z, ox, oy, f32(0.0))
                        wn = np.fmax(f32(0.0), dm.dot3(u, uq))
                        for _ in range(normal_power_log2):
                            wn = wn * wn
                        den = gx * f32(s * abs(dx)) + gy * f32(s * abs(dy))
                        den = sigma_depth * den
                        den = den + zterm
                        wz = dm.wexp(np.abs(z - zq) / den)
                        wl = dm.wexp(np.abs(lp - lum(xq)) / lden)
                        w = ((k * wn) * wz) * wl
                    take = valid & vq_ok
                    acc = np.where(take[..., None], acc + xq * w[..., None], acc)
                    wsum = np.where(take, wsum + w, wsum)
                    vacc = np.where(take, vacc + vq * (w * w), vacc)
            x = np.where(valid[..., None], acc / wsum[..., None], x).astype(f32)
            v = np.where(valid, vacc / (wsum * wsum), v).astype(f32)
        out = x * d if demod else x
        out = np.where(valid[..., None], out, c).astype(f32)
        return out.reshape(-1, 3).copy()


def denoise_var_with(params, width, height, samples, accum, moments, guides):
    """denoise_var() with the fields of a pt_denoise_params structure."""
    return denoise_var(width, height, samples, accum, moments, guides, int(params.iterations), params.sigma_color,
                       params.sigma_depth, int(params.normal_power_log2), int(params.flags))


def synthetic_moments(samples, accum, seed):
    """Moments [n, 2] for an accumulator of dm.synthetic_inputs: consistent with the pixel's luminance, a relative spread
    between 0 and ~1, and the three special populations - exactly zero variance (m2 = m1^2/N up to its rounding), m2 BELOW
    m1^2/N (the clamp of s2), and fireflies (one sample carries the pixel)."""
    rng = np.random.default_rng(seed)
    accum = np.asarray(accum, f32)
    n = len(accum)
    N = f32(samples)
    m1 = lum(accum)
    base = (m1 * m1) / N
    m2 = (base * (f32(1.0) + rng.random(n).astype(f32))).astype(f32)
    kind = rng.random(n)
    m2 = np.where(kind < 0.15, base, m2)
    m2 = np.where((kind >= 0.15) & (kind < 0.25), base * f32(0.9), m2)
    m2 = np.where(kind >= 0.97, m1 * m1, m2)
    return np.stack([m1, m2], axis=1).astype(f32)


# ------------------------------------------------------------------------------------------------ inputs without a GPU
def inputs_from_oracle(pta, oracle, scene_path, width, height, spp, bounces):
    """(accum, moments, guides) of a golden scene for the quality measurements (tools/measure_denoise_var_gain.py and its
    test): the oracle's frame, moments from the differences of its partial sums (moments_from_partial_sums: not the device's
    bits) and dm.guides_from_oracle."""
    hs = pta.HostScene.load_isf(scene_path)
    osc = oracle.OracleScene(hs.desc, oracle.PTO_BVH)
    prof = pta.Profile.make(width, height, spp, bounces)
    partials = np.stack([osc.render(prof, sample_count=k)[1] for k in range(1, spp + 1)])
    return partials[-1], moments_from_partial_sums(partials), dm.guides_from_oracle(osc, hs.camera, width, height)
