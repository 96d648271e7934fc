"""The film filter of include/ptgpu.h (pt_film_denoise, pt_film_filtered_noise, pt_film_render_until_filtered)
restated in numpy float32: the prep of pt_denoise / pt_denoise_var with a sample count per pixel, their passes (the text of
denoise_model.py / denoise_var_model.py, whose helpers this file calls), the error figure of the filtered mean, the tile
reduction over it and the selection of the filtered loop.  Written from the header's text, one IEEE operation per step; with
a constant count array it must give denoise_model's and denoise_var_model's bits (tests/test_film_denoise_model.py), and
the GPU tests hold the kernels to it bit for bit."""
import numpy as np

import denoise_model as dm
import denoise_var_model as dvm
import film_adaptive_model as am
import film_model as fm

f32 = np.float32
NO_DEMODULATE = dm.NO_DEMODULATE


class Prep:
    """What prep leaves per pixel ([H, W] or [H, W, 3] float32): c = accum / N, x (demodulated), v (variance filter only),
    u, z, d, the depth slopes, and which pixels are valid."""


def prep(width, height, counts, accum, moments, guides, flags, variance):
    P = Prep()
    acc_in = np.asarray(accum, f32).reshape(height, width, 3)
    g = np.asarray(guides, f32).reshape(height, width, 8)
    n = np.broadcast_to(np.asarray(counts, np.uint32).reshape(-1), (width * height,)).reshape(height, width)
    N = n.astype(f32)
    P.c = (acc_in / N[..., None]).astype(f32)
    nrm, P.z, albedo = g[..., 0:3], g[..., 3], g[..., 4:7]
    P.valid = P.z >= f32(0.0)
    nn = dm.dot3(nrm, nrm)
    P.u = np.where(((nn > 0) & np.isfinite(nn))[..., None], dm.normalize3(nrm), f32(0.0)).astype(f32)
    P.demod = not (flags & NO_DEMODULATE)
    P.d = albedo + f32(0.01) if P.demod else np.ones_like(albedo)
    P.x = P.c / P.d if P.demod else P.c.copy()
    P.v = None
    if variance:
        mom = np.asarray(moments, f32).reshape(height, width, 2)
        mu = mom[..., 0] / N
        e2 = mom[..., 1] / N
        s2 = np.fmax(f32(0.0), e2 - mu * mu)
        v = s2 / (n - np.uint32(1)).astype(f32)
        if P.demod:
            ld = dvm.lum(P.d)
            v = v / (ld * ld)
        P.v = np.where(P.valid, v, f32(0.0)).astype(f32)
    P.gx = dm._slope(P.z, P.valid, 1)
    P.gy = dm._slope(P.z, P.valid, 0)
    return P


def _geometry_weight(P, k, s, dx, dy, sigma_depth, zterm, normal_power_log2):
    """(k * wn) * wz of one tap that is not the centre, and the shifted validity."""
    ox, oy = s * dx, s * dy
    uq = dm._shifted(P.u, ox, oy, f32(0.0))
    zq = dm._shifted(P.z, ox, oy, f32(0.0))
    wn = np.fmax(f32(0.0), dm.dot3(P.u, uq))
    for _ in range(normal_power_log2):
        wn = wn * wn
    den = P.gx * f32(s * abs(dx)) + P.gy * f32(s * abs(dy))
    den = sigma_depth * den
    den = den + zterm
    wz = dm.wexp(np.abs(P.z - zq) / den)
    return (k * wn) * wz


def plain_passes(P, iterations, sigma_color, sigma_depth, normal_power_log2):
    """pt_denoise's passes over prep's planes: the filtered x."""
    x, valid, z = P.x, P.valid, P.z
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
                k = dm.H_KERNEL[abs(dx)] * dm.H_KERNEL[abs(dy)]
                vq = dm._shifted(valid, s * dx, s * dy, False)
                xq = dm._shifted(x, s * dx, s * dy, f32(0.0))
                if dx == 0 and dy == 0:
                    w = np.full_like(z, k)
                else:
                    w = _geometry_weight(P, k, s, dx, dy, sigma_depth, zterm, normal_power_log2)
                    if sigma_color != 0:
                        dl = x - xq
                        w = w * dm.wexp(dm.dot3(dl, dl) / sc2)
                    else:
                        w = w * f32(1.0)
                take = valid & vq
                acc = np.where(take[..., None], acc + xq * w[..., None], acc)
                wsum = np.where(take, wsum + w, wsum)
        x = np.where(valid[..., None], acc / wsum[..., None], x).astype(f32)
    return x


def variance_passes(P, iterations, sigma_color, sigma_depth, normal_power_log2):
    """pt_denoise_var's passes over prep's planes: the filtered (x, v)."""
    x, v, valid, z = P.x, P.v, P.valid, P.z
    sigma_color, sigma_depth = f32(sigma_color), f32(sigma_depth)
    zterm = f32(1e-4) * z
    for i in range(iterations):
        s = 1 << i
        b = np.zeros_like(z)
        bs = np.zeros_like(z)
        for dy in range(-1, 2):
            for dx in range(-1, 2):
                gw = dvm.G_KERNEL[abs(dx) + abs(dy)]
                vq_ok = dm._shifted(valid, dx, dy, False)
                vq = dm._shifted(v, dx, dy, f32(0.0))
                b = np.where(vq_ok, b + vq * gw, b)
                bs = np.where(vq_ok, bs + gw, bs)
        vb = b / bs
        lden = sigma_color * np.sqrt(vb) + f32(1e-6)
        lp = dvm.lum(x)
        acc = np.zeros_like(x)
        wsum = np.zeros_like(z)
        vacc = np.zeros_like(z)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                k = dm.H_KERNEL[abs(dx)] * dm.H_KERNEL[abs(dy)]
                vq_ok = dm._shifted(valid, s * dx, s * dy, False)
                xq = dm._shifted(x, s * dx, s * dy, f32(0.0))
                vq = dm._shifted(v, s * dx, s * dy, f32(0.0))
                if dx == 0 and dy == 0:
                    w = np.full_like(z, k)
                else:
                    w = _geometry_weight(P, k, s, dx, dy, sigma_depth, zterm, normal_power_log2)
                    w = w * dm.wexp(np.abs(lp - dvm.lum(xq)) / lden)
                take = valid & vq_ok
                acc = np.where(take[..., None], acc + xq * w[..., None], acc)
                wsum = np.where(take, wsum + w, wsum)
                vacc = np.where(take, vacc + vq * (w * w), vacc)
        x = np.where(valid[..., None], acc / wsum[..., None], x).astype(f32)
        v = np.where(valid, vacc / (wsum * wsum), v).astype(f32)
    return x, v


def raw_error(moments, counts, lum_floor=fm.DEFAULT_LUM_FLOOR):
    """pt_film_noise's err with n = the pixel's own count."""
    n = np.broadcast_to(np.asarray(counts, np.uint32).reshape(-1), (len(np.asarray(moments).reshape(-1, 2)),))
    return am.pixel_error(moments, n, lum_floor)


def film_denoise(width, height, counts, accum, moments, guides, iterations, sigma_color, sigma_depth, normal_power_log2, flags=0,
                 variance=True, lum_floor=fm.DEFAULT_LUM_FLOOR):
    """(color [H*W, 3], ferr [H*W] or None for the plain filter) float32 of pt_film_denoise; counts: [H*W] uint32, or one
    number (a uniform film)."""
    with np.errstate(all="ignore"):
        P = prep(width, height, counts, accum, moments, guides, flags, variance)
        raw = raw_error(moments, counts, lum_floor) if variance else None
        if iterations == 0:
            return P.c.reshape(-1, 3).copy(), raw
        if variance:
            x, v = variance_passes(P, iterations, sigma_color, sigma_depth, normal_power_log2)
        else:
            x, v = plain_passes(P, iterations, sigma_color, sigma_depth, normal_power_log2), None
        out = x * P.d if P.demod else x
        out = np.where(P.valid[..., None], out, P.c).astype(f32)
        if not variance:
            return out.reshape(-1, 3).copy(), None
        vf = v
        if P.demod:
            ld = dvm.lum(P.d)
            vf = vf * (ld * ld)
        se = np.sqrt(vf)
        den = np.maximum(dvm.lum(out), f32(lum_floor))
        ferr = se / den
        ferr = np.where(P.valid, ferr, raw.reshape(height, width)).astype(f32)
        return out.reshape(-1, 3).copy(), ferr.reshape(-1).copy()


def film_denoise_with(params, width, height, counts, accum, moments, guides, variance=True, lum_floor=fm.DEFAULT_LUM_FLOOR):
    """film_denoise() with the fields of a pt_denoise_params structure."""
    return film_denoise(width, height, counts, accum, moments, guides, int(params.iterations), params.sigma_color,
                        params.sigma_depth, int(params.normal_power_log2), int(params.flags), variance, lum_floor)


def tile_reduce(tiling, err):
    """(tile_sum, tile_max) of an error plane: pt_film_tile_noise's per-tile steps."""
    return am.tile_arrays(tiling, err)


def filtered_noise(tiling, params, counts, accum, moments, guides, target, lum_floor=fm.DEFAULT_LUM_FLOOR, active_tiles=0):
    """(statistics, ferr, tile_sum, tile_max) of pt_film_filtered_noise."""
    _, ferr = film_denoise_with(params, tiling.width, tiling.height, counts, accum, moments, guides, True, lum_floor)
    tsum, tmax = tile_reduce(tiling, ferr)
    n = np.broadcast_to(np.asarray(counts, np.uint32).reshape(-1), (tiling.n_pixels,))
    return am.statistics(tiling, tsum, n, target, active_tiles), ferr, tsum, tmax


def render_until_filtered(tiling, filtered_sums_after, first, uniform_samples, dilate_by, target, max_samples, last=0, total=0):
    """pt_film_render_until_filtered: pt_film_render_until_adaptive's loop, the tile sums being those of ferr.
    filtered_sums_after(k, samples, tiles) -> tile_sum of filtered_noise() of the film after pass k."""
    return am.render_until_adaptive(tiling, filtered_sums_after, first, uniform_samples, dilate_by, target, max_samples, last, total)
