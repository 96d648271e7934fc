// Denoised previews: the first-hit guide planes and an edge-avoiding a-trous wavelet filter (Dammertz et al. 2010).
//
//   k_guides      first hit of the pixel-centre ray at float precision (what k_debug quantises): 8 f32 per pixel
//   k_dn_prep     accum / samples, demodulated by the albedo; unit normals; depth slopes
//   k_dn_pass<S>  one a-trous pass (5x5 taps, step s); S = 0 gathers every tap from global memory, S = 1 / 2 is the
//                 pass of step S from an LDS tile with a 2*S halo
//   k_dn_finish   remodulation, f32 colour and / or tone-mapped rgb8
//
// The arithmetic is f32, one IEEE operation per step in the order of include/ptgpu.h (pt_denoise) and no transcendental
// function, so that tests/denoise_model.py can restate it bit for bit; the file is compiled without contraction
// (pt_math.h).  The tap order (dy outer, dx inner) is part of that contract: both forms of k_dn_pass keep it.
#pragma once
#include "pt_integrator.h"

// ------------------------------------------------------------------ guides
__global__ __launch_bounds__(256) void k_guides(DevScene S, uint32_t width, uint32_t height, float4* __restrict__ guides) {
    uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= width * height) return;
    uint32_t x = i % width, y = i / width;
    f3 o, d;
    primary_ray(S, x, y, width, height, 0.5f, 0.5f, o, d);
    LocalCtr lc = {0, 0, 0, 0, 0, 0};
    RawHit h;
    float4 a = make_float4(0.f, 0.f, 0.f, -1.0f), b = make_float4(0.f, 0.f, 0.f, __int_as_float(-1));
    if (next_hit<false>(S, o, d, -INFINITY, 0u, h, lc)) {
        Surface sf;
        make_surface(S, o, d, h, sf);
        MatSample ms;
        material_sample(S, sf.model, sf.sphere, sf.uv, ms);
        f3 n = shading_normal(S, sf);
        a = make_float4(n.x, n.y, n.z, h.key);
        b = make_float4(ms.albedo.x, ms.albedo.y, ms.albedo.z, __int_as_float((int32_t)PT_PRIM_INDEX(h.pid)));
    }
    guides[2 * (size_t)i] = a;
    guides[2 * (size_t)i + 1] = b;
}

// ------------------------------------------------------------------ filter
struct DnParams {
    float sigma_depth;
    float sc2;          // (sigma_color * 2^-pass)^2
    uint32_t npow;      // normal_power_log2
    uint32_t color_on;  // sigma_color != 0
};

enum { DN_TILE_W = 32, DN_TILE_H = 8 };  // pixels per 256-lane workgroup of k_dn_pass

// compact-support stand-in for exp(-e): max(0, 1 - e/8)^8; a NaN or +inf argument gives 0
PT_D float dn_wexp(float e) {
    float r = max_rs(0.f, 1.f - e * 0.125f);
    r = r * r;
    r = r * r;
    r = r * r;
    return r;
}

// |z(a) - z(b)| of the valid in-image neighbours on one axis: the smaller of the two, the only one, or 0
PT_D float dn_slope(float z, bool has_m, float zm, bool has_p, float zp) {
    const float dm = fabsf(z - zm), dp = fabsf(zp - z);
    if (has_m && has_p) return fminf(dp, dm);
    if (has_p) return dp;
    if (has_m) return dm;
    return 0.f;
}

__global__ __launch_bounds__(256) void k_dn_prep(const float* __restrict__ accum, const float4* __restrict__ guides,
                                                 uint32_t width, uint32_t height, uint32_t samples, uint32_t no_demod,
                                                 float4* __restrict__ X, float4* __restrict__ U, float2* __restrict__ G,
                                                 float* __restrict__ D) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= width * height) return;
    const uint32_t x = i % width, y = i / width;
    const float4 g0 = guides[2 * (size_t)i], g1 = guides[2 * (size_t)i + 1];
    const f3 c = mk3(accum[3 * (size_t)i], accum[3 * (size_t)i + 1], accum[3 * (size_t)i + 2]) / (float)samples;
    const float z = g0.w;
    if (!(z >= 0.f)) {   // no hit: the pixel keeps c and is never a tap
        X[i] = make_float4(c.x, c.y, c.z, -1.0f);
        U[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        G[i] = make_float2(0.f, 0.f);
        D[3 * (size_t)i] = 1.f;
        D[3 * (size_t)i + 1] = 1.f;
        D[3 * (size_t)i + 2] = 1.f;
        return;
    }
    const f3 n = mk3(g0.x, g0.y, g0.z);
    const float nn = dot3(n, n);
    f3 u = mk3(0.f, 0.f, 0.f);
    if (nn > 0.f && nn < INFINITY) u = normalize3(n);
    f3 d = mk3(1.f, 1.f, 1.f), xc = c;
    if (!no_demod) {
        d = mk3(g1.x + 0.01f, g1.y + 0.01f, g1.z + 0.01f);
        xc = div_ew(c, d);
    }
    float zxm = -1.f, zxp = -1.f, zym = -1.f, zyp = -1.f;
    if (x > 0u) zxm = guides[2 * (size_t)(i - 1u)].w;
    if (x + 1u < width) zxp = guides[2 * (size_t)(i + 1u)].w;
    if (y > 0u) zym = guides[2 * (size_t)(i - width)].w;
    if (y + 1u < height) zyp = guides[2 * (size_t)(i + width)].w;
    const float gx = dn_slope(z, zxm >= 0.f, zxm, zxp >= 0.f, zxp);
    const float gy = dn_slope(z, zym >= 0.f, zym, zyp >= 0.f, zyp);
    X[i] = make_float4(xc.x, xc.y, xc.z, z);
    U[i] = make_float4(u.x, u.y, u.z, 0.f);
    G[i] = make_float2(gx, gy);
    D[3 * (size_t)i] = d.x;
    D[3 * (size_t)i + 1] = d.y;
    D[3 * (size_t)i + 2] = d.z;
}

// The weight of one tap that is not the centre.
PT_D float dn_tap_weight(const DnParams& P, float k, f3 up, f3 uq, f3 xp, f3 xq, float zp, float zq, float gx, float gy,
                         int sdx, int sdy) {
    float wn = max_rs(0.f, dot3(up, uq));
    for (uint32_t j = 0; j < P.npow; ++j) wn = wn * wn;
    const float den = P.sigma_depth * (gx * (float)sdx + gy * (float)sdy) + 1e-4f * zp;
    const float wz = dn_wexp(fabsf(zp - zq) / den);
    float wc = 1.f;
    if (P.color_on) {
        const f3 dl = xp - xq;
        wc = dn_wexp(dot3(dl, dl) / P.sc2);
    }
    return ((k * wn) * wz) * wc;
}

template <int S>
__global__ __launch_bounds__(256) void k_dn_pass(const float4* __restrict__ X, const float4* __restrict__ U,
                                                 const float2* __restrict__ G, float4* __restrict__ Y, int width, int height,
                                                 int step, DnParams P) {
    constexpr int HALO = 2 * S, TW = DN_TILE_W + 2 * HALO, TH = DN_TILE_H + 2 * HALO;
    __shared__ float4 tile_x[S ? TW * TH : 1];
    __shared__ float4 tile_u[S ? TW * TH : 1];
    const int tx = (int)(threadIdx.x & (DN_TILE_W - 1)), ty = (int)(threadIdx.x / DN_TILE_W);
    const int x0 = (int)blockIdx.x * DN_TILE_W, y0 = (int)blockIdx.y * DN_TILE_H;
    const int px = x0 + tx, py = y0 + ty;
    if (S) {
        // the tile and its halo; what lies outside the image is stored as an invalid pixel (z < 0): skipped like one
        for (int e = (int)threadIdx.x; e < TW * TH; e += 256) {
            const int qx = x0 - HALO + e % TW, qy = y0 - HALO + e / TW;
            float4 xq = make_float4(0.f, 0.f, 0.f, -1.0f), uq = make_float4(0.f, 0.f, 0.f, 0.f);
            if (qx >= 0 && qx < width && qy >= 0 && qy < height) {
                const size_t q = (size_t)qy * (size_t)width + (size_t)qx;
                xq = X[q];
                if (xq.w >= 0.f) uq = U[q];
            }
            tile_x[e] = xq;
            tile_u[e] = uq;
        }
        __syncthreads();
        step = S;
    }
    if (px >= width || py >= height) return;
    const size_t p = (size_t)py * (size_t)width + (size_t)px;
    const float4 xp4 = S ? tile_x[(ty + HALO) * TW + tx + HALO] : X[p];
    if (!(xp4.w >= 0.f)) {
        Y[p] = xp4;
        return;
    }
    const float4 up4 = S ? tile_u[(ty + HALO) * TW + tx + HALO] : U[p];
    const float2 g = G[p];
    const f3 xp = mk3(xp4.x, xp4.y, xp4.z), up = mk3(up4.x, up4.y, up4.z);
    const float zp = xp4.w;
    const float hk[3] = {0.375f, 0.25f, 0.0625f};
    f3 acc = mk3(0.f, 0.f, 0.f);
    float wsum = 0.f;
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy) {
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            const int ax = dx < 0 ? -dx : dx, ay = dy < 0 ? -dy : dy;
            const float k = hk[ax] * hk[ay];
            float4 xq4, uq4 = make_float4(0.f, 0.f, 0.f, 0.f);
            if (dx == 0 && dy == 0) {
                xq4 = xp4;
            } else if (S) {
                const int e = (ty + HALO + S * dy) * TW + tx + HALO + S * dx;
                xq4 = tile_x[e];
                if (!(xq4.w >= 0.f)) continue;
                uq4 = tile_u[e];
            } else {
                const int qx = px + step * dx, qy = py + step * dy;
                if (qx < 0 || qx >= width || qy < 0 || qy >= height) continue;
                const size_t q = (size_t)qy * (size_t)width + (size_t)qx;
                xq4 = X[q];
                if (!(xq4.w >= 0.f)) continue;
                uq4 = U[q];
            }
            const f3 xq = mk3(xq4.x, xq4.y, xq4.z);
            float w = k;
            if (dx != 0 || dy != 0)
                w = dn_tap_weight(P, k, up, mk3(uq4.x, uq4.y, uq4.z), xp, xq, zp, xq4.w, g.x, g.y, step * ax, step * ay);
            acc = acc + xq * w;
            wsum = wsum + w;
        }
    }
    const f3 o = acc / wsum;
    Y[p] = make_float4(o.x, o.y, o.z, zp);
}

// X == nullptr: no filtering at all (iterations = 0), out = accum / samples
__global__ __launch_bounds__(256) void k_dn_finish(const float4* __restrict__ X, const float* __restrict__ D,
                                                   const float* __restrict__ accum, uint32_t samples, uint32_t n,
                                                   uint32_t no_demod, int tonemap_type, float* __restrict__ out_color,
                                                   uint8_t* __restrict__ out_rgb8) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    f3 o;
    if (X == nullptr) {
        o = mk3(accum[3 * (size_t)i], accum[3 * (size_t)i + 1], accum[3 * (size_t)i + 2]) / (float)samples;
    } else {
        const float4 x = X[i];
        o = mk3(x.x, x.y, x.z);
        if (x.w >= 0.f && !no_demod) o = mul_ew(o, mk3(D[3 * (size_t)i], D[3 * (size_t)i + 1], D[3 * (size_t)i + 2]));
    }
    if (out_color != nullptr) {
        out_color[3 * (size_t)i] = o.x;
        out_color[3 * (size_t)i + 1] = o.y;
        out_color[3 * (size_t)i + 2] = o.z;
    }
    if (out_rgb8 != nullptr) {
        const f3 c = tonemap(tonemap_type, o);
        out_rgb8[3 * (size_t)i] = as_u8(pt_pow_inv_gamma(c.x) * 255.f);
        out_rgb8[3 * (size_t)i + 1] = as_u8(pt_pow_inv_gamma(c.y) * 255.f);
        out_rgb8[3 * (size_t)i + 2] = as_u8(pt_pow_inv_gamma(c.z) * 255.f);
    }
}
