// Per-pixel sample moments and the variance-guided a-trous filter.
//
//   k_accumulate_moments  k_accumulate (same operations, same order: the same accum bits) + the running sums of the samples'
//                         luminance and squared luminance, from the staging lines it reads anyway
//   k_samples_copy        test hook: the staged samples of one batch into the caller's planes, culled pixels filled in
//   k_dnv_prep            k_dn_prep + the variance of the pixel mean, demodulated like the colour
//   k_dnv_pass            one a-trous pass whose colour weight is a luminance difference in standard deviations of the
//                         3x3-blurred variance; the variance is filtered with the squared weights and ping-pongs with x
//
// The arithmetic is f32, one IEEE operation per step in the order of include/ptgpu.h (pt_render_moments, pt_denoise_var), so
// that tests/denoise_var_model.py can restate it bit for bit; compiled without contraction, IEEE divide and sqrt (pt_math.h).
//
// Planes of the filter (the scratch of pt_denoise, used differently): X = (x.r, x.g, x.b, v) ping-pongs, v = -1 marks an
// invalid pixel (a variance is never negative; an invalid pixel's variance is never read); U = (u.x, u.y, u.z, z) is
// constant.  A tap is two 16-byte loads, as in k_dn_pass: a wavefront's row of 32 pixels is 512 contiguous bytes per plane.
#pragma once
#include "pt_denoise.h"

PT_D float pv_lum(f3 a) { return (0.2126f * a.x + 0.7152f * a.y) + 0.0722f * a.z; }

// ------------------------------------------------------------------ moments
__global__ __launch_bounds__(256) void k_accumulate_moments(const float* __restrict__ staging, float* __restrict__ accum,
                                                            float2* __restrict__ moments, uint32_t n_local, uint32_t batch,
                                                            int first, const uint8_t* __restrict__ pixel_empty, float bg_r,
                                                            float bg_g, float bg_b) {
    uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= n_local) return;
    f3 acc = mk3(0.f, 0.f, 0.f);
    float m1 = 0.f, m2 = 0.f;
    if (!first) {
        acc = mk3(accum[3 * (size_t)p], accum[3 * (size_t)p + 1], accum[3 * (size_t)p + 2]);
        const float2 m = moments[p];
        m1 = m.x;
        m2 = m.y;
    }
    if (pixel_empty != nullptr && pixel_empty[p]) {
        // camera-grid cull: the value k_accumulate adds for the pixel, once per sample
        const f3 c = mk3(0.f, 0.f, 0.f) + mul_ew(mk3(1.f, 1.f, 1.f), mk3(bg_r, bg_g, bg_b));
        const float L = pv_lum(c);
        for (uint32_t s = 0; s < batch; ++s) {
            acc = acc + c;
            m1 = m1 + L;
            m2 = m2 + L * L;
        }
    } else {
        for (uint32_t s = 0; s < batch; ++s) {
            const float* v = staging + ((size_t)s * n_local + p) * 3;
            const f3 c = mk3(v[0], v[1], v[2]);
            const float L = pv_lum(c);
            acc = acc + c;
            m1 = m1 + L;
            m2 = m2 + L * L;
        }
    }
    accum[3 * (size_t)p] = acc.x;
    accum[3 * (size_t)p + 1] = acc.y;
    accum[3 * (size_t)p + 2] = acc.z;
    moments[p] = make_float2(m1, m2);
}

// samples: the planes of the whole frame, sample s of packed pixel p at (s * n_local + p) * 3; this batch starts at s0
__global__ __launch_bounds__(256) void k_samples_copy(const float* __restrict__ staging, float* __restrict__ samples,
                                                      uint32_t n_local, uint32_t batch, uint32_t s0,
                                                      const uint8_t* __restrict__ pixel_empty, float bg_r, float bg_g, float bg_b) {
    uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= n_local) return;
    const bool empty = pixel_empty != nullptr && pixel_empty[p];
    const f3 bg = mk3(0.f, 0.f, 0.f) + mul_ew(mk3(1.f, 1.f, 1.f), mk3(bg_r, bg_g, bg_b));
    for (uint32_t s = 0; s < batch; ++s) {
        const float* v = staging + ((size_t)s * n_local + p) * 3;
        const f3 c = empty ? bg : mk3(v[0], v[1], v[2]);
        float* o = samples + ((size_t)(s0 + s) * n_local + p) * 3;
        o[0] = c.x;
        o[1] = c.y;
        o[2] = c.z;
    }
}

// ------------------------------------------------------------------ filter
struct DnvParams {
    float sigma_depth;
    float sigma_lum;   // sigma_color: the luminance sigma in standard deviations
    uint32_t npow;     // normal_power_log2
};

__global__ __launch_bounds__(256) void k_dnv_prep(const float* __restrict__ accum, const float2* __restrict__ moments,
                                                  const float4* __restrict__ guides, uint32_t width, uint32_t height,
                                                  uint32_t samples, uint32_t no_demod, float4* __restrict__ X,
                                                  float4* __restrict__ U, float2* __restrict__ G, float* __restrict__ D) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= width * height) return;
    const uint32_t x = i % width, y = i / width;
    const float4 g0 = guides[2 * (size_t)i], g1 = guides[2 * (size_t)i + 1];
    const float N = (float)samples;
    const f3 c = mk3(accum[3 * (size_t)i], accum[3 * (size_t)i + 1], accum[3 * (size_t)i + 2]) / N;
    const float z = g0.w;
    if (!(z >= 0.f)) {   // no hit: the pixel keeps c and is never a tap
        X[i] = make_float4(c.x, c.y, c.z, -1.0f);
        U[i] = make_float4(0.f, 0.f, 0.f, -1.0f);
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
    const float2 m = moments[i];
    const float mu = m.x / N, e2 = m.y / N;
    const float s2 = max_rs(0.f, e2 - mu * mu);
    float v = s2 / (float)(samples - 1u);
    f3 d = mk3(1.f, 1.f, 1.f), xc = c;
    if (!no_demod) {
        d = mk3(g1.x + 0.01f, g1.y + 0.01f, g1.z + 0.01f);
        xc = div_ew(c, d);
        const float ld = pv_lum(d);
        v = v / (ld * ld);
    }
    float zxm = -1.f, zxp = -1.f, zym = -1.f, zyp = -1.f;
    if (x > 0u) zxm = guides[2 * (size_t)(i - 1u)].w;
    if (x + 1u < width) zxp = guides[2 * (size_t)(i + 1u)].w;
    if (y > 0u) zym = guides[2 * (size_t)(i - width)].w;
    if (y + 1u < height) zyp = guides[2 * (size_t)(i + width)].w;
    const float gx = dn_slope(z, zxm >= 0.f, zxm, zxp >= 0.f, zxp);
    const float gy = dn_slope(z, zym >= 0.f, zym, zyp >= 0.f, zyp);
    X[i] = make_float4(xc.x, xc.y, xc.z, v);
    U[i] = make_float4(u.x, u.y, u.z, z);
    G[i] = make_float2(gx, gy);
    D[3 * (size_t)i] = d.x;
    D[3 * (size_t)i + 1] = d.y;
    D[3 * (size_t)i + 2] = d.z;
}

__global__ __launch_bounds__(256) void k_dnv_pass(const float4* __restrict__ X, const float4* __restrict__ U,
                                                  const float2* __restrict__ G, float4* __restrict__ Y, int width, int height,
                                                  int step, DnvParams P) {
    const int tx = (int)(threadIdx.x & (DN_TILE_W - 1)), ty = (int)(threadIdx.x / DN_TILE_W);
    const int px = (int)blockIdx.x * DN_TILE_W + tx, py = (int)blockIdx.y * DN_TILE_H + ty;
    if (px >= width || py >= height) return;
    const size_t p = (size_t)py * (size_t)width + (size_t)px;
    const float4 xp4 = X[p];
    if (!(xp4.w >= 0.f)) {
        Y[p] = xp4;
        return;
    }
    const float4 up4 = U[p];
    const float2 g = G[p];
    const f3 xp = mk3(xp4.x, xp4.y, xp4.z), up = mk3(up4.x, up4.y, up4.z);
    const float zp = up4.w, lp = pv_lum(xp);
    // the variance, blurred 3x3 at unit spacing over the valid pixels
    const float gk[3] = {0.25f, 0.125f, 0.0625f};
    float b = 0.f, bs = 0.f;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy) {
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
            const int qx = px + dx, qy = py + dy;
            if (qx < 0 || qx >= width || qy < 0 || qy >= height) continue;
            const float vq = (dx == 0 && dy == 0) ? xp4.w : X[(size_t)qy * (size_t)width + (size_t)qx].w;
            if (!(vq >= 0.f)) continue;
            const float gw = gk[(dx < 0 ? -dx : dx) + (dy < 0 ? -dy : dy)];
            b = b + vq * gw;
            bs = bs + gw;
        }
    }
    const float vb = b / bs;
    const float lden = P.sigma_lum * sqrtf(vb) + 1e-6f;
    const float hk[3] = {0.375f, 0.25f, 0.0625f};
    f3 acc = mk3(0.f, 0.f, 0.f);
    float wsum = 0.f, vacc = 0.f;
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy) {
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            const int ax = dx < 0 ? -dx : dx, ay = dy < 0 ? -dy : dy;
            const float k = hk[ax] * hk[ay];
            float4 xq4 = xp4;
            float w = k;
            if (dx != 0 || dy != 0) {
                const int qx = px + step * dx, qy = py + step * dy;
                if (qx < 0 || qx >= width || qy < 0 || qy >= height) continue;
                const size_t q = (size_t)qy * (size_t)width + (size_t)qx;
                xq4 = X[q];
                if (!(xq4.w >= 0.f)) continue;
                const float4 uq4 = U[q];
                float wn = max_rs(0.f, dot3(up, mk3(uq4.x, uq4.y, uq4.z)));
                for (uint32_t j = 0; j < P.npow; ++j) wn = wn * wn;
                const float den = P.sigma_depth * (g.x * (float)(step * ax) + g.y * (float)(step * ay)) + 1e-4f * zp;
                const float wz = dn_wexp(fabsf(zp - uq4.w) / den);
                const float wl = dn_wexp(fabsf(lp - pv_lum(mk3(xq4.x, xq4.y, xq4.z))) / lden);
                w = ((k * wn) * wz) * wl;
            }
            acc = acc + mk3(xq4.x, xq4.y, xq4.z) * w;
            wsum = wsum + w;
            vacc = vacc + xq4.w * (w * w);
        }
    }
    const f3 o = acc / wsum;
    Y[p] = make_float4(o.x, o.y, o.z, vacc / (wsum * wsum));
}
