// Temporal history: the sums of the frames of a camera path, carried from view to view by projecting every
// pixel's AOV surface point into the previous camera.
//
//   k_hist_advance   one lane per destination pixel: the surface of the new view from its AOV record, the projection into the
//                    previous view, the 2x2 footprint of taps there, the merge of the first tap that passes with the frame
//
// A history keeps two sets of planes (accum 3 f32, moments 2 f32, count u32, surf 2 x float4 per pixel); the launch reads the
// previous set and the frame, writes the next set and nothing else: no atomics, no LDS, no cross-lane traffic.  The arithmetic
// is f32, one IEEE operation per step in the order of include/ptgpu.h (pt_history_advance), compiled without contraction,
// IEEE divide and sqrt (pt_math.h); tests/history_model.py restates it bit for bit.
#pragma once
#include "pt_math.h"

struct HistView {   // the constants of one camera for the history's image size (pt_history_view)
    float c3[3];
    float M[9];     // row-major inverse of the transform's 3x3
    float tx, ty;
};

struct HistArgs {
    HistView prev;
    uint32_t width, height;
    uint32_t samples;       // N of the frame
    uint32_t max_samples;
    float normal_cos, plane_tol;
};

// Reason codes of the map.
enum : int32_t { HIST_NO_SURFACE = -1, HIST_OUTSIDE = -2, HIST_FAIL_COUNT = -3, HIST_FAIL_SURF = -4, HIST_FAIL_NORMAL = -5, HIST_FAIL_PLANE = -6 };

// 0: tap q passes; else the code of the first test it fails.
PT_D int32_t hist_tap_test(const HistArgs& H, const uint32_t* __restrict__ pc, const float4* __restrict__ ps, uint32_t q, f3 P, f3 u,
                           float dist) {
    if (!(pc[q] > 0u)) return HIST_FAIL_COUNT;
    const float4 s0 = ps[2 * (size_t)q];
    if (!(s0.w >= 0.f)) return HIST_FAIL_SURF;
    const float4 s1 = ps[2 * (size_t)q + 1];
    const float cs = (u.x * s1.x + u.y * s1.y) + u.z * s1.z;
    if (!(cs >= H.normal_cos)) return HIST_FAIL_NORMAL;
    const f3 e = mk3(s0.x - P.x, s0.y - P.y, s0.z - P.z);
    const float along = (e.x * u.x + e.y * u.y) + e.z * u.z;
    if (!(fabsf(along) <= H.plane_tol * dist)) return HIST_FAIL_PLANE;
    return 0;
}

__global__ __launch_bounds__(256) void k_hist_advance(HistArgs H, const float4* __restrict__ aov, const float* __restrict__ fa,
                                                      const float2* __restrict__ fm, const float* __restrict__ pa,
                                                      const float2* __restrict__ pm, const uint32_t* __restrict__ pc,
                                                      const float4* __restrict__ ps, float* __restrict__ na,
                                                      float2* __restrict__ nm, uint32_t* __restrict__ nc, float4* __restrict__ ns,
                                                      int32_t* __restrict__ map) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    const uint32_t W = H.width, Ht = H.height;
    if (p >= W * Ht) return;
    const float4 r0 = aov[4 * (size_t)p], r1 = aov[4 * (size_t)p + 1], r2 = aov[4 * (size_t)p + 2], r3 = aov[4 * (size_t)p + 3];
    const float cov = r1.w, fn = (float)H.samples;
    const bool valid = cov > 0.f && cov + cov >= fn;
    f3 P = mk3(0.f, 0.f, 0.f), u = mk3(0.f, 0.f, 0.f);
    float dist = -1.0f;
    int32_t prim = -1;
    if (valid) {
        P = mk3(r2.x / cov, r2.y / cov, r2.z / cov);
        dist = r0.w / cov;
        const float nn = (r0.x * r0.x + r0.y * r0.y) + r0.z * r0.z;
        if (nn > 0.f && nn < INFINITY) {
            const float inv = 1.0f / sqrtf(nn);
            u = mk3(r0.x * inv, r0.y * inv, r0.z * inv);
        }
        prim = __float_as_int(r3.z);
    }
    ns[2 * (size_t)p] = make_float4(P.x, P.y, P.z, dist);
    ns[2 * (size_t)p + 1] = make_float4(u.x, u.y, u.z, __int_as_float(prim));

    int32_t src = HIST_NO_SURFACE;
    if (valid) {
        const HistView& V = H.prev;
        const f3 v = mk3(P.x - V.c3[0], P.y - V.c3[1], P.z - V.c3[2]);
        const float qx = (V.M[0] * v.x + V.M[1] * v.y) + V.M[2] * v.z;
        const float qy = (V.M[3] * v.x + V.M[4] * v.y) + V.M[5] * v.z;
        const float qz = (V.M[6] * v.x + V.M[7] * v.y) + V.M[8] * v.z;
        const float w = -qz;
        const float fw = (float)W, fh = (float)Ht;
        src = HIST_OUTSIDE;
        if (w > 0.f) {
            const float fx = ((qx / w / V.tx + 1.f) * 0.5f) * fw;
            const float fy = ((1.f - qy / w / V.ty) * 0.5f) * fh;
            if (fx >= 0.f && fx < fw && fy >= 0.f && fy < fh) {
                const int x0 = (int)floorf(fx), y0 = (int)floorf(fy);
                const int sx = (fx - (float)x0 >= 0.5f) ? 1 : -1, sy = (fy - (float)y0 >= 0.5f) ? 1 : -1;
                // (x0, y0) is inside the image: 0 <= fx < W, and the same for fy
                const uint32_t q0 = (uint32_t)x0 + (uint32_t)y0 * W;
                src = hist_tap_test(H, pc, ps, q0, P, u, dist);
                if (src == 0) {
                    src = (int32_t)q0;
                } else {   // the footprint's other three taps, in order; the map keeps the primary tap's code when none passes
                    const int x1 = x0 + sx, y1 = y0 + sy;
                    const bool xin = x1 >= 0 && x1 < (int)W, yin = y1 >= 0 && y1 < (int)Ht;
                    const uint32_t q1 = (uint32_t)(xin ? x1 : x0) + (uint32_t)y0 * W;
                    const uint32_t q2 = (uint32_t)x0 + (uint32_t)(yin ? y1 : y0) * W;
                    const uint32_t q3 = (uint32_t)(xin ? x1 : x0) + (uint32_t)(yin ? y1 : y0) * W;
                    if (xin && hist_tap_test(H, pc, ps, q1, P, u, dist) == 0) src = (int32_t)q1;
                    else if (yin && hist_tap_test(H, pc, ps, q2, P, u, dist) == 0) src = (int32_t)q2;
                    else if (xin && yin && hist_tap_test(H, pc, ps, q3, P, u, dist) == 0) src = (int32_t)q3;
                }
            }
        }
    }

    const float2 mf = fm[p];
    const float a0 = fa[3 * (size_t)p], a1 = fa[3 * (size_t)p + 1], a2 = fa[3 * (size_t)p + 2];
    if (src >= 0) {
        const uint32_t q = (uint32_t)src;
        uint32_t c = pc[q];
        float h0 = pa[3 * (size_t)q], h1 = pa[3 * (size_t)q + 1], h2 = pa[3 * (size_t)q + 2];
        float2 hm = pm[q];
        if (c > H.max_samples) {
            const float f = (float)H.max_samples / (float)c;
            h0 = h0 * f;
            h1 = h1 * f;
            h2 = h2 * f;
            hm.x = hm.x * f;
            hm.y = hm.y * f;
            c = H.max_samples;
        }
        na[3 * (size_t)p] = h0 + a0;
        na[3 * (size_t)p + 1] = h1 + a1;
        na[3 * (size_t)p + 2] = h2 + a2;
        nm[p] = make_float2(hm.x + mf.x, hm.y + mf.y);
        nc[p] = c + H.samples;
    } else {
        na[3 * (size_t)p] = a0;
        na[3 * (size_t)p + 1] = a1;
        na[3 * (size_t)p + 2] = a2;
        nm[p] = mf;
        nc[p] = H.samples;
    }
    if (map != nullptr) map[p] = src;
}
