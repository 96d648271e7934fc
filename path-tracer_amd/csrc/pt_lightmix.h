// Light mixer: a frame is linear in every light's colour, so a view whose lights only change colour is
//     accum = E + sum_l f_l (x) D_l        per channel, f_l = colour_l / unit_l
// over planes captured once (pt_lightmix_capture): E the frame with every light black, D_l the frame of light l alone at
// (unit_l, unit_l, unit_l) minus E.
//
//   k_lightmix_diff    D = F - E over one plane, in place (the capture's subtraction)
//   k_lightmix_apply   the mix: one float4 of every plane per lane, one float4 of accum and four u8 out
//
// Every step - tone maps included - is per channel, so the planes are streamed as flat floats: float k of a plane has channel
// k mod 3, and the float4 q (floats 4q .. 4q+3) has channels (q, q+1, q+2, q) mod 3.  A plane starts on a 256-byte boundary
// and its stride is a multiple of 4 floats (the padding is zero), so every lane's loads are 16 bytes wide and the last,
// partial float4 of a plane is loaded like any other; only the STORES of that last float4 are element by element, because the
// caller's buffers end where the image ends.  The factors travel in the kernel arguments; the light loop is wave-uniform.
// The arithmetic is f32, one IEEE operation per step in the order of include/ptgpu.h (pt_lightmix_apply), compiled without
// contraction (pt_math.h); tests/lightmix_model.py restates it bit for bit.
#pragma once
#include "pt_integrator.h"

struct LmFactors {
    float f[PT_LIGHTMIX_MAX_LIGHTS][3];
};

enum { LM_MAX_BLOCKS = 2048 };   // grid-stride above this many workgroups of 256

// n4: float4s of one plane (stride / 4)
__global__ __launch_bounds__(256) void k_lightmix_diff(float4* __restrict__ D, const float4* __restrict__ E, uint64_t n4) {
    for (uint64_t q = (uint64_t)blockIdx.x * 256u + threadIdx.x; q < n4; q += (uint64_t)gridDim.x * 256u) {
        const float4 f = D[q], e = E[q];
        D[q] = make_float4(f.x - e.x, f.y - e.y, f.z - e.z, f.w - e.w);
    }
}

// k_postprocess's arithmetic on one channel
PT_D uint32_t lm_u8(int tonemap_type, float a, float samples) {
    const float c = a / samples;
    const float t = tonemap(tonemap_type, mk3(c, c, c)).x;
    return (uint32_t)as_u8(pt_pow_inv_gamma(t) * 255.f);
}

// planes: plane 0 = E, plane 1 + l = D_l, `stride` floats apart; n_floats = 3 * n_local.  accum (16-byte aligned) and rgb8
// (4-byte aligned): either may be null.
__global__ __launch_bounds__(256) void k_lightmix_apply(const float* __restrict__ planes, uint64_t stride, uint32_t n_lights,
                                                        LmFactors F, uint64_t n_floats, uint32_t samples, int tonemap_type,
                                                        float* __restrict__ accum, uint8_t* __restrict__ rgb8) {
    const uint64_t n4 = (n_floats + 3u) / 4u;
    const float fs = (float)samples;
    for (uint64_t q = (uint64_t)blockIdx.x * 256u + threadIdx.x; q < n4; q += (uint64_t)gridDim.x * 256u) {
        const uint32_t c = (uint32_t)(q % 3u);   // channel of the float4's first float
        float4 a = *(const float4*)(planes + 4u * q);
#pragma unroll
        for (uint32_t l = 0; l < PT_LIGHTMIX_MAX_LIGHTS; ++l) {
            if (l >= n_lights) break;
            const float r = F.f[l][0], g = F.f[l][1], b = F.f[l][2];
            const float f0 = c == 0u ? r : (c == 1u ? g : b);
            const float f1 = c == 0u ? g : (c == 1u ? b : r);
            const float f2 = c == 0u ? b : (c == 1u ? r : g);
            const float4 d = *(const float4*)(planes + (uint64_t)(l + 1u) * stride + 4u * q);
            a.x = a.x + f0 * d.x;
            a.y = a.y + f1 * d.y;
            a.z = a.z + f2 * d.z;
            a.w = a.w + f0 * d.w;
        }
        const uint64_t k = 4u * q;
        const bool whole = k + 4u <= n_floats;
        if (accum != nullptr) {
            if (whole) {
                *(float4*)(accum + k) = a;
            } else {
                accum[k] = a.x;
                if (k + 1u < n_floats) accum[k + 1u] = a.y;
                if (k + 2u < n_floats) accum[k + 2u] = a.z;
            }
        }
        if (rgb8 != nullptr) {
            const uint32_t u0 = lm_u8(tonemap_type, a.x, fs), u1 = lm_u8(tonemap_type, a.y, fs);
            const uint32_t u2 = lm_u8(tonemap_type, a.z, fs), u3 = lm_u8(tonemap_type, a.w, fs);
            if (whole) {
                *(uint32_t*)(rgb8 + k) = u0 | (u1 << 8) | (u2 << 16) | (u3 << 24);
            } else {
                rgb8[k] = (uint8_t)u0;
                if (k + 1u < n_floats) rgb8[k + 1u] = (uint8_t)u1;
                if (k + 2u < n_floats) rgb8[k + 2u] = (uint8_t)u2;
            }
        }
    }
}
