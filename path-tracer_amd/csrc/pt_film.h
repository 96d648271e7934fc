// Progressive film: the sums of several whole frames of one view - accum and the luminance moments of
// pt_render_moments - and a noise figure made from the moments.
//
//   k_film_merge   film = film + pass over both plane pairs (accum: 3 floats per pixel, moments: 2), one f32 addition per float
//   k_film_noise   the relative standard error of every pixel's mean luminance, and its sum and maximum over every block of
//                  256 packed pixels
//   k_film_color   color = accum / (float)n (pt_film_resolve's f32 output; the u8 output is k_postprocess's)
//
// The planes are streamed as flat floats.  Every plane starts on a 256-byte boundary and its stride is a multiple of 64
// floats (the padding is zero and stays zero: 0 + 0), so k_film_merge loads and stores whole float4s up to the padded end -
// the planes are the film's own, no caller's buffer ends inside one.
// The arithmetic is f32, one IEEE operation per step in the order of include/ptgpu.h (pt_film_noise), compiled without
// contraction, IEEE divide and sqrt (pt_math.h); tests/film_model.py restates it bit for bit.  The block sum is a fixed tree:
// strides 128 and 64 through LDS, strides 32 .. 1 inside wave 0, where __shfl_down hands lane i the value of lane i + stride -
// v[i] + v[i + stride] for every i < stride, exactly the definition's additions (the lanes above compute values nobody reads).
#pragma once
#include "pt_integrator.h"

enum { FILM_MAX_BLOCKS = 2048 };   // k_film_merge strides above this many workgroups of 256

// n4a / n4m: float4s of an accum / a moments plane (stride / 4)
__global__ __launch_bounds__(256) void k_film_merge(float4* __restrict__ film_accum, const float4* __restrict__ pass_accum,
                                                    uint64_t n4a, float4* __restrict__ film_mom,
                                                    const float4* __restrict__ pass_mom, uint64_t n4m) {
    const uint64_t n4 = n4a > n4m ? n4a : n4m;
    for (uint64_t q = (uint64_t)blockIdx.x * 256u + threadIdx.x; q < n4; q += (uint64_t)gridDim.x * 256u) {
        if (q < n4a) {
            const float4 f = film_accum[q], p = pass_accum[q];
            film_accum[q] = make_float4(f.x + p.x, f.y + p.y, f.z + p.z, f.w + p.w);
        }
        if (q < n4m) {
            const float4 f = film_mom[q], p = pass_mom[q];
            film_mom[q] = make_float4(f.x + p.x, f.y + p.y, f.z + p.z, f.w + p.w);
        }
    }
}

// One workgroup is one block of the definition: packed pixels [256 b, 256 b + 256).  n: the film's total samples (>= 2).
// err (n_local f32) may be null; block_sum / block_max have one entry per workgroup.
__global__ __launch_bounds__(256) void k_film_noise(const float2* __restrict__ moments, uint32_t n_local, uint32_t n,
                                                    float lum_floor, float* __restrict__ err, float* __restrict__ block_sum,
                                                    float* __restrict__ block_max) {
    __shared__ float vs[256];
    __shared__ float vm[256];
    const uint32_t t = threadIdx.x;
    const uint32_t p = blockIdx.x * 256u + t;
    float e = 0.f;
    if (p < n_local) {
        const float2 m = moments[p];
        const float N = (float)n;
        const float mu = m.x / N;
        const float e2 = m.y / N;
        const float s2 = max_rs(0.f, e2 - mu * mu);
        const float vL = s2 / (float)(n - 1u);
        const float se = sqrtf(vL);
        const float den = max_rs(mu, lum_floor);
        e = se / den;
        if (err != nullptr) err[p] = e;
    }
    vs[t] = e;
    vm[t] = e;
    __syncthreads();
    if (t < 128u) {
        vs[t] = vs[t] + vs[t + 128u];
        vm[t] = max_rs(vm[t], vm[t + 128u]);
    }
    __syncthreads();
    if (t < 64u) {   // wave 0
        float s = vs[t] + vs[t + 64u];
        float m = max_rs(vm[t], vm[t + 64u]);
#pragma unroll
        for (int stride = 32; stride >= 1; stride >>= 1) {
            s = s + __shfl_down(s, stride);
            m = max_rs(m, __shfl_down(m, stride));
        }
        if (t == 0u) {
            block_sum[blockIdx.x] = s;
            block_max[blockIdx.x] = m;
        }
    }
}

__global__ __launch_bounds__(256) void k_film_color(const float* __restrict__ accum, float* __restrict__ color,
                                                    uint64_t n_floats, float samples) {
    for (uint64_t k = (uint64_t)blockIdx.x * 256u + threadIdx.x; k < n_floats; k += (uint64_t)gridDim.x * 256u)
        color[k] = accum[k] / samples;
}
