// Film filter: the a-trous filters of pt_denoise.h / pt_variance.h on a film's own planes, where every pixel may
// have its own sample count, and the error figure of the filtered mean.
//
//   k_fdn_prep<VAR>      k_dn_prep (VAR = 0) / k_dnv_prep (VAR = 1) with the pixel's own count for `samples`; the same X / U /
//                        G / D planes, so k_dn_pass and k_dnv_pass run on them unmodified
//   k_fdn_finish         k_dn_finish of the variance filter + ferr: the relative standard error of the FILTERED mean
//                        luminance from the variance the last pass left in X.w; pt_film_noise's raw err where nothing was
//                        filtered (an invalid pixel, iterations = 0)
//   k_film_tile_reduce   k_film_tile_noise's sums and maxima per tile over an error plane that exists already
//
// `count` is the film's u32 count plane, or null on a uniform film: then every pixel has `n_uniform` samples.  The planes
// are in image order (an unsharded film).  The arithmetic is f32, one IEEE operation per step in the order of
// include/ptgpu.h (pt_film_denoise), compiled without contraction, IEEE divide and sqrt (pt_math.h);
// tests/film_denoise_model.py restates it bit for bit.
#pragma once
#include "pt_film.h"
#include "pt_variance.h"

template <int VAR>
__global__ __launch_bounds__(256) void k_fdn_prep(const float* __restrict__ accum, const float2* __restrict__ moments,
                                                  const uint32_t* __restrict__ count, uint32_t n_uniform,
                                                  const float4* __restrict__ guides, uint32_t width, uint32_t height,
                                                  uint32_t no_demod, float4* __restrict__ X, float4* __restrict__ U,
                                                  float2* __restrict__ G, float* __restrict__ D) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= width * height) return;
    const uint32_t x = i % width, y = i / width;
    const float4 g0 = guides[2 * (size_t)i], g1 = guides[2 * (size_t)i + 1];
    const uint32_t samples = count != nullptr ? count[i] : n_uniform;
    const float N = (float)samples;
    const f3 c = mk3(accum[3 * (size_t)i], accum[3 * (size_t)i + 1], accum[3 * (size_t)i + 2]) / N;
    const float z = g0.w;
    if (!(z >= 0.f)) {   // no hit: the pixel keeps c and is never a tap
        X[i] = make_float4(c.x, c.y, c.z, -1.0f);
        U[i] = make_float4(0.f, 0.f, 0.f, VAR ? -1.0f : 0.f);
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
    float v = 0.f;
    if (VAR) {
        const float2 m = moments[i];
        const float mu = m.x / N, e2 = m.y / N;
        const float s2 = max_rs(0.f, e2 - mu * mu);
        v = s2 / (float)(samples - 1u);
    }
    f3 d = mk3(1.f, 1.f, 1.f), xc = c;
    if (!no_demod) {
        d = mk3(g1.x + 0.01f, g1.y + 0.01f, g1.z + 0.01f);
        xc = div_ew(c, d);
        if (VAR) {
            const float ld = pv_lum(d);
            v = v / (ld * ld);
        }
    }
    float zxm = -1.f, zxp = -1.f, zym = -1.f, zyp = -1.f;
    if (x > 0u) zxm = guides[2 * (size_t)(i - 1u)].w;
    if (x + 1u < width) zxp = guides[2 * (size_t)(i + 1u)].w;
    if (y > 0u) zym = guides[2 * (size_t)(i - width)].w;
    if (y + 1u < height) zyp = guides[2 * (size_t)(i + width)].w;
    const float gx = dn_slope(z, zxm >= 0.f, zxm, zxp >= 0.f, zxp);
    const float gy = dn_slope(z, zym >= 0.f, zym, zyp >= 0.f, zyp);
    X[i] = make_float4(xc.x, xc.y, xc.z, VAR ? v : z);
    U[i] = make_float4(u.x, u.y, u.z, VAR ? z : 0.f);
    G[i] = make_float2(gx, gy);
    D[3 * (size_t)i] = d.x;
    D[3 * (size_t)i + 1] = d.y;
    D[3 * (size_t)i + 2] = d.z;
}

// The finish of the variance filter with its error output.  X == nullptr: nothing was filtered (iterations = 0): out = accum /
// count and ferr is the raw err for every pixel.  out_color, out_rgb8 and ferr may each be null.
__global__ __launch_bounds__(256) void k_fdn_finish(const float4* __restrict__ X, const float* __restrict__ D,
                                                    const float* __restrict__ accum, const float2* __restrict__ moments,
                                                    const uint32_t* __restrict__ count, uint32_t n_uniform, uint32_t n,
                                                    uint32_t no_demod, int tonemap_type, float lum_floor,
                                                    float* __restrict__ out_color, uint8_t* __restrict__ out_rgb8,
                                                    float* __restrict__ ferr) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint32_t samples = count != nullptr ? count[i] : n_uniform;
    f3 o;
    float vf = -1.0f;   // the variance of the filtered mean; negative: the pixel was not filtered
    if (X == nullptr) {
        o = mk3(accum[3 * (size_t)i], accum[3 * (size_t)i + 1], accum[3 * (size_t)i + 2]) / (float)samples;
    } else {
        const float4 x = X[i];
        o = mk3(x.x, x.y, x.z);
        if (x.w >= 0.f) {
            vf = x.w;
            if (!no_demod) {
                const f3 d = mk3(D[3 * (size_t)i], D[3 * (size_t)i + 1], D[3 * (size_t)i + 2]);
                o = mul_ew(o, d);
                const float ld = pv_lum(d);
                vf = vf * (ld * ld);
            }
        }
    }
    if (ferr != nullptr) {
        float e;
        if (vf >= 0.f) {
            const float se = sqrtf(vf);
            const float den = max_rs(pv_lum(o), lum_floor);
            e = se / den;
        } else {   // pt_film_noise's err with n = the pixel's count
            const float2 m = moments[i];
            const float N = (float)samples;
            const float mu = m.x / N;
            const float e2 = m.y / N;
            const float s2 = max_rs(0.f, e2 - mu * mu);
            const float vL = s2 / (float)(samples - 1u);
            const float se = sqrtf(vL);
            const float den = max_rs(mu, lum_floor);
            e = se / den;
        }
        ferr[i] = e;
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

// One workgroup per tile of the image: k_film_tile_noise's gather and tree over err (image order), which is only read.
__global__ __launch_bounds__(256) void k_film_tile_reduce(const float* __restrict__ err, FilmTiling T,
                                                          float* __restrict__ tile_sum, float* __restrict__ tile_max) {
    __shared__ float vs[256];
    __shared__ float vm[256];
    const uint32_t i = threadIdx.x;
    const FilmTile t = film_tile(T, blockIdx.x);
    const uint32_t P = t.cw * t.ch;
    float v = 0.f, w = 0.f;
    for (uint32_t j = i; j < P; j += 256u) {
        const float e = err[t.pixel(j, T.width)];
        v = v + e;
        w = max_rs(w, e);
    }
    vs[i] = v;
    vm[i] = w;
    __syncthreads();
    if (i < 128u) {
        vs[i] = vs[i] + vs[i + 128u];
        vm[i] = max_rs(vm[i], vm[i + 128u]);
    }
    __syncthreads();
    if (i < 64u) {   // wave 0
        float s = vs[i] + vs[i + 64u];
        float m = max_rs(vm[i], vm[i + 64u]);
#pragma unroll
        for (int stride = 32; stride >= 1; stride >>= 1) {
            s = s + __shfl_down(s, stride);
            m = max_rs(m, __shfl_down(m, stride));
        }
        if (i == 0u) {
            tile_sum[blockIdx.x] = s;
            tile_max[blockIdx.x] = m;
        }
    }
}
