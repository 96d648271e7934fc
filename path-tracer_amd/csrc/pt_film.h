// Progressive film: the sums of several whole frames of one view - accum and the luminance moments of
// pt_render_moments - and a noise figure made from the moments.
//
//   k_film_merge   film = film + pass over both plane pairs (accum: 3 floats per pixel, moments: 2), one f32 addition per float
//   k_film_noise   the relative standard error of every pixel's mean luminance, and its sum and maximum over every block of
//                  256 packed pixels
//   k_film_color   color = accum / (float)n (pt_film_resolve's f32 output; the u8 output is k_postprocess's)
//
// The adaptive film: a film that has taken a pass over a list of tiles keeps a sample count per pixel.
//
//   k_film_merge_tiles     film = film + pass for the pixels of the listed tiles (the pass planes are packed in list order),
//                          count = count + samples; no other pixel is read or written
//   k_film_tile_noise      k_film_noise's figure with n = the pixel's own count, summed over every TILE of the image
//   k_film_color_counts    color = accum / (float)count[p]
//   k_film_post_counts     k_postprocess with samples = count[p]
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

// ------------------------------------------------------------------ adaptive film
// The tiling of an unsharded film: tile k = ty * tiles_x + tx covers the pixels [tx tile_w, ..) x [ty tile_h, ..) clipped to the
// image - cw x ch of them, numbered j = y * cw + x.  The film's planes are in image order (p = x + y * width).
struct FilmTiling {
    uint32_t width, height, tile_w, tile_h, tiles_x;
};
struct FilmTile {
    uint32_t x0, y0, cw, ch;
    __device__ __forceinline__ uint32_t pixel(uint32_t j, uint32_t width) const { return (y0 + j / cw) * width + x0 + j % cw; }
};
__device__ __forceinline__ FilmTile film_tile(const FilmTiling& T, uint32_t k) {
    FilmTile t;
    t.x0 = (k % T.tiles_x) * T.tile_w;
    t.y0 = (k / T.tiles_x) * T.tile_h;
    t.cw = min(T.tile_w, T.width - t.x0);
    t.ch = min(T.tile_h, T.height - t.y0);
    return t;
}

// The layout of a film's planes is the template parameter of the tile kernels' bodies: FilmTiling - image order, the unsharded
// film - or FilmPacked - a shard film, whose planes hold the rank's own tiles one after the other: pixel j of tile
// k is packed pixel base[k] + j (base: one entry per tile of the IMAGE, FILM_NOT_OWNED for another rank's tile).  The
// image-order kernels are the bodies' FilmTiling instances, inlined: the code they were before the parameter existed.
enum : uint32_t { FILM_NOT_OWNED = 0xffffffffu };
struct FilmPacked {
    FilmTiling T;
    const uint32_t* base;
};
struct FilmSpan {   // where the pixels of one tile are: p(j), j < P
    FilmTile t;
    uint32_t width, base;
    template <bool PACKED>
    __device__ __forceinline__ size_t pixel(uint32_t j) const {
        if constexpr (PACKED) return (size_t)base + j;
        else return t.pixel(j, width);
    }
};
__device__ __forceinline__ const FilmTiling& film_tiling_of(const FilmTiling& T) { return T; }
__device__ __forceinline__ const FilmTiling& film_tiling_of(const FilmPacked& L) { return L.T; }
template <class L>
struct FilmLayoutIs;
template <>
struct FilmLayoutIs<FilmTiling> {
    static constexpr bool packed = false;
};
template <>
struct FilmLayoutIs<FilmPacked> {
    static constexpr bool packed = true;
};
__device__ __forceinline__ FilmSpan film_span(const FilmTiling& T, uint32_t k) { return FilmSpan{film_tile(T, k), T.width, 0u}; }
__device__ __forceinline__ FilmSpan film_span(const FilmPacked& L, uint32_t k) { return FilmSpan{film_tile(L.T, k), L.T.width, L.base[k]}; }

// One workgroup per listed tile.  table: n_list + 1 packed offsets, then the n_list tile numbers (the table of the frame that
// rendered the pass).  Pixel j of listed tile lt is packed pixel table[lt] + j of the pass planes.
template <class Layout>
__device__ __forceinline__ void film_merge_tiles_body(const float* __restrict__ pass_accum, const float2* __restrict__ pass_mom,
                                                      const uint32_t* __restrict__ table, uint32_t n_list, const Layout& T,
                                                      float* __restrict__ film_accum, float2* __restrict__ film_mom,
                                                      uint32_t* __restrict__ count, uint32_t samples) {
    constexpr bool PK = FilmLayoutIs<Layout>::packed;
    const uint32_t lt = blockIdx.x;
    const FilmSpan t = film_span(T, table[n_list + 1u + lt]);
    const uint32_t off = table[lt], P = t.t.cw * t.t.ch;
    for (uint32_t j = threadIdx.x; j < P; j += 256u) {
        const size_t p = t.template pixel<PK>(j), q = (size_t)off + j;
        film_accum[3 * p] = film_accum[3 * p] + pass_accum[3 * q];
        film_accum[3 * p + 1] = film_accum[3 * p + 1] + pass_accum[3 * q + 1];
        film_accum[3 * p + 2] = film_accum[3 * p + 2] + pass_accum[3 * q + 2];
        const float2 f = film_mom[p], m = pass_mom[q];
        film_mom[p] = make_float2(f.x + m.x, f.y + m.y);
        count[p] += samples;
    }
}
__global__ __launch_bounds__(256) void k_film_merge_tiles(const float* __restrict__ pass_accum, const float2* __restrict__ pass_mom,
                                                          const uint32_t* __restrict__ table, uint32_t n_list, FilmTiling T,
                                                          float* __restrict__ film_accum, float2* __restrict__ film_mom,
                                                          uint32_t* __restrict__ count, uint32_t samples) {
    film_merge_tiles_body(pass_accum, pass_mom, table, n_list, T, film_accum, film_mom, count, samples);
}
__global__ __launch_bounds__(256) void k_film_merge_tiles_packed(const float* __restrict__ pass_accum, const float2* __restrict__ pass_mom,
                                                                 const uint32_t* __restrict__ table, uint32_t n_list, FilmPacked T,
                                                                 float* __restrict__ film_accum, float2* __restrict__ film_mom,
                                                                 uint32_t* __restrict__ count, uint32_t samples) {
    film_merge_tiles_body(pass_accum, pass_mom, table, n_list, T, film_accum, film_mom, count, samples);
}

// One workgroup per tile of the image.  n of pixel p: count[p], or the film's uniform total `n_uniform` where count is null.
// Thread i adds the errors of the tile's pixels i, i + 256, ... to 0.f in that order; then k_film_noise's tree.  err (image
// order; the packed variant: the film's packed order) may be null.  A tile of another rank (packed variant only) gets the sum
// and the maximum 0.f: nothing of it is read.
template <class Layout>
__device__ __forceinline__ void film_tile_noise_body(const float2* __restrict__ moments, const uint32_t* __restrict__ count,
                                                     uint32_t n_uniform, const Layout& T, float lum_floor, float* __restrict__ err,
                                                     float* __restrict__ tile_sum, float* __restrict__ tile_max) {
    constexpr bool PK = FilmLayoutIs<Layout>::packed;
    __shared__ float vs[256];
    __shared__ float vm[256];
    const uint32_t i = threadIdx.x;
    const FilmSpan t = film_span(T, blockIdx.x);
    if constexpr (PK) {
        if (t.base == FILM_NOT_OWNED) {   // (the whole workgroup)
            if (i == 0u) {
                tile_sum[blockIdx.x] = 0.f;
                tile_max[blockIdx.x] = 0.f;
            }
            return;
        }
    }
    const uint32_t P = t.t.cw * t.t.ch;
    float v = 0.f, w = 0.f;
    for (uint32_t j = i; j < P; j += 256u) {
        const size_t p = t.template pixel<PK>(j);
        const uint32_t n = count != nullptr ? count[p] : n_uniform;
        const float2 m = moments[p];
        const float N = (float)n;
        const float mu = m.x / N;
        const float e2 = m.y / N;
        const float s2 = max_rs(0.f, e2 - mu * mu);
        const float vL = s2 / (float)(n - 1u);
        const float se = sqrtf(vL);
        const float den = max_rs(mu, lum_floor);
        const float e = se / den;
        if (err != nullptr) err[p] = e;
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
__global__ __launch_bounds__(256) void k_film_tile_noise(const float2* __restrict__ moments, const uint32_t* __restrict__ count,
                                                         uint32_t n_uniform, FilmTiling T, float lum_floor, float* __restrict__ err,
                                                         float* __restrict__ tile_sum, float* __restrict__ tile_max) {
    film_tile_noise_body(moments, count, n_uniform, T, lum_floor, err, tile_sum, tile_max);
}
__global__ __launch_bounds__(256) void k_film_tile_noise_packed(const float2* __restrict__ moments, const uint32_t* __restrict__ count,
                                                                uint32_t n_uniform, FilmPacked T, float lum_floor, float* __restrict__ err,
                                                                float* __restrict__ tile_sum, float* __restrict__ tile_max) {
    film_tile_noise_body(moments, count, n_uniform, T, lum_floor, err, tile_sum, tile_max);
}

__global__ __launch_bounds__(256) void k_film_color_counts(const float* __restrict__ accum, const uint32_t* __restrict__ count,
                                                           float* __restrict__ color, uint64_t n_floats) {
    for (uint64_t k = (uint64_t)blockIdx.x * 256u + threadIdx.x; k < n_floats; k += (uint64_t)gridDim.x * 256u)
        color[k] = accum[k] / (float)count[k / 3u];
}

// k_postprocess (pt_gpu.hip) with the pixel's own count for `samples`
__global__ __launch_bounds__(256) void k_film_post_counts(const float* __restrict__ accum, const uint32_t* __restrict__ count,
                                                          uint8_t* __restrict__ rgb8, uint32_t n, int tonemap_type) {
    uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    f3 c = mk3(accum[3 * (size_t)i], accum[3 * (size_t)i + 1], accum[3 * (size_t)i + 2]) / (float)count[i];
    c = tonemap(tonemap_type, c);
    rgb8[3 * (size_t)i] = as_u8(pt_pow_inv_gamma(c.x) * 255.f);
    rgb8[3 * (size_t)i + 1] = as_u8(pt_pow_inv_gamma(c.y) * 255.f);
    rgb8[3 * (size_t)i + 2] = as_u8(pt_pow_inv_gamma(c.z) * 255.f);
}
