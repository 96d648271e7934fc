// Windowed films: a film whose passes are windows [s0, s1) of ONE N-sample enumeration.  A window frame carries
// its sums in from the buffers it renders into (pt_render_window), so a tile window needs the listed tiles' sums in the packed
// order of the frame before it runs, and back in image order after it:
//
//   k_film_gather_tiles    pass = film for the pixels of the listed tiles (accum: 3 floats per pixel, moments: 2), packed in
//                          list order - what the window frame's first batch continues
//   k_film_scatter_tiles   film = pass for the same pixels, count = count + samples; launched only after the frame has completed
//
// Both are copies: no arithmetic on the sums, no atomics, one lane per pixel (a tile row is contiguous in both layouts).  No
// pixel outside the list is read or written.  The list table is k_film_merge_tiles' (pt_film.h), and so is the template
// parameter of the bodies: the film's layout - image order here, packed in the _packed kernels of shard films.
#pragma once
#include "pt_film.h"

// One workgroup per listed tile.  table: n_list + 1 packed offsets, then the n_list tile numbers.  Pixel j of listed tile lt
// is packed pixel table[lt] + j of the pass planes.
template <class Layout>
__device__ __forceinline__ void film_gather_tiles_body(const float* __restrict__ film_accum, const float2* __restrict__ film_mom,
                                                           const uint32_t* __restrict__ table, uint32_t n_list, const Layout& T,
                                                           float* __restrict__ pass_accum, float2* __restrict__ pass_mom) {
    constexpr bool PK = FilmLayoutIs<Layout>::packed;
    const uint32_t lt = blockIdx.x;
    if (lt >= n_list) return;
    const FilmSpan t = film_span(T, table[n_list + 1u + lt]);
    const uint32_t off = table[lt], P = t.t.cw * t.t.ch;
    for (uint32_t j = threadIdx.x; j < P; j += 256u) {
        const size_t p = t.template pixel<PK>(j), q = (size_t)off + j;
        const float r = film_accum[3 * p], g = film_accum[3 * p + 1], b = film_accum[3 * p + 2];
        const float2 m = film_mom[p];
        pass_accum[3 * q] = r;
        pass_accum[3 * q + 1] = g;
        pass_accum[3 * q + 2] = b;
        pass_mom[q] = m;
    }
}
__global__ __launch_bounds__(256) void k_film_gather_tiles(const float* __restrict__ film_accum, const float2* __restrict__ film_mom,
                                                           const uint32_t* __restrict__ table, uint32_t n_list, FilmTiling T,
                                                           float* __restrict__ pass_accum, float2* __restrict__ pass_mom) {
    film_gather_tiles_body(film_accum, film_mom, table, n_list, T, pass_accum, pass_mom);
}
__global__ __launch_bounds__(256) void k_film_gather_tiles_packed(const float* __restrict__ film_accum, const float2* __restrict__ film_mom,
                                                           const uint32_t* __restrict__ table, uint32_t n_list, FilmPacked T,
                                                           float* __restrict__ pass_accum, float2* __restrict__ pass_mom) {
    film_gather_tiles_body(film_accum, film_mom, table, n_list, T, pass_accum, pass_mom);
}

template <class Layout>
__device__ __forceinline__ void film_scatter_tiles_body(const float* __restrict__ pass_accum, const float2* __restrict__ pass_mom,
                                                            const uint32_t* __restrict__ table, uint32_t n_list, const Layout& T,
                                                            float* __restrict__ film_accum, float2* __restrict__ film_mom,
                                                            uint32_t* __restrict__ count, uint32_t samples) {
    constexpr bool PK = FilmLayoutIs<Layout>::packed;
    const uint32_t lt = blockIdx.x;
    if (lt >= n_list) return;
    const FilmSpan t = film_span(T, table[n_list + 1u + lt]);
    const uint32_t off = table[lt], P = t.t.cw * t.t.ch;
    for (uint32_t j = threadIdx.x; j < P; j += 256u) {
        const size_t p = t.template pixel<PK>(j), q = (size_t)off + j;
        const float r = pass_accum[3 * q], g = pass_accum[3 * q + 1], b = pass_accum[3 * q + 2];
        const float2 m = pass_mom[q];
        film_accum[3 * p] = r;
        film_accum[3 * p + 1] = g;
        film_accum[3 * p + 2] = b;
        film_mom[p] = m;
        count[p] += samples;
    }
}
__global__ __launch_bounds__(256) void k_film_scatter_tiles(const float* __restrict__ pass_accum, const float2* __restrict__ pass_mom,
                                                            const uint32_t* __restrict__ table, uint32_t n_list, FilmTiling T,
                                                            float* __restrict__ film_accum, float2* __restrict__ film_mom,
                                                            uint32_t* __restrict__ count, uint32_t samples) {
    film_scatter_tiles_body(pass_accum, pass_mom, table, n_list, T, film_accum, film_mom, count, samples);
}
__global__ __launch_bounds__(256) void k_film_scatter_tiles_packed(const float* __restrict__ pass_accum, const float2* __restrict__ pass_mom,
                                                            const uint32_t* __restrict__ table, uint32_t n_list, FilmPacked T,
                                                            float* __restrict__ film_accum, float2* __restrict__ film_mom,
                                                            uint32_t* __restrict__ count, uint32_t samples) {
    film_scatter_tiles_body(pass_accum, pass_mom, table, n_list, T, film_accum, film_mom, count, samples);
}
