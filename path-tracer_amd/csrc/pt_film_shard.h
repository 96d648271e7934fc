// Sharded films: a shard film holds one rank's tiles of a film that shard_count ranks hold together, in the packed
// local order of pt_local_pixel_map - the rank's tiles in ascending tile number, each row-major and clipped.  Its tile kernels are
// the FilmPacked instances of the bodies in pt_film.h and pt_film_window.h (k_film_merge_tiles_packed, k_film_tile_noise_packed,
// k_film_gather_tiles_packed, k_film_scatter_tiles_packed): the same arithmetic per tile, in the same order, on pixels that are
// found at base[tile] + j.  What is here is the way back to one device:
//
//   k_film_import_shard    whole = shard for the pixels of the shard's tiles: accum (3 f32), moments (2 f32) and, where the films
//                          are non-uniform, counts (u32), from packed order into the image order of an unsharded film.  A copy,
//                          one streaming pass: lane j of a tile reads packed pixel off + j - consecutive lanes, consecutive
//                          addresses - and writes a tile row's run of the image.
#pragma once
#include "pt_film.h"

// One workgroup per tile of the shard.  table: n_list + 1 packed offsets, then the n_list tile numbers (the shard's own tile map).
// src_count and dst_count are both null (uniform films) or both set.
__global__ __launch_bounds__(256) void k_film_import_shard(const float* __restrict__ src_accum, const float2* __restrict__ src_mom,
                                                           const uint32_t* __restrict__ src_count, const uint32_t* __restrict__ table,
                                                           uint32_t n_list, FilmTiling T, float* __restrict__ dst_accum,
                                                           float2* __restrict__ dst_mom, uint32_t* __restrict__ dst_count) {
    const uint32_t lt = blockIdx.x;
    if (lt >= n_list) return;
    const FilmTile t = film_tile(T, table[n_list + 1u + lt]);
    const uint32_t off = table[lt], P = t.cw * t.ch;
    for (uint32_t j = threadIdx.x; j < P; j += 256u) {
        const size_t p = t.pixel(j, T.width), q = (size_t)off + j;
        const float r = src_accum[3 * q], g = src_accum[3 * q + 1], b = src_accum[3 * q + 2];
        const float2 m = src_mom[q];
        dst_accum[3 * p] = r;
        dst_accum[3 * p + 1] = g;
        dst_accum[3 * p + 2] = b;
        dst_mom[p] = m;
        if (src_count != nullptr) dst_count[p] = src_count[q];
    }
}
