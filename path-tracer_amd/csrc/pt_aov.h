// Sample-coherent AOVs: the camera cast and the alpha walk of every sample of the frame, replayed - same
// generator, same jitter, same draws as render_pixel (mod.rs:107-124, 182-205) - and nothing after it; the features of the
// surfaces the walks stop at, summed per pixel.
//
//   k_aov<ALPHA, GRID>          one lane per (pixel, sample), the samples of a pixel in consecutive lanes of one wavefront;
//                               the pixel record (16 f32) is reduced across those lanes and stored by the segment's first lane
//   k_aov_samples<ALPHA, GRID>  the per-sample records themselves (test hook): N planes of n_local x 16 f32
//   k_aov_guides                pixel records -> the 8-float guide layout of k_guides (pt_denoise.h)
//
// The arithmetic is f32, one IEEE operation per step in the order of include/ptgpu.h (pt_render_aov); the file is compiled
// without contraction (pt_math.h); tests/aov_model.py restates the sums and the guide rule bit for bit.  The kernels read
// the scene (DevScene) and, sharded, the frame's tile table; they read no frame cache and write nothing but their output.
#pragma once
#include "pt_grid.h"

struct AovParams {
    uint32_t width, height, samples;
    uint32_t n_local;         // pixels of this rank
    uint32_t flags;           // PT_AOV_FIRST_ENTRY | PT_AOV_CENTRE
    uint32_t log2_seg;        // k_aov: lanes per pixel = 1 << log2_seg = min(64, next power of two >= samples)
    uint32_t n_local_tiles;   // != 0: sharded - tiles[0 .. n] are the packed offsets of the rank's tiles, tiles[n + 1 + lt] their numbers
    uint32_t tile_w, tile_h, tiles_x;
};

struct AovSample {
    float v[14];      // floats 0..13 of the sample record
    int32_t prim;     // float 14
    bool covered;     // floats 7 and 15 are 1.0
};

// Local pixel (packed order of pt_local_pixel_map) -> global pixel index x + y * width.
PT_D uint32_t aov_global_pixel(const AovParams& A, const uint32_t* __restrict__ tiles, uint32_t local) {
    if (A.n_local_tiles == 0u) return local;
    uint32_t lo = 0u, hi = A.n_local_tiles;   // the last tile whose offset is <= local
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (tiles[mid] <= local) lo = mid;
        else hi = mid;
    }
    const uint32_t k = tiles[A.n_local_tiles + 1u + lo], rel = local - tiles[lo];
    const uint32_t tx = k % A.tiles_x, ty = k / A.tiles_x;
    const uint32_t cw = min(A.tile_w, A.width - tx * A.tile_w);
    return (tx * A.tile_w + rel % cw) + (ty * A.tile_h + rel / cw) * A.width;
}

// Word `idx` of the sample's generator; the block that holds it is kept in w (held: its number, 0xffffffff = none).
PT_D uint32_t aov_rng_word(uint64_t seed, uint32_t idx, uint32_t& held, uint32_t (&w)[16]) {
    if ((idx >> 4) != held) {
        held = idx >> 4;
        pt_chacha12_block(seed, held, w);
    }
    uint32_t word = w[0];
#pragma unroll
    for (int i = 1; i < 16; ++i) word = (idx & 15u) == (uint32_t)i ? w[i] : word;
    return word;
}

// The record of sample s (1-based) of global pixel i.
template <bool ALPHA, bool GRID>
PT_D void aov_sample(const DevScene& S, const AovParams& A, uint32_t i, uint32_t s, AovSample& r) {
#pragma unroll
    for (int k = 0; k < 14; ++k) r.v[k] = 0.f;
    r.prim = -1;
    r.covered = false;
    const uint64_t seed = (uint64_t)s + (uint64_t)i * (uint64_t)A.samples;
    const bool walk = ALPHA && !(A.flags & PT_AOV_FIRST_ENTRY);
    uint32_t w[16], held = 0xffffffffu;
    float r1 = 0.5f, r2 = 0.5f;
    if (!(A.flags & PT_AOV_CENTRE)) {
        r1 = (float)(aov_rng_word(seed, 0u, held, w) >> 8) * (1.0f / 16777216.0f);
        r2 = (float)(aov_rng_word(seed, 1u, held, w) >> 8) * (1.0f / 16777216.0f);
    }
    f3 o, d;
    primary_ray(S, i % A.width, i / A.width, A.width, A.height, r1, r2, o, d);
    LocalCtr lc = {0, 0, 0, 0, 0, 0};
    uint32_t cell = 0u;
    float kmax = 0.f;
    if (GRID) {
        cell = og_cell(S.cam_grid, d);
        const float dlen = mag3(d);
        kmax = (dlen > 1.0f ? dlen : 1.0f) * 1.00002f;
    }
    auto cast = [&](float t_prev, uint32_t ord_prev, RawHit& h) {
        if (GRID) return og_next_hit<false>(S, S.cam_grid, cell, o, d, kmax, INFINITY, t_prev, ord_prev, h, lc);
        return next_hit<false>(S, o, d, t_prev, ord_prev, h, lc);
    };
    RawHit best;
    bool hit = cast(-INFINITY, 0u, best);
    if (walk) {   // mod.rs:188-205: the draws follow the jitter's two
        RawHit kept = best;
        bool have_kept = false;
        uint32_t draw = 2u;
        while (hit) {
            const float opacity = hit_opacity(S, o, d, best);
            bool stop = opacity >= 1.f;
            if (!stop && opacity > 0.001f) {
                const float u = (float)(aov_rng_word(seed, draw, held, w) >> 8) * (1.0f / 16777216.0f);
                ++draw;
                stop = u < opacity;
            }
            if (stop) break;
            kept = best;
            have_kept = true;
            hit = cast(kept.key, kept.ord, best);
        }
        if (!hit && have_kept) {   // every entry skipped: the last one is shaded
            best = kept;
            hit = true;
        }
    }
    if (!hit) return;
    Surface sf;
    make_surface(S, o, d, best, sf);
    MatSample ms;
    material_sample(S, sf.model, sf.sphere, sf.uv, ms);
    const f3 n = shading_normal(S, sf);
    const float nn = dot3(n, n);
    f3 u = mk3(0.f, 0.f, 0.f);
    if (nn > 0.f && nn < INFINITY) u = n * (1.0f / sqrtf(nn));
    r.v[0] = u.x;
    r.v[1] = u.y;
    r.v[2] = u.z;
    r.v[3] = best.key;
    r.v[4] = ms.albedo.x;
    r.v[5] = ms.albedo.y;
    r.v[6] = ms.albedo.z;
    r.v[7] = 1.0f;
    r.v[8] = sf.pos.x;
    r.v[9] = sf.pos.y;
    r.v[10] = sf.pos.z;
    r.v[11] = ms.roughness;
    r.v[12] = ms.metalness;
    r.v[13] = (0.2126f * ms.emissive.x + 0.7152f * ms.emissive.y) + 0.0722f * ms.emissive.z;
    r.prim = (int32_t)PT_PRIM_INDEX(best.pid);
    r.covered = true;
}

// ------------------------------------------------------------------ pixel records
// Lane t of the launch: pixel t >> log2_seg (local), lane t & (seg - 1) of its segment.  A block of 64 consecutive sample
// numbers is summed by the pairwise tree x[j] = x[2j] + x[2j+1] - the xor butterfly below, every lane ending with the sum of
// its segment; the levels above a short segment would add +0.0f, which changes nothing but the sign of a zero: one such
// addition stands for them.  Every lane of a wavefront takes part in every cross-lane operation (no early return).
template <bool ALPHA, bool GRID>
__global__ __launch_bounds__(256) void k_aov(DevScene S, AovParams A, const uint32_t* __restrict__ tiles, float4* __restrict__ out) {
    const uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const uint32_t seg = 1u << A.log2_seg;
    const uint32_t local = (uint32_t)(t >> A.log2_seg), j = (uint32_t)t & (seg - 1u);
    const bool pixel_ok = (t >> A.log2_seg) < (uint64_t)A.n_local;
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t seg_mask = (seg == 64u ? ~0ull : ((1ull << seg) - 1ull)) << (lane & ~(seg - 1u));
    const uint32_t gi = pixel_ok ? aov_global_pixel(A, tiles, local) : 0u;
    float sum[14];
    int32_t first_prim = -1;
    uint32_t first_count = 0u;
    for (uint32_t base = 0u; base < A.samples; base += 64u) {
        const uint32_t s = base + j + 1u;   // (seg < 64: one block, base = 0)
        AovSample r;
        if (pixel_ok && s <= A.samples) {
            aov_sample<ALPHA, GRID>(S, A, gi, s, r);
        } else {
#pragma unroll
            for (int k = 0; k < 14; ++k) r.v[k] = 0.f;
            r.prim = -1;
            r.covered = false;
        }
        for (uint32_t m = 1u; m < seg; m <<= 1) {
#pragma unroll
            for (int k = 0; k < 14; ++k) r.v[k] = r.v[k] + __shfl_xor(r.v[k], (int)m);
        }
        if (seg < 64u) {
#pragma unroll
            for (int k = 0; k < 14; ++k) r.v[k] = r.v[k] + 0.f;
        }
#pragma unroll
        for (int k = 0; k < 14; ++k) sum[k] = base ? sum[k] + r.v[k] : r.v[k];
        // the primitive of the lowest-numbered covered sample, and how many covered samples have it
        const uint64_t cov = __ballot(r.covered) & seg_mask;
        const int32_t block_first = __shfl(r.prim, cov != 0ull ? (int)__builtin_ctzll(cov) : (int)lane);
        if (first_prim < 0 && cov != 0ull) first_prim = block_first;
        const uint64_t same = __ballot(r.covered && r.prim == first_prim) & seg_mask;
        first_count += (uint32_t)__popcll(same);
    }
    if (pixel_ok && j == 0u) {
        float4* p = out + (size_t)local * 4;
        p[0] = make_float4(sum[0], sum[1], sum[2], sum[3]);
        p[1] = make_float4(sum[4], sum[5], sum[6], sum[7]);
        p[2] = make_float4(sum[8], sum[9], sum[10], sum[11]);
        p[3] = make_float4(sum[12], sum[13], __int_as_float(first_prim), (float)first_count);
    }
}

// ------------------------------------------------------------------ sample records (test hook)
// records[((s - 1) * n_local + local) * 16 ..]: one lane per (sample, local pixel)
template <bool ALPHA, bool GRID>
__global__ __launch_bounds__(256) void k_aov_samples(DevScene S, AovParams A, const uint32_t* __restrict__ tiles,
                                                     float4* __restrict__ records) {
    const uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (t >= (uint64_t)A.samples * A.n_local) return;
    const uint32_t local = (uint32_t)(t % A.n_local), s = (uint32_t)(t / A.n_local) + 1u;
    AovSample r;
    aov_sample<ALPHA, GRID>(S, A, aov_global_pixel(A, tiles, local), s, r);
    const float one = r.covered ? 1.0f : 0.f;
    float4* p = records + (size_t)t * 4;
    p[0] = make_float4(r.v[0], r.v[1], r.v[2], r.v[3]);
    p[1] = make_float4(r.v[4], r.v[5], r.v[6], r.v[7]);
    p[2] = make_float4(r.v[8], r.v[9], r.v[10], r.v[11]);
    p[3] = make_float4(r.v[12], r.v[13], __int_as_float(r.prim), one);
}

// ------------------------------------------------------------------ guides from pixel records
__global__ __launch_bounds__(256) void k_aov_guides(const float4* __restrict__ aov, uint64_t n, uint32_t samples,
                                                    float4* __restrict__ guides) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const float4 r0 = aov[4 * i], r1 = aov[4 * i + 1], r3 = aov[4 * i + 3];
    const float cov = r1.w, fn = (float)samples;
    float4 a = make_float4(0.f, 0.f, 0.f, -1.0f), b = make_float4(0.f, 0.f, 0.f, __int_as_float(-1));
    if (cov > 0.f && cov + cov >= fn) {
        a = make_float4(r0.x, r0.y, r0.z, r0.w / cov);
        b = make_float4(r1.x / fn, r1.y / fn, r1.z / fn, r3.z);
    }
    guides[2 * i] = a;
    guides[2 * i + 1] = b;
}
