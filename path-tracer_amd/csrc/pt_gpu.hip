// libptgpu.so — HIP kernels and the C ABI of include/ptgpu.h (gfx950 only).
//
// Integrators
//   wavefront (default)  pt_wavefront.h: k_wf_rng, then per bounce k_wf_trace (persistent),
//                        k_wf_shade, k_wf_shadow (persistent, on a side stream beside the next trace);
//                        k_accumulate adds the staged per-sample radiance in the reference's sample order.
//                        pt_grid.h: camera rays and the shadow rays of point lights are cast through origin
//                        grids (k_og_primary, k_og_shadow) instead of the KD-tree (PT_FLAG_NO_GRIDS: KD only)
//   megakernel           k_render<COUNT> (PT_FLAG_MEGAKERNEL): one lane per pixel, samples looped inside the
//                        lane (renderer/mod.rs:105-130), KD-tree only; the second, independent implementation
//                        the parity tests cross-check the wavefront integrator with
// Other kernels
//   k_postprocess     Renderer::post_processing (mod.rs:335-353)
//   k_assemble        scatter all-gathered packed tiles into a row-major image
//   k_debug           --debug-textures G-buffer pass (debug_renderer.rs:64-105)
//   k_guides, k_dn_*  pt_denoise.h: first-hit guide planes and the a-trous filter of denoised previews
//   k_accumulate_moments, k_dnv_*  pt_variance.h: per-pixel sample moments and the variance-guided form of that filter
//   k_film_*          pt_film.h: the progressive film - merging passes, the noise figure of its moments
//   k_film_*_packed, k_film_import_shard   pt_film_shard.h: the tile kernels of shard films, and their way back to one device
//   k_aov, k_aov_samples, k_aov_guides   pt_aov.h: sample-coherent feature planes (the samples' camera casts and alpha walks) and guides from them
//   k_hist_advance                       pt_history.h: a camera path's sums carried from view to view through the AOV positions
//   k_stream_copy     achievable-HBM yardstick of the roofline (pt_measure_copy_bandwidth)
//   k_trace / k_trace_all / k_escape_query / k_isect / k_rng / k_math   parity-test hooks
#include <hip/hip_runtime.h>

#include <dlfcn.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <future>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <tuple>
#include <type_traits>
#include <unordered_map>
#include <vector>

#include "pt_integrator.h"
#include "pt_wavefront.h"
#include "pt_grid_kernels.h"
#include "pt_escape_build.h"
#include "pt_grid_build.h"
#include "pt_denoise.h"
#include "pt_variance.h"
#include "pt_lightmix.h"
#include "pt_film.h"
#include "pt_film_denoise.h"
#include "pt_film_window.h"
#include "pt_film_shard.h"
#include "pt_aov.h"
#include "pt_history.h"
#include "pthost.h"
#include "../host/scene_check.h"

// ------------------------------------------------------------------ errors
namespace {
thread_local std::string g_err;

struct GpuError {
    int code;
    std::string msg;
};

[[noreturn]] void fail(int code, const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    throw GpuError{code, buf};
}

#define HIP_CHECK(expr)                                                                            \
    do {                                                                                           \
        hipError_t _e = (expr);                                                                    \
        if (_e != hipSuccess) fail(PT_ERR_DEVICE, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
    } while (0)

template <class F>
int guarded(F&& fn) {
    try {
        fn();
        return PT_OK;
    } catch (const GpuError& e) {
        g_err = e.msg;
        return e.code;
    } catch (const std::bad_alloc&) {
        g_err = "out of host memory";
        return PT_ERR_INVALID;
    } catch (const std::exception& e) {
        g_err = e.what();
        return PT_ERR_INVALID;
    }
}
}  // namespace

// ------------------------------------------------------------------ pixel mapping
// Thread -> pixel.  Grid: one 256-thread workgroup per quarter of a tile_w x
// tile_h tile (4 wavefronts, each an 8x8 pixel block).  Local tile lt is global
// tile k = tile_table[tile_k_base + lt] (the rank's tiles in ascending order; unsharded: k = lt).
struct PixelRef {
    uint32_t x, y;
    uint32_t global_index;  // x + y*W  (seed formula, mod.rs:107-112)
    uint32_t out_index;     // position in the packed output
    bool valid;
};

__device__ __forceinline__ PixelRef map_pixel(const RenderParams& P, const uint32_t* __restrict__ tile_offsets) {
    PixelRef r;
    const uint32_t per_tile = P.tile_w * P.tile_h;
    const uint32_t blocks_per_tile = per_tile / 256u;
    uint32_t lt = blockIdx.x / blocks_per_tile;
    uint32_t q = (blockIdx.x % blocks_per_tile) * 256u + threadIdx.x;
    uint32_t wave = q >> 6, lane = q & 63u;
    uint32_t waves_x = P.tile_w >> 3;
    uint32_t tx = (wave % waves_x) * 8u + (lane & 7u);
    uint32_t ty = (wave / waves_x) * 8u + (lane >> 3);
    uint32_t k = P.tile_k_base ? tile_offsets[P.tile_k_base + lt] : lt;
    uint32_t tile_x = k % P.tiles_x, tile_y = k / P.tiles_x;
    r.x = tile_x * P.tile_w + tx;
    r.y = tile_y * P.tile_h + ty;
    r.valid = tile_y < P.tiles_y && r.x < P.width && r.y < P.height;
    r.global_index = r.x + r.y * P.width;
    if (P.shard_count <= 1) {
        r.out_index = r.global_index;
    } else {
        uint32_t cw = min(P.tile_w, P.width - tile_x * P.tile_w);
        r.out_index = tile_offsets[lt] + ty * cw + tx;
    }
    return r;
}

template <bool COUNT>
__global__ __launch_bounds__(256) void k_render(DevScene S, RenderParams P, const uint32_t* __restrict__ tile_offsets,
                                                float* __restrict__ accum, DevCounters* __restrict__ ctr) {
    __shared__ uint32_t slab[16 * PT_RNG_BLOCK];
    PixelRef px = map_pixel(P, tile_offsets);
    if (!px.valid) return;
    const uint32_t tid = threadIdx.x;
    float* out = accum + (size_t)px.out_index * 3;
    f3 acc = mk3(0.f, 0.f, 0.f);
    if (P.sample_begin != 0) acc = mk3(out[0], out[1], out[2]);
    LocalCtr lc = {0, 0, 0, 0, 0, 0};
    uint32_t draws = 0;
    for (uint32_t s = P.sample_begin + 1; s <= P.sample_end; ++s) {
        PtRng rng;
        pt_rng_seed(rng, (uint64_t)s + (uint64_t)px.global_index * (uint64_t)P.samples);
        float r1 = pt_rng_f32(rng, slab, tid);
        float r2 = pt_rng_f32(rng, slab, tid);
        f3 o, d;
        primary_ray(S, px.x, px.y, P.width, P.height, r1, r2, o, d);
        f3 color = render_path<COUNT>(S, P.bounces, o, d, rng, slab, tid, lc);
        acc = acc + color;
        if (COUNT) draws += rng.draws;
    }
    out[0] = acc.x;
    out[1] = acc.y;
    out[2] = acc.z;
    if (COUNT) {
        atomicAdd(&ctr->samples, (unsigned long long)(P.sample_end - P.sample_begin));
        atomicAdd(&ctr->segments, (unsigned long long)lc.segments);
        atomicAdd(&ctr->shadow_rays, (unsigned long long)lc.shadow_rays);
        atomicAdd(&ctr->nodes_visited, (unsigned long long)lc.nodes);
        atomicAdd(&ctr->tris_tested, (unsigned long long)lc.tris);
        atomicAdd(&ctr->shaded_hits, (unsigned long long)lc.shaded);
        atomicAdd(&ctr->rng_draws, (unsigned long long)draws);
        atomicAdd(&ctr->restarts, (unsigned long long)lc.restarts);
    }
}

// accum[p] (+)= staging[0][p] + staging[1][p] + ... in sample order: the reference's
// `*pixel += color` once per sample pass (mod.rs:105,130).
__global__ __launch_bounds__(256) void k_accumulate(const float* __restrict__ staging, float* __restrict__ accum,
                                                    uint32_t n_local, uint32_t batch, int first,
                                                    const uint8_t* __restrict__ pixel_empty, float bg_r, float bg_g, float bg_b) {
    uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= n_local) return;
    f3 acc = mk3(0.f, 0.f, 0.f);
    if (!first) acc = mk3(accum[3 * (size_t)p], accum[3 * (size_t)p + 1], accum[3 * (size_t)p + 2]);
    if (pixel_empty != nullptr && pixel_empty[p]) {
        // camera-grid cull (k_cam_block_mask): every sample of this pixel is the background - the value the bounce-0
        // kernel would have staged (mod.rs:184-186 with the initial throughput and colour), added once per sample
        const f3 c = mk3(0.f, 0.f, 0.f) + mul_ew(mk3(1.f, 1.f, 1.f), mk3(bg_r, bg_g, bg_b));
        for (uint32_t s = 0; s < batch; ++s) acc = acc + c;
    } else {
        for (uint32_t s = 0; s < batch; ++s) {
            const float* v = staging + ((size_t)s * n_local + p) * 3;
            acc = acc + mk3(v[0], v[1], v[2]);
        }
    }
    accum[3 * (size_t)p] = acc.x;
    accum[3 * (size_t)p + 1] = acc.y;
    accum[3 * (size_t)p + 2] = acc.z;
}

__global__ __launch_bounds__(256) void k_postprocess(const float* __restrict__ accum, uint8_t* __restrict__ rgb8,
                                                     uint32_t n, uint32_t samples, int tonemap_type) {
    uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    f3 c = mk3(accum[3 * (size_t)i], accum[3 * (size_t)i + 1], accum[3 * (size_t)i + 2]) / (float)samples;
    c = tonemap(tonemap_type, c);
    rgb8[3 * (size_t)i] = as_u8(pt_pow_inv_gamma(c.x) * 255.f);
    rgb8[3 * (size_t)i + 1] = as_u8(pt_pow_inv_gamma(c.y) * 255.f);
    rgb8[3 * (size_t)i + 2] = as_u8(pt_pow_inv_gamma(c.z) * 255.f);
}

// gathered: shard_count slices of slice_pixels packed pixels; tile_src[k] = rank (high 8 bits) and packed offset of
// global tile k inside its rank's slice... as two words: tile_src[2k] = rank, tile_src[2k + 1] = offset
__global__ __launch_bounds__(256) void k_assemble(const uint8_t* __restrict__ gathered, uint8_t* __restrict__ image,
                                                  const uint32_t* __restrict__ tile_src,
                                                  uint32_t width, uint32_t height,
                                                  uint32_t tile_w, uint32_t tile_h, uint32_t tiles_x,
                                                  uint64_t slice_pixels, uint32_t elem_bytes) {
    uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= width * height) return;
    uint32_t x = i % width, y = i / width;
    uint32_t tile_x = x / tile_w, tile_y = y / tile_h;
    uint32_t k = tile_y * tiles_x + tile_x;
    uint32_t cw = min(tile_w, width - tile_x * tile_w);
    uint64_t src = (uint64_t)tile_src[2 * (size_t)k] * slice_pixels + tile_src[2 * (size_t)k + 1] +
                   (uint64_t)(y - tile_y * tile_h) * cw + (x - tile_x * tile_w);
    const uint8_t* s = gathered + src * elem_bytes;
    uint8_t* d = image + (uint64_t)i * elem_bytes;
    for (uint32_t b = 0; b < elem_bytes; ++b) d[b] = s[b];
}

// The counts of one chunk, gathered into one line of the frame's statistics (frame_plan, render_chunk).
// cold / lean_out (the lean bounce-0 variant's eligibility, frame_plan): the block of the bounce-1 hits' device counters and this
// line's word behind the frame's lines - the workgroups of the loading bounce-0 launches that cast for a light ([8]) and their
// lanes that found no continuation record ([6]) or ran the escape test themselves ([7]) since the last line was taken; [9]
// keeps the sum that line saw.  No block: all ones, "not known".  shadow_out: this line's two words behind the cold words.
__global__ void k_wf_stats(const WfCounters* __restrict__ ctr, uint32_t levels, uint32_t* __restrict__ out,
                           unsigned long long* __restrict__ cold, uint32_t* __restrict__ lean_out, uint32_t* __restrict__ shadow_out) {
    const uint32_t b = threadIdx.x;
    // (the lean shade pass of bounces 1 and 2: the shadow records written there, apart from those the fused pass inlined)
    if ((b == 1 || b == 2) && b < levels) shadow_out[b - 1u] = ctr[b].shadow_count;
    else if ((b == 1 || b == 2)) shadow_out[b - 1u] = 0u;
    if (b == 0) {
        uint32_t since = 0xffffffffu;
        if (cold) {
            const unsigned long long sum = cold[6] + cold[7] + cold[8];
            since = (uint32_t)min(sum - cold[9], 0xfffffffeull);
            cold[9] = sum;
        }
        *lean_out = since;
    }
    if (b >= levels) return;
    // (+ the records the bounce-0 kernel elided for the bounce-1 hit cache: the plan sizes queues, counts rays for the inline
    // rule and finds a chunk's last bounce as a frame that casts would - a plan outlives the frames that elide)
    // (+ what the bounce-1 shade pass that adds the known lights itself left unwritten: shadow records, and the list entries
    // of the survivors that ended there - the same rule, k_wf_shade_fused)
    out[4 * b + 0] = ctr[b].queue_count + ctr[b].elided_count;
    out[4 * b + 1] = ctr[b].shadow_count + ctr[b].inlined_count;
    out[4 * b + 2] = ctr[b].exact_count + ctr[b].exact_elided;
    out[4 * b + 3] = b == 0 ? ctr[0].overflow : ctr[b].offgrid_count;
}

// ------------------------------------------------------------------ test-hook kernels
__device__ __forceinline__ void store_hit(pt_hit& o, const RawHit& h) {
    o.prim = (int32_t)PT_PRIM_INDEX(h.pid);
    o.flags = (int32_t)h.flags;
    o.dist = h.key;
    o.u = (h.flags & 2u) ? 0.f : h.u;
    o.v = (h.flags & 2u) ? 0.f : h.v;
}

__global__ __launch_bounds__(256) void k_trace(DevScene S, const float* __restrict__ rays, uint64_t n,
                                               pt_hit* __restrict__ out) {
    uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    f3 o = mk3(rays[6 * i], rays[6 * i + 1], rays[6 * i + 2]);
    f3 d = mk3(rays[6 * i + 3], rays[6 * i + 4], rays[6 * i + 5]);
    LocalCtr lc = {0, 0, 0, 0, 0, 0};
    RawHit h;
    if (next_hit<false>(S, o, d, -INFINITY, 0u, h, lc)) store_hit(out[i], h);
    else out[i] = pt_hit{-1, 0, 0.f, 0.f, 0.f};
}

__global__ __launch_bounds__(256) void k_trace_all(DevScene S, const float* __restrict__ rays, uint64_t n,
                                                   uint32_t max_hits, pt_hit* __restrict__ out,
                                                   uint32_t* __restrict__ counts) {
    uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    f3 o = mk3(rays[6 * i], rays[6 * i + 1], rays[6 * i + 2]);
    f3 d = mk3(rays[6 * i + 3], rays[6 * i + 4], rays[6 * i + 5]);
    LocalCtr lc = {0, 0, 0, 0, 0, 0};
    RawHit h;
    float t_prev = -INFINITY;
    uint32_t ord_prev = 0, cnt = 0;
    while (cnt < 4096u && next_hit<false>(S, o, d, t_prev, ord_prev, h, lc)) {
        if (cnt < max_hits) store_hit(out[i * max_hits + cnt], h);
        ++cnt;
        t_prev = h.key;
        ord_prev = h.ord;
    }
    counts[i] = cnt;
    for (uint32_t j = cnt; j < max_hits; ++j) out[i * max_hits + j] = pt_hit{-1, 0, 0.f, 0.f, 0.f};
}

// The lookup k_wf_shade makes when it has sampled a bounce direction, one query per lane: the function itself, so that a test
// asks the device which cell it reads for a direction on a border instead of restating it.  prims are checked on the host.
__global__ __launch_bounds__(256) void k_escape_query(DevScene S, const uint32_t* __restrict__ prims, const float* __restrict__ rays,
                                                      uint64_t n, uint8_t* __restrict__ proven) {
    uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    f3 o = mk3(rays[6 * i], rays[6 * i + 1], rays[6 * i + 2]);
    f3 d = mk3(rays[6 * i + 3], rays[6 * i + 4], rays[6 * i + 5]);
    proven[i] = escape_proves_miss(S, prims[i], o, d) ? 1 : 0;
}

// render_debug_pixels (src/renderer/debug_renderer.rs:64-105): first hit of the pixel-centre ray
__global__ __launch_bounds__(256) void k_debug(DevScene S, uint32_t width, uint32_t height, uint8_t* __restrict__ planes,
                                               int* __restrict__ any_hit) {
    uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= width * height) return;
    uint32_t x = i % width, y = i / width;
    f3 o, d;
    primary_ray(S, x, y, width, height, 0.5f, 0.5f, o, d);  // screen = x + 0.5 (debug_renderer.rs:24-30)
    LocalCtr lc = {0, 0, 0, 0, 0, 0};
    RawHit h;
    if (!next_hit<false>(S, o, d, -INFINITY, 0u, h, lc)) return;
    Surface sf;
    make_surface(S, o, d, h, sf);
    MatSample ms;
    material_sample(S, sf.model, sf.sphere, sf.uv, ms);
    f3 n = shading_normal(S, sf);
    float ior = S.materials[sf.model].ior;
    const f3 one = mk3(1.f, 1.f, 1.f);
    f3 v[PT_DEBUG_PLANES] = {mk3(n.x * 0.5f + 0.5f, n.y * 0.5f + 0.5f, n.z * 0.5f + 0.5f), ms.albedo, one * ms.opacity,
                             one * ms.metalness, one * ms.roughness, ms.emissive, (one * ior) / 3.f};
    size_t npix = (size_t)width * height;
#pragma unroll
    for (int p = 0; p < PT_DEBUG_PLANES; ++p) {
        uint8_t* out = planes + ((size_t)p * npix + i) * 3;
        out[0] = as_u8(v[p].x * 255.f);
        out[1] = as_u8(v[p].y * 255.f);
        out[2] = as_u8(v[p].z * 255.f);
    }
    *any_hit = 1;
}

__global__ __launch_bounds__(256) void k_isect(const float* __restrict__ rays, const float* __restrict__ tris,
                                               uint64_t n, pt_hit* __restrict__ out) {
    uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    f3 o = mk3(rays[6 * i], rays[6 * i + 1], rays[6 * i + 2]);
    f3 d = mk3(rays[6 * i + 3], rays[6 * i + 4], rays[6 * i + 5]);
    f3 v0 = ld3(tris + 9 * i), v1 = ld3(tris + 9 * i + 3), v2 = ld3(tris + 9 * i + 6);
    float dist, u, v;
    bool bf;
    if (isect_triangle(o, d, v0, v1 - v0, v2 - v0, dist, u, v, bf)) {
        // tex_coords of the unit-test triangle (uv0=(0,0), uv1=(1,0), uv2=(0,1); triangle.rs:165-184)
        f2 uv0 = {0.f, 0.f}, uv1 = {1.f, 0.f}, uv2 = {0.f, 1.f};
        f2 tc = uv0 + u * (uv1 - uv0) + v * (uv2 - uv0);
        out[i] = pt_hit{0, bf ? 1 : 0, dist, tc.x, tc.y};
    } else {
        out[i] = pt_hit{-1, 0, 0.f, 0.f, 0.f};
    }
}

__global__ __launch_bounds__(256) void k_rng(const uint64_t* __restrict__ seeds, uint64_t n_seeds, uint32_t n_words,
                                             uint32_t* __restrict__ out) {
    __shared__ uint32_t slab[16 * PT_RNG_BLOCK];
    uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n_seeds) return;
    PtRng rng;
    pt_rng_seed(rng, seeds[i]);
    for (uint32_t w = 0; w < n_words; ++w) out[i * n_words + w] = pt_rng_next_u32(rng, slab, threadIdx.x);
}

// plain streaming copy, 16 B per lane per step: the achievable-HBM yardstick of the roofline
typedef float pt_v4f __attribute__((ext_vector_type(4)));
__global__ __launch_bounds__(256) void k_stream_copy(const float4* __restrict__ src4, float4* __restrict__ dst4, uint64_t n) {
    const pt_v4f* src = (const pt_v4f*)src4;
    pt_v4f* dst = (pt_v4f*)dst4;
    uint64_t i = (uint64_t)blockIdx.x * 1024u + threadIdx.x;   // 4 independent 16-byte loads in flight per lane
    if (i + 768u < n) {
        pt_v4f a = __builtin_nontemporal_load(src + i), b = __builtin_nontemporal_load(src + i + 256u);
        pt_v4f c = __builtin_nontemporal_load(src + i + 512u), d = __builtin_nontemporal_load(src + i + 768u);
        __builtin_nontemporal_store(a, dst + i);
        __builtin_nontemporal_store(b, dst + i + 256u);
        __builtin_nontemporal_store(c, dst + i + 512u);
        __builtin_nontemporal_store(d, dst + i + 768u);
    } else {
        for (; i < n; i += 256u) dst[i] = src[i];
    }
}

// scattered 8- / 16-byte loads, eight independent ones in flight per lane (pt_measure_gather_rate)
template <int BYTES>
__global__ __launch_bounds__(256) void k_gather(const uint4* __restrict__ table, uint32_t mask, uint32_t rounds,
                                                uint32_t* __restrict__ sink) {
    uint32_t x = (blockIdx.x * 256u + threadIdx.x) * 2654435761u + 12345u, acc = 0;
    for (uint32_t r = 0; r < rounds; ++r) {
        uint32_t idx[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            x = x * 1664525u + 1013904223u;      // LCG: a different 16-byte slot per lane and load
            idx[k] = (x >> 8) & mask;
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            if (BYTES == 16) {
                uint4 v = table[idx[k]];
                acc += v.x ^ v.w;
            } else {
                uint2 v = *(const uint2*)(table + idx[k]);
                acc += v.x ^ v.y;
            }
        }
    }
    if (acc == 0x9e3779b9u) sink[0] = acc;   // (keeps the loads alive)
}

__global__ __launch_bounds__(256) void k_math(int fn, const float* __restrict__ x, uint64_t n, float* __restrict__ out) {
    uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    float v = x[i], r;
    switch (fn) {
        case 0: r = pt_pow_inv_gamma(v); break;
        case 1: r = pt_acosf(v); break;
        case 2: r = pt_sinf(v); break;
        case 3: r = pt_cosf(v); break;
        default: r = NAN;
    }
    out[i] = r;
}

// ------------------------------------------------------------------ host side
namespace {

struct TileMap {
    uint32_t tile_w, tile_h, tiles_x, tiles_y, count, rank;
    uint32_t n_local_tiles;
    uint64_t n_local;
    std::vector<uint32_t> offsets;  // n_local_tiles + 1 (only used when count > 1)
    std::vector<uint32_t> tiles;    // global number (ty * tiles_x + tx) of every local tile, ascending
};

void normalise_opts(const pt_profile& p, const pt_opts* in, pt_opts& o) {
    if (in) o = *in;
    else memset(&o, 0, sizeof o), o.device = -1;
    if (o.shard_count == 0) o.shard_count = 1;
    if (o.tile_w == 0) o.tile_w = 32;
    if (o.tile_h == 0) o.tile_h = 32;
    if (o.shard_rank >= o.shard_count) fail(PT_ERR_INVALID, "shard_rank %u >= shard_count %u", o.shard_rank, o.shard_count);
    if ((o.tile_w & 7u) || (o.tile_h & 7u) || ((o.tile_w * o.tile_h) & 255u))
        fail(PT_ERR_INVALID, "tile_w/tile_h must be multiples of 8 with tile_w*tile_h a multiple of 256");
    if (p.width == 0 || p.height == 0) fail(PT_ERR_INVALID, "profile resolution must be non-zero");
    if ((uint64_t)p.width * p.height >= (1ull << 31)) fail(PT_ERR_UNSUPPORTED, "image too large");
}

// Which rank renders tile (tx, ty): (tx + ty * stride) mod count - diagonal stripes, so that every rank takes tiles
// from every column and every row of the image.  (k mod count, the obvious rule, degenerates into vertical stripes
// whenever the tile columns are a multiple of count / 2: at 1920x1080 with 32x32 tiles and 8 ranks it gave each rank
// every fourth column, and the per-rank frame times of config 3 ranged from 6.7 to 8.1 ms.)  stride = the smallest
// odd number >= 3 that is coprime to count (1 for count <= 2: a checkerboard).
uint32_t tile_rank_stride(uint32_t count) {
    if (count <= 2) return 1;
    for (uint32_t s = 3;; s += 2) {
        uint32_t a = s, b = count;
        while (b) {
            uint32_t t = a % b;
            a = b;
            b = t;
        }
        if (a == 1) return s;
    }
}
inline uint32_t tile_rank(uint32_t tx, uint32_t ty, uint32_t count, uint32_t stride) {
    return (uint32_t)(((uint64_t)tx + (uint64_t)ty * stride) % count);
}

TileMap make_tile_map(const pt_profile& p, const pt_opts& o, uint32_t rank) {
    TileMap m;
    m.tile_w = o.tile_w;
    m.tile_h = o.tile_h;
    m.tiles_x = (p.width + o.tile_w - 1) / o.tile_w;
    m.tiles_y = (p.height + o.tile_h - 1) / o.tile_h;
    m.count = o.shard_count;
    m.rank = rank;
    const uint32_t stride = tile_rank_stride(m.count);
    uint64_t off = 0;
    for (uint32_t ty = 0; ty < m.tiles_y; ++ty)
        for (uint32_t tx = 0; tx < m.tiles_x; ++tx) {
            if (m.count > 1 && tile_rank(tx, ty, m.count, stride) != rank) continue;
            uint32_t cw = std::min(o.tile_w, p.width - tx * o.tile_w);
            uint32_t ch = std::min(o.tile_h, p.height - ty * o.tile_h);
            m.tiles.push_back(ty * m.tiles_x + tx);
            m.offsets.push_back((uint32_t)off);
            off += (uint64_t)cw * ch;
        }
    m.n_local_tiles = (uint32_t)m.tiles.size();
    m.offsets.push_back((uint32_t)off);
    m.n_local = off;
    return m;
}

// The tile map of a tile-list frame (pt_render_tiles): the listed tiles in list order, packed one after the other -
// what make_tile_map gives a rank, with the list in place of the rank rule.  PT_ERR_INVALID: a null or empty list, one that
// is not strictly ascending, a tile number beyond the image's tiles, a sharded frame.
TileMap make_tile_list_map(const char* who, const pt_profile& p, const pt_opts& o, const uint32_t* tiles, uint32_t n_tiles) {
    if (!tiles || !n_tiles) fail(PT_ERR_INVALID, "%s: the tile list is empty", who);
    if (o.shard_count > 1) fail(PT_ERR_INVALID, "%s: a tile list and shard_count %u exclude each other", who, o.shard_count);
    TileMap m;
    m.tile_w = o.tile_w;
    m.tile_h = o.tile_h;
    m.tiles_x = (p.width + o.tile_w - 1) / o.tile_w;
    m.tiles_y = (p.height + o.tile_h - 1) / o.tile_h;
    m.count = 1;
    m.rank = 0;
    uint64_t off = 0;
    for (uint32_t lt = 0; lt < n_tiles; ++lt) {
        const uint32_t k = tiles[lt];
        if (k >= m.tiles_x * m.tiles_y) fail(PT_ERR_INVALID, "%s: tile %u of an image of %u x %u tiles", who, k, m.tiles_x, m.tiles_y);
        if (lt && k <= tiles[lt - 1]) fail(PT_ERR_INVALID, "%s: the tile list is not strictly ascending (%u after %u)", who, k, tiles[lt - 1]);
        const uint32_t tx = k % m.tiles_x, ty = k / m.tiles_x;
        const uint32_t cw = std::min(o.tile_w, p.width - tx * o.tile_w), ch = std::min(o.tile_h, p.height - ty * o.tile_h);
        m.tiles.push_back(k);
        m.offsets.push_back((uint32_t)off);
        off += (uint64_t)cw * ch;
    }
    m.n_local_tiles = n_tiles;
    m.offsets.push_back((uint32_t)off);
    m.n_local = off;
    return m;
}

struct DeviceBuffer {
    void* p = nullptr;
    size_t bytes = 0;
    void ensure(size_t n) {
        if (!try_ensure(n)) fail(PT_ERR_DEVICE, "hipMalloc of %zu bytes failed: out of device memory", n);
    }
    bool try_ensure(size_t n) {  // false (buffer released) when the device cannot provide n bytes
        if (n <= bytes) return true;
        release();
        if (hipMalloc(&p, n) != hipSuccess) {
            (void)hipGetLastError();  // clear the sticky error
            p = nullptr;
            return false;
        }
        bytes = n;
        return true;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
    }
    ~DeviceBuffer() {
        if (p) (void)hipFree(p);
    }
};

}  // namespace

// What pt_scene_set_camera / _set_lights / _set_materials need to give a scene the grids and tables pt_scene_create would
// have made for an edited description, without the caller's pt_scene_desc or the prep: the primitives' geometry as the grid
// footprints take it (9 floats: three positions, or centre + radius) with the id | sphere-bit word, the positions of the
// triangles no model owns (og_params_point's and params_ortho's extents scan every triangle of the description), the inputs
// of the grids' resolution rule (grid_rule), and the model -> material indices with the texture table a new material table
// is checked against.  Shared by a prep and the scenes made from it (host memory: 40 B per primitive).
struct CamGridSource {
    std::vector<float> og_geom;
    std::vector<uint32_t> og_words;
    std::vector<float> unowned;   // 9 floats per triangle outside every model's range
    bool device_grids = false;    // false: PT_OG_HOST=1 (a moved camera, edited lights go without grids)
    bool grids_on = false;        // PT_OG
    uint32_t cam_res = 0;         // resolution of a camera grid; 0: none whatever the camera (PT_OG=0, no primitives, budget)
    double budget = 0;            // PT_OG_BUDGET_GIB in bytes
    std::vector<int32_t> model_material;   // pt_model.material of every model
    uint32_t n_materials = 0;
    std::vector<pt_texture> textures;
    uint64_t n_texel_bytes = 0;
};

// One origin grid of a scene: what the kernels read of it, its header (enabled = 0: no grid) and the bytes of its two arrays.
struct GridSlot {
    DevGrid dev{};
    pth_origin_grid hdr{};
    uint64_t bytes = 0;
};

// The origin grids of a scene, said once.  grids_on_device makes one (PT_OG_HOST=1: upload_host_grids, from the prep's), an
// edit makes the part it replaces, and install_camera_grid / install_light_grids hand it to the scene - with what DevScene
// restates of it.  What pt_scene_get_info reports of the grids is read from here when it is asked for (grid_facts).
struct SceneGrids {
    GridSlot cam;
    std::vector<GridSlot> lights;   // one per light of the scene
    bool all_lights = false;        // every light has a grid: the shadow rays take them (no lights at all: vacuously)
    bool ortho = false;             // some light grid is orthographic (a directional light): kernel variants DIRL
    bool headers = false;           // built on the device: pt_scene_grid_header / _copy show them (host-built grids: all zero)
    float seconds = 0.f;            // what building them on the device took
    void lights_done(bool all) {    // the light slots stand, all of them, or none does (emptied)
        if (!all) lights.assign(lights.size(), GridSlot{});
        all_lights = all;
        ortho = std::any_of(lights.begin(), lights.end(), [](const GridSlot& g) { return g.dev.kind != 0; });
    }
    const GridSlot* slot(uint32_t which) const {   // 0: the camera's, 1 + i: light i's; nullptr: no such light
        return which == 0 ? &cam : which - 1 < lights.size() ? &lights[which - 1] : nullptr;
    }
};

struct pt_scene {
    int device = 0;
    DevScene dev{};
    std::vector<void*> allocations;
    pt_scene_info info{};   // (device_bytes: every allocation but the grids' arrays; the grids' rows: grid_facts)
    SceneGrids grids;
    std::vector<uint32_t> host_prim_entry;
    std::shared_ptr<const CamGridSource> cam_src;   // (pt_scene_set_camera, _set_lights, _set_materials)
    uint32_t cam_res = 0;                             // the camera grid's resolution rule for the scene's light count (grid_rule)
    pt_timing timing{};
    pt_counters counters{};
    DeviceBuffer accum_scratch, counter_buf, staging_buf;
    // The queues of the chunk of work items in flight.  The shadow casts of bounce b run on a side stream
    // beside the trace of bounce b+1, so the tail of one persistent launch is filled by the other's head.
    struct WfPipe {
        DeviceBuffer queue[2], hits, shadow, contrib, ctr, rng[2], draws, offgrid, deferred, exact[2], block_mask;
        // the hits of queue 2 where the bounce-1 shade pass answers its survivors' casts from the bounce-2 hit cache itself: that
        // launch is still reading `hits`.  As long as queue 2 (20 B per record); like the cache it serves, not part of queue_bytes
        DeviceBuffer hits_next;
        // the hand-over list of the lean shade pass of bounces 1 and 2 (k_wf_shade_fused<SB_VIS1 | SB_LEAN1>, code 8448): WF_HANDOVER_HEAD count
        // words by bounce, zeroed once per chunk, then queue indices - as long as the longer queue.  Not part of queue_bytes either
        DeviceBuffer handover;
        hipStream_t side = nullptr, side_wide = nullptr, side_exact = nullptr;
        hipEvent_t ev_shade = nullptr, ev_shadow = nullptr, ev_rng = nullptr, ev_chunk = nullptr, ev_trace = nullptr, ev_wide = nullptr,
                   ev_exact = nullptr, ev_exact_go = nullptr;
    };
    WfPipe pipe;
    // What a frame of one configuration produced: records per queue and bounce, per chunk of work items.  A frame is a pure
    // function of (scene, profile, options) - the seeds are the pixels' - so the counts of one frame are those of every later
    // one: the FIRST frame of a configuration runs in chunks small enough for a fixed budget with every queue as long as the
    // chunk, the later ones get queues as long as the records that exist (frame_plan).
    struct FrameStats {
        uint32_t cap_items = 0, n_slots = 0, levels = 0;   // the chunking the numbers were taken with; (batch, chunk) slots; bounces + 2
        uint32_t* host = nullptr;                         // pinned: n_slots x levels x 4 words (queue, shadow, exact, offgrid | overflow)
        hipEvent_t done = nullptr;
        bool pending = false, valid = false, planned = false;
        bool stats_planned = false;   // the counts on their way were taken by a frame that ran the plan
        // the counts (on their way / the plan's) are of a frame that loaded the hits of these bounces (bit b; hit1_cache,
        // hit2_cache): the shade pass before listed no ray for k_wf_trace_exact, so the exact count of that bounce is lower than
        // a frame that casts would have
        uint32_t stats_hit_loads = 0, plan_hit_loads = 0;
        std::vector<uint32_t> first_item_of_slot;         // (which chunk a slot was)
        // the plan made from them: work items per chunk, records per queue / hit / shadow / exact array, the bounces whose
        // shadow casts go inline; fresh until its buffers have been allocated once (buffers much larger are given back then)
        uint32_t plan_cap = 0, plan_q[2] = {0, 0}, plan_h = 0, plan_s = 0, plan_e = 0;
        std::vector<uint8_t> plan_inline;
        std::vector<uint32_t> plan_last;   // per chunk of the plan: the last bounce that has a ray (later ones are not launched)
        bool plan_fresh = false, plan_failed = false;   // (failed: the device could not provide the plan's buffers)
        // The lean bounce-0 variant (k_wf_shade_hits<.. | SB_CONT_LOAD | SB_LEAN>, code 6379).  lean: the last counted frame of the configuration was a
        // planned one whose bounce-0 launches all loaded every cache with the escape answers in the records, and none of their
        // lanes cast for a light, lacked a record, ran the escape test or wrote a shadow record; lean_sig: the state of the
        // caches and masks it was counted under (lean_signature) - a frame under another state takes the general variant.
        // stats_lean_ok, stats_sig: the same of the counts on their way.
        bool lean = false, stats_lean_ok = false;
        std::vector<uint64_t> lean_sig, stats_sig;
        const uint32_t* cold_words() const { return host + (size_t)n_slots * levels * 4u; }   // one word per line, behind the lines
        // The lean shade pass of bounces 1 and 2 (k_wf_shade_fused<SB_VIS1 | SB_LEAN1>, code 8448), by bounce - 1.  b1_lean: the last counted frame
        // of the configuration was a planned one that wrote at that bounce fewer shadow records than 1 / PT_B1_LEAN_SHARE of
        // the records it shaded (shadow records + those whose lights the fused pass added itself); b1_sig: the state it was
        // counted under (lean_sig's, plus that bounce's visibility and hit planes); stats_b1_sig: the same of the counts on
        // their way.  shadow_words: two words per line behind the cold words - the shadow records written at bounces 1 and 2.
        bool b1_lean[2] = {false, false}, stats_b1_ok = false;   // (stats_b1_ok: the counts on their way are a plain frame's)
        std::vector<uint64_t> b1_sig[2], stats_b1_sig[2];
        const uint32_t* shadow_words() const { return cold_words() + n_slots; }
        static size_t host_bytes(uint32_t slots, uint32_t lv) { return (size_t)slots * lv * 16u + (size_t)slots * 12u; }
        ~FrameStats() {
            if (host) (void)hipHostFree(host);
            if (done) (void)hipEventDestroy(done);
        }
    };
    // What earlier frames left that an edit of the scene invalidates (drop_frame_state): the counts of every configuration
    // (a plan sized from another camera's, light's or material's counts may overflow) and the size of the last frame's
    // camera-grid cull table
    struct FrameState {
        std::map<std::vector<uint64_t>, std::unique_ptr<FrameStats>> stats;
        uint32_t mask_blocks = 0;   // blocks of the last frame's camera-grid cull table (0: no cull in that frame)
    } frame_state;
    // A tile-list frame (pt_render_tiles) keeps out of all that: its counts go to a slot of its own, reset by every such frame
    // (which waits for the device first: no copy into `host` and no `done` is in flight then), and its tile table - offsets, tile
    // numbers, visiting order - to a buffer of its own, rewritten by every such frame (tile_tables is cached by a key that does
    // not know the list)
    std::unique_ptr<FrameStats> tile_frame_stats;
    DeviceBuffer tile_list_table;
    DeviceBuffer stats_dev;
    // A frame cache: one value per work item that later frames of the same key read instead of computing it again.  The
    // mechanics they all share (frame_cache_frame, render_chunk): the plane is indexed by frame-global item g = batch x
    // items per batch + item and - words and hits - filled as a prefix [0, mark) in frame order, whatever the chunking; it is
    // keyed to a key in the SECOND consecutive frame of that key, so a one-shot render never pays for it and a caller
    // alternating two keys never thrashes it; it is not an edit's to drop (drop_frame_state: an edit that matters changes the
    // key) and not part of queue_bytes / device_bytes.  One event, behind the last launch that wrote the plane (the
    // visibility plane: that may have written), is what a frame on another stream waits for: the caller orders the frames
    // of a scene - they share its queues - so the earlier writes are behind it.
    struct FrameCache {
        DeviceBuffer buf;
        std::vector<uint64_t> key, last_key;   // what the contents are of; the key of the scene's last wavefront frame
        uint64_t items = 0;                    // work items of the keyed frame
        uint64_t stride = 0;                   // of them, those the budget has room for
        uint64_t mark = 0;                     // items of the prefix written so far
        uint64_t counter[3] = {0, 0, 0};       // since the scene was made (pt_get_*_cache_stats name them)
        hipEvent_t ev = nullptr;
        hipStream_t stream = nullptr;          // the one `ev` was last recorded on
        bool recorded = false, failed = false;   // (failed: the device could not provide the plane: no such cache for this scene)
        ~FrameCache() {
            if (ev) (void)hipEventDestroy(ev);
        }
        // a launch on `st` touched the plane
        void touched(hipStream_t st) {
            HIP_CHECK(hipEventRecord(ev, st));
            recorded = true;
            stream = st;
        }
        // `st` goes on behind the last launch that touched the plane
        void wait_on(hipStream_t st) const {
            if (recorded && stream != st) HIP_CHECK(hipStreamWaitEvent(st, ev, 0));
        }
    };
    // Words 0-7 of ChaCha block 0 of every work item of ONE item enumeration: a sample's seed is sample + pixel x samples -
    // the enumeration alone, not the scene, the camera, the lights, the materials or the bounces - so the frames of a
    // camera path, of live edits or of a steady state read them instead of deriving them again.  Two planes of `stride`
    // uint4 (words 0-3, words 4-7).  counter[0]: fill launches.
    FrameCache rng_cache;
    // The camera rays' closest hits of ONE view: the hit of a camera ray depends on the item enumeration (the jitter
    // words), the camera and the geometry - not on the lights, the bounces or, in an opaque scene, the materials - so the
    // frames of light and material edits and of a steady state read it instead of casting again.  One plane of uint4
    // (pack_hit), written by the storing variant of the bounce-0 kernel.  A camera move resets the mark (the allocation
    // stays).  counter[0], [1]: launches of the storing / loading variants.
    FrameCache hit_cache;
    // The answers of the bounce-0 shadow casts of ONE view and ONE set of light positions: in an opaque scene og_blocked
    // for an item and a light depends on the item's camera hit, the light's kind and position and the geometry - not on the
    // materials, the light's colour or the bounces - so the frames of material and colour edits and of a steady state read
    // it instead of casting again.  One byte per item: two bits per light (scenes of at most four), 0 unknown / 1 not
    // blocked / 2 blocked.  No high-water mark: zero is "unknown", and the kernel that reads the plane casts for what it
    // finds unknown and writes the answer back (k_wf_shade_hits<.. | SB_VIS>); a moved light or camera makes a new key (one
    // memset, the allocation stays).  counter[0], [1]: times the plane was zeroed / launches of the variant.
    FrameCache vis_cache;
    // The closest hits of the bounce-1 rays of ONE view and ONE material table: in an opaque scene that ray is made from the
    // item's camera hit, the material record there and words 2-3 of its ChaCha block - not from a light's position, kind,
    // colour or count, nor from the bounces - so the frames of light edits and of a steady state read its hit instead of
    // casting again.  One plane of uint4 (pack_hit, bit 28 of the word flipped: zero is "never written"), zeroed when it is
    // keyed AND filled as a prefix: which items reach bounce 1 may differ between frames of one key (escape masks, surfaces
    // lit through the shadow queue), so a chunk below the mark may still meet an item without a record, and casts for it
    // (k_wf_hits_store / k_wf_hits_load in pt_wavefront.h).  A camera move resets the mark.  counter[0], [1], [2]: times
    // the plane was zeroed / storing launches / loading launches; hit1_unknown: the casts the loading launches left to
    // k_wf_trace_exact (one uint64 on the device).
    // (hit1_unknown: four uint64 - behind the counter of unknown casts, what the bounce-0 launches that read the plane
    // themselves counted: records written, records elided, unknown; hit1_fused_launches: those launches.
    // pt_get_hit1_fused_stats)
    FrameCache hit1_cache;
    DeviceBuffer hit1_unknown;
    uint64_t hit1_fused_launches = 0;
    // The bounce-0 continuations of ONE view and ONE material table - the direction the BRDF samples at the camera hit and the
    // throughput behind it: made from what the bounce-1 hits' key holds, so that key, its eligibility and its re-keying are
    // theirs.  Two planes of `stride` uint4 (pt_wf_shade_body.h CONT_STORE / CONT_LOAD), zeroed when they are keyed and filled
    // as a prefix with a mark of its own: by the bounce-0 launches of the chunks whose bounce-1 hits are stored in that frame
    // (k_wf_shade_hits<.. | SB_CONT_STORE>), read by the launches that read the bounce-1 hits themselves (<.. | SB_CONT_LOAD>).  A camera move
    // resets the mark.  counter[0], [1], [2]: times the planes were zeroed / storing launches / loading launches; the hit
    // lanes a loading launch found without a record (none, ever) are word 6 of hit1_unknown.  pt_get_cont_cache_stats
    // (the escape test's answer in the records, PT_CONT_ESCAPE: escape_generation is bumped wherever the masks are built, dropped
    // or rebuilt; cont_escape_generation is the one the records were stored under - 0: none, or stored under more than one)
    FrameCache cont_cache;
    uint64_t escape_generation = 1, cont_escape_generation = 0;
    // (records stored before the masks existed get their answers from k_cont_escape_fill, chunk by chunk in the first frame
    // that finds masks the prefix was not stored under - render_chunk: [0, cont_fill_mark) has those of cont_fill_generation,
    // and once that covers the prefix cont_escape_generation is the masks'.  cont_fill_launches / _items: those launches and
    // the items they went over; cont_flagged_launches: loading launches told that the records have answers; the lanes of
    // such launches that ran the test all the same are word 7 of hit1_unknown.  pt_get_cont_escape_stats)
    uint64_t cont_fill_generation = 0, cont_fill_mark = 0;
    uint64_t cont_fill_launches = 0, cont_fill_items = 0, cont_flagged_launches = 0;
    // (the loading bounce-0 launches by variant - lean, k_wf_shade_hits<.. | SB_LEAN> (6379), and general - and the frames a lean launch
    // flagged because it met a lane it does not contain the code for: none, ever.  pt_get_b0_lean_stats)
    uint64_t b0_lean_launches = 0, b0_general_launches = 0, b0_lean_guard_trips = 0;
    // (the fused shade launches of bounces 1 and 2 by variant - lean, k_wf_shade_fused<SB_VIS1 | SB_LEAN1> (8448) with its list pass behind it,
    // by bounce - 1, and general; the entries handed over are word 6 of those bounces' fused counter blocks.  pt_get_b1_lean_stats)
    uint64_t b1_lean_launches[2] = {0, 0}, b1_general_launches = 0;
    // The closest hits of the bounce-2 rays, same key: that ray is made from the bounce-1 hit, the material there and the
    // item's words - again no light, and the Russian roulette starts behind it - so what holds for bounce 1 holds one bounce
    // later.  In use in the frames hit1_cache serves that have a bounce 2; the record, the zeroing, the prefix, the counters
    // and hit2_unknown as for hit1_cache (render_chunk drives both from one table, WfFrame::bounce_hits).
    // (hit2_unknown: eight uint64 - behind the counter of unknown casts, what the bounce-1 shade launches that read the
    // bounce-1 visibility and this plane themselves counted, k_wf_shade_fused in pt_wavefront.h; b1_fused_launches: the
    // chunks that took that kernel.  pt_get_bounce1_fused_stats.  Allocated with either cache.)
    FrameCache hit2_cache;
    DeviceBuffer hit2_unknown;
    uint64_t b1_fused_launches = 0;
    // The answers of the bounce-1 shadow casts of ONE view, ONE material table and ONE set of light positions: the casts
    // k_og_shadow makes for the surfaces bounce 1 reached - those depend on what hit1_cache's key holds - towards lights whose
    // kind and position are in the key, colour and intensity not.  One byte per item in vis_cache's encoding, indexed by the
    // sample's slot in its batch's staging area (the shadow record carries that, not the item: a bijection onto the batch's
    // valid items that the enumeration fixes), no mark; k_og_shadow_vis reads a record's byte, casts for what is unknown
    // and writes the byte back.  counter[0], [1]: times the plane was zeroed / launches of the variant.
    FrameCache vis1_cache;
    // The same pairing for the bounces behind them, by bounce: the closest hits of the rays of bounces 3-5 (tail_hits[b - 3];
    // the roulette of bounces 4+ draws from the item's words, so the bounce-1 hits' key holds for every later bounce) and the
    // shadow visibility of bounces 2-4 (tail_vis[b - 2]; vis1_cache's key, encoding and index).  One plane, one event and one
    // block of device counters each.  hits_unknown(b): eight uint64 - [0] the casts the loading launches of bounce b left to
    // k_wf_trace_exact, [1..5] what the shade launches of bounce b - 1 that read that bounce's visibility themselves counted
    // (k_wf_shade_fused; hit2_unknown above is hits_unknown(2)); fused_launches(b): the chunks whose bounce-b shade pass took
    // that kernel.  hits_cache(b), vis_cache_of(b): the table by bounce, bounces 1 and 2 included (pt_get_bounce_*_stats).
    static constexpr uint32_t HIT_BOUNCES = 6;   // bounces 1-5 have a hit cache, bounces 1-4 a visibility cache
    FrameCache tail_hits[HIT_BOUNCES - 3], tail_vis[HIT_BOUNCES - 3];
    DeviceBuffer tail_unknown[HIT_BOUNCES - 3];
    uint64_t tail_fused_launches[HIT_BOUNCES - 3] = {0, 0, 0};
    FrameCache& hits_cache(uint32_t b) { return b == 1u ? hit1_cache : b == 2u ? hit2_cache : tail_hits[b - 3u]; }
    const FrameCache& hits_cache(uint32_t b) const { return const_cast<pt_scene*>(this)->hits_cache(b); }
    DeviceBuffer& hits_unknown(uint32_t b) { return b == 1u ? hit1_unknown : b == 2u ? hit2_unknown : tail_unknown[b - 3u]; }
    const DeviceBuffer& hits_unknown(uint32_t b) const { return const_cast<pt_scene*>(this)->hits_unknown(b); }
    FrameCache& vis_cache_of(uint32_t b) { return b == 1u ? vis1_cache : tail_vis[b - 2u]; }
    const FrameCache& vis_cache_of(uint32_t b) const { return const_cast<pt_scene*>(this)->vis_cache_of(b); }
    uint64_t& fused_launches(uint32_t b) { return b == 1u ? b1_fused_launches : tail_fused_launches[b - 2u]; }
    uint64_t fused_launches(uint32_t b) const { return b == 1u ? b1_fused_launches : tail_fused_launches[b - 2u]; }
    std::vector<DevLight> host_lights;  // the lights as the device has them (the visibility cache's key)
    uint64_t camera_generation = 0;   // bumped by pt_scene_set_camera
    uint64_t material_generation = 0;   // bumped by pt_scene_set_materials
    uint64_t queue_bytes_last = 0;   // bytes of the path queues of the last frame (pt_scene_get_info)
    uint32_t queue_chunk_last = 0, frame_planned_last = 0;
    // escape masks: wanted (PT_ESCAPE), built when the scene has rendered `escape_after` frames of the default pipeline
    bool escape_wanted = false, escape_tried = false;
    uint32_t escape_after = 2;
    float escape_delta = 0.f;   // the delta_in the masks were built with (pt_scene_set_camera keeps them while a camera needs no more)
    uint32_t frames_rendered = 0;
    int trace_blocks = 0, shadow_blocks = 0, n_cu = 0;
    uint32_t wf_cap_ok = 0;   // largest queue capacity the device provided so far (0: not tried)
    // tile tables of the sharded renders, one per configuration (image size, rank, count, tile size) and never rewritten:
    // pt_render_device is asynchronous, two calls for different ranks may be in flight on the caller's streams at once
    typedef std::tuple<uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t> TileKey;
    std::map<TileKey, std::unique_ptr<DeviceBuffer>> tile_tables;
    std::vector<hipEvent_t> events;

    ~pt_scene() {
        (void)hipSetDevice(device);
        frame_state.stats.clear();
        tile_frame_stats.reset();
        for (void* p : allocations) (void)hipFree(p);
        for (hipEvent_t e : events) (void)hipEventDestroy(e);
        for (hipEvent_t e : {pipe.ev_shade, pipe.ev_shadow, pipe.ev_rng, pipe.ev_chunk, pipe.ev_trace, pipe.ev_wide, pipe.ev_exact, pipe.ev_exact_go})
            if (e) (void)hipEventDestroy(e);
        if (pipe.side_exact) (void)hipStreamDestroy(pipe.side_exact);
        if (pipe.side) (void)hipStreamDestroy(pipe.side);
        if (pipe.side_wide) (void)hipStreamDestroy(pipe.side_wide);
    }
    // Free one of the scene's device allocations (nullptr: nothing).
    void release(const void* q) {
        if (!q) return;
        auto it = std::find(allocations.begin(), allocations.end(), q);
        if (it != allocations.end()) allocations.erase(it);
        (void)hipFree(const_cast<void*>(q));
    }
    template <class T>
    const T* upload(const T* host, size_t count) {
        size_t bytes = std::max<size_t>(16, count * sizeof(T));
        void* d = nullptr;
        HIP_CHECK(hipMalloc(&d, bytes));
        allocations.push_back(d);
        if (count) HIP_CHECK(hipMemcpy(d, host, count * sizeof(T), hipMemcpyHostToDevice));
        info.device_bytes += bytes;
        return (const T*)d;
    }
};

namespace {

void select_device(int device) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n == 0) fail(PT_ERR_DEVICE, "no HIP device available (%s)", hipGetErrorString(e));
    if (device >= n) fail(PT_ERR_DEVICE, "device %d out of range (%d devices)", device, n);
    if (device >= 0) HIP_CHECK(hipSetDevice(device));
}

}  // namespace

// Everything pt_scene_create computes on the HOST: validated copies of the small tables, the KD-tree in device
// layout, the per-primitive arrays, the origin grids.  Built once per process and uploaded to as many devices as
// the caller renders on (the CLI's --devices, a multi-GPU host): the KD build and the grid builds are seconds of
// CPU work that do not depend on the device.
struct pt_prep {
    std::vector<pth_kd_node> nodes;            // treelet order (see below)
    std::vector<float4> leaf, attr, pos;
    std::vector<uint2> entry_lists;            // entry lists of the KD-tree (csrc/pt_wavefront.h trav_enter) ...
    std::vector<uint32_t> prim_entry;          // ... and the word (list offset << 6 | entries) of every primitive
    std::vector<pt_material> model_mat;
    std::vector<pt_texture> textures;
    std::vector<uint8_t> texels;
    std::vector<DevLight> lights;
    float lut[256];
    DevScene dev{};                            // scalars filled in; pointers are set per device
    pt_scene_info info{};
    struct Grid {
        pth_origin_grid g{};
        Grid() = default;
        Grid(const Grid&) = delete;
        Grid& operator=(const Grid&) = delete;
        ~Grid() { pth_origin_grid_free(&g); }
    };
    std::unique_ptr<Grid> cam_grid;
    std::vector<std::unique_ptr<Grid>> light_grids;
    bool all_lights_gridded = false;
    // grids built on the device at upload time (csrc/pt_grid_build.h; PT_OG_HOST=1: built here, on the host, as above):
    // what every grid needs beside the primitives - its parameters and header - and the primitives' geometry as the
    // footprints take it (9 floats: three positions, or centre + radius), with the id | sphere-bit word
    struct GridJob {
        pth::og::GridParams params;
        pth_origin_grid hdr{};
        bool valid = false;
    };
    GridJob cam_job;
    std::vector<GridJob> light_jobs;
    std::shared_ptr<CamGridSource> src = std::make_shared<CamGridSource>();   // og_geom, og_words (+ what an edit needs)
};

namespace {

// pt_scene_create makes its prep for exactly one scene: the prep's grid thread then builds that scene's grids on the device
// WHILE the KD-tree is being built on the host, and scene_upload finds them here.
struct EarlyGrids {
    pt_scene& scene;
    int device;
    SceneGrids grids;
    bool built = false;
};

SceneGrids grids_on_device(const pt_prep& P, pt_scene& s);

// A light as the device reads it (tame: every colour component finite and below 1e30).
DevLight dev_light(const pt_light& l) {
    DevLight o{};
    o.kind = l.kind;
    memcpy(o.vec, l.vec, 12);
    memcpy(o.color, l.color, 12);
    o.tame = 1u;
    for (int k = 0; k < 3; ++k)
        if (!(fabsf(l.color[k]) < 1e30f)) o.tame = 0u;  // also catches NaN
    return o;
}

// A camera as the device reads it: the columns of its transform, Rad::tan(fov / 2.) (mod.rs:116,120) with the host libm.
void dev_camera(const pt_camera& cam, DevScene& D) {
    const float* M = cam.transform;
    memcpy(D.cam_c0, M, 12);
    memcpy(D.cam_c1, M + 4, 12);
    memcpy(D.cam_c2, M + 8, 12);
    memcpy(D.cam_c3, M + 12, 12);
    D.tan_half_fov = tanf(cam.fov / 2.f);
}

// Byte budget over ALL grids of the scene (PT_OG_BUDGET_GIB, default 48 of the 288 GB): the grids are an optional
// accelerator in front of the KD-tree, one per camera and per light, 6 res^2 cells of 4 B plus ~1.5x that in list
// entries each (8192^2: ~4 GB a grid) - a scene with many lights must not run the host or the device out of
// memory over them.  The resolution is halved (down to 512) until the estimate fits; if it still does not, or
// the grids as built exceed the budget, the lights go without (their shadow rays take the KD-tree).  Evaluated by
// prep_create, and again by pt_scene_set_lights for the new light count.
struct GridRule {
    uint32_t res = 0;         // the camera grid's resolution
    uint32_t light_res = 0;   // the light grids' (PT_OG_RES_LIGHT: experiments - a resolution of their own)
    bool cam_fits = false;    // the camera grid's estimate fits the budget
    bool lights_fit = false;  // every grid's estimate at `res` fits the budget
    uint32_t cam_res = 0;     // res if a camera grid is to be had at all (PT_OG, primitives, budget), else 0
    bool lights = false;      // the lights get grids (if every one of them can have one)
};
double grid_estimate(uint32_t r) { return 6.0 * r * r * 4.0 * 2.5; }
GridRule grid_rule(uint64_t n_prims, uint32_t n_lights, double budget, bool grids_on) {
    GridRule R;
    uint32_t res = pth_origin_grid_auto_resolution(n_prims);
    const double n_grids = 1.0 + n_lights;
    while (res > 512u && grid_estimate(res) * n_grids > budget) res >>= 1;
    R.lights_fit = grid_estimate(res) * n_grids <= budget;
    R.light_res = [&] {
        const char* e = getenv("PT_OG_RES_LIGHT");
        return e && *e && atoi(e) >= 32 ? (uint32_t)atoi(e) : res;
    }();
    if (!R.lights_fit) {   // the camera grid alone, at the resolution it is worth having
        res = pth_origin_grid_auto_resolution(n_prims);
        while (res > 512u && grid_estimate(res) > budget) res >>= 1;
    }
    R.res = res;
    R.cam_fits = grid_estimate(res) <= budget;
    R.cam_res = grids_on && n_prims > 0 && R.cam_fits ? res : 0u;
    R.lights = grids_on && n_prims > 0 && R.lights_fit;
    return R;
}

// ---- the grid of the camera and of a light, each said once.  `ext` is where the scene's extent about the grid comes from,
// and with it what becomes of the parameters: the description, scanned on the host (DescJobs: the jobs of a fresh scene's
// device build; HostBuilt: the host builder, PT_OG_HOST=1), or the footprints, reduced on the device (EditFootprints: the
// edits).  The numbers are the same; a path's source decides what its setup time overlaps with.

// A point light's shadow ray starts n * 1e-5 off the line through the light (mod.rs:319): the grids' margin covers
// |n| <= max_normal, longer normals take the KD-tree per surface (DevScene.light_grid_max_normal2).
constexpr float max_normal = 1.5f;

// A cube map around a point light; an orthographic grid along a directional light's shadow rays, which run along
// -direction (mod.rs:291), as it is.
template <class Ext>
auto light_grid(uint32_t kind, const float vec[3], uint32_t light_res, Ext&& ext) {
    if (kind == PT_LIGHT_POINT) return ext.point(vec, light_res, 1.05e-5f * max_normal, 1.001f);
    const float sd[3] = {-1.f * vec[0], -1.f * vec[1], -1.f * vec[2]};
    return ext.ortho(sd, light_res);
}

// A cube map around the camera of transform M, for directions as long as a camera ray's can be: |M dir| <= ||M||_F for the
// unit vector dir (mod.rs:122-123).  A norm that is not in (0, 64): no grid (what `ext` gives by default).
template <class Ext>
auto camera_grid(const float* M, uint32_t res, Ext&& ext) -> decltype(ext.point(M, res, 0.f, 0.f)) {
    double fro = 0;
    for (int k = 0; k < 3; ++k)
        for (int r = 0; r < 3; ++r) fro += (double)M[4 * k + r] * M[4 * k + r];
    fro = std::sqrt(fro);
    if (!(fro > 0 && fro < 64.0)) return {};
    return ext.point(M + 12, res, 0.f, (float)(fro * 1.001));
}

struct DescJobs {
    const pt_scene_desc& d;
    pt_prep::GridJob point(const float o[3], uint32_t res, float ray_offset, float max_dir_len) const {
        pt_prep::GridJob job;
        job.valid = pth::og_params_point(d, o, res, ray_offset, max_dir_len, job.params, job.hdr);
        return job;
    }
    pt_prep::GridJob ortho(const float sd[3], uint32_t res) const {
        pt_prep::GridJob job;
        job.valid = pth::og_params_ortho(d, sd, res, job.params, job.hdr);
        return job;
    }
};

struct HostBuilt {
    const pt_scene_desc& d;
    std::string what;   // (of the error message)
    void check(int rc) const {
        if (rc != PT_OK) fail(PT_ERR_INVALID, "origin grid (%s): %s", what.c_str(), pth_last_error());
    }
    std::unique_ptr<pt_prep::Grid> point(const float o[3], uint32_t res, float ray_offset, float max_dir_len) const {
        auto g = std::make_unique<pt_prep::Grid>();
        check(pth_origin_grid_build(&d, o, res, ray_offset, max_dir_len, &g->g));
        return g;
    }
    std::unique_ptr<pt_prep::Grid> ortho(const float sd[3], uint32_t res) const {
        auto g = std::make_unique<pt_prep::Grid>();
        check(pth_ortho_grid_build(&d, sd, res, &g->g));
        return g;
    }
};

struct Join {   // (an exception on the way out must not leave the thread behind)
    std::future<void>& f;
    ~Join() { if (f.valid()) f.wait(); }
};

// ---- prep_create, stage by stage

// validation, and what pt_scene_set_materials checks a new table against and resolves it through
void prep_tables(const pt_scene_desc& d, pt_prep& P) {
    for (uint32_t m = 0; m < d.n_models; ++m) {
        const pt_model& mo = d.models[m];
        if (mo.material < 0 || (uint32_t)mo.material >= d.n_materials) fail(PT_ERR_INVALID, "model %u: bad material index", m);
        if (mo.kind == PT_MODEL_MESH && (uint64_t)mo.tri_first + mo.tri_count > d.n_triangles)
            fail(PT_ERR_INVALID, "model %u: triangle range out of bounds", m);
        if (mo.kind != PT_MODEL_MESH && mo.kind != PT_MODEL_SPHERE) fail(PT_ERR_INVALID, "model %u: bad kind", m);
    }
    pth::check_materials(d.materials, d.n_materials, d.textures, d.n_textures, d.n_texel_bytes);
    P.src->model_material.resize(d.n_models);
    for (uint32_t m = 0; m < d.n_models; ++m) P.src->model_material[m] = d.models[m].material;
    P.src->n_materials = d.n_materials;
    P.src->textures.assign(d.textures, d.textures + d.n_textures);
    P.src->n_texel_bytes = d.n_texel_bytes;
}

// The per-primitive arrays (attributes, positions, the grids' footprints) and the per-model materials; true: some material
// is translucent.
bool prep_primitives(const pt_scene_desc& d, uint64_t n_prims, pt_prep& P) {
    std::vector<float4>&attr = P.attr, &pos = P.pos;
    attr.resize(n_prims * 4);
    pos.resize(n_prims * 3);
    P.src->og_geom.resize(n_prims * 9);
    P.src->og_words.resize(n_prims);
    P.model_mat.resize(d.n_models);
    bool translucent = false;
    uint64_t prim = 0;
    for (uint32_t m = 0; m < d.n_models; ++m) {
        const pt_model& mo = d.models[m];
        P.model_mat[m] = d.materials[mo.material];
        if (P.model_mat[m].opacity != 1.0f || P.model_mat[m].tex_opacity >= 0) translucent = true;
        float mbits;
        memcpy(&mbits, &m, 4);
        if (mo.kind == PT_MODEL_MESH) {
            for (uint32_t t = 0; t < mo.tri_count; ++t, ++prim) {
                const float* v = d.triangles + (size_t)(mo.tri_first + t) * 24;
                const float *a = v, *b = v + 8, *c = v + 16;
                attr[prim * 4 + 0] = make_float4(a[3], a[4], a[5], a[6]);
                attr[prim * 4 + 1] = make_float4(b[3], b[4], b[5], a[7]);
                attr[prim * 4 + 2] = make_float4(c[3], c[4], c[5], b[6]);
                attr[prim * 4 + 3] = make_float4(b[7], c[6], c[7], mbits);
                float e1[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]};
                float e2[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
                uint32_t pid = (uint32_t)prim;
                float pbits;
                memcpy(&pbits, &pid, 4);
                pos[prim * 3 + 0] = make_float4(a[0], a[1], a[2], pbits);
                pos[prim * 3 + 1] = make_float4(e1[0], e1[1], e1[2], e2[0]);
                pos[prim * 3 + 2] = make_float4(e2[1], e2[2], 0.f, 0.f);
                float* og = &P.src->og_geom[prim * 9];
                og[0] = a[0]; og[1] = a[1]; og[2] = a[2];
                og[3] = b[0]; og[4] = b[1]; og[5] = b[2];
                og[6] = c[0]; og[7] = c[1]; og[8] = c[2];
                P.src->og_words[prim] = pid;
            }
        } else {
            attr[prim * 4 + 0] = make_float4(mo.center[0], mo.center[1], mo.center[2], mo.radius);
            attr[prim * 4 + 1] = attr[prim * 4 + 2] = make_float4(0, 0, 0, 0);
            attr[prim * 4 + 3] = make_float4(0, 0, 0, mbits);
            uint32_t pid = (uint32_t)prim | PT_PRIM_SPHERE;
            float pbits;
            memcpy(&pbits, &pid, 4);
            pos[prim * 3 + 0] = make_float4(mo.center[0], mo.center[1], mo.center[2], pbits);
            pos[prim * 3 + 1] = make_float4(mo.radius, 0, 0, 0);
            pos[prim * 3 + 2] = make_float4(0, 0, 0, 0);
            float* og = &P.src->og_geom[prim * 9];
            og[0] = mo.center[0]; og[1] = mo.center[1]; og[2] = mo.center[2]; og[3] = mo.radius;
            og[4] = og[5] = og[6] = og[7] = og[8] = 0.f;
            P.src->og_words[prim] = pid;
            ++prim;
        }
    }
    return translucent;
}

// The triangles no model owns (pt_scene_set_camera: the extent of a camera grid includes them, as og_params_point's does).
void prep_unowned(const pt_scene_desc& d, pt_prep& P) {
    std::vector<uint8_t> owned(d.n_triangles, 0);
    for (uint32_t m = 0; m < d.n_models; ++m)
        if (d.models[m].kind == PT_MODEL_MESH)
            std::fill(owned.begin() + d.models[m].tri_first, owned.begin() + d.models[m].tri_first + d.models[m].tri_count, (uint8_t)1);
    for (uint64_t t = 0; t < d.n_triangles; ++t)
        if (!owned[t])
            for (int k = 0; k < 3; ++k)
                for (int a = 0; a < 3; ++a) P.src->unowned.push_back(d.triangles[t * 24 + k * 8 + a]);
}

// kdtree-ray's slab test (scene_slab, pt_integrator.h): the exact bounding box of the scene - the union of
// Model::bound() (model.rs:76-86: the positions' bounds for a mesh, centre -+ radius for a sphere).  A cast whose origin
// is not strictly inside it runs the test once, at its end (hit_passes_slab).
void prep_slab_box(const pt_scene_desc& d, DevScene& D) {
    for (int a = 0; a < 3; ++a) {
        D.slab_min[a] = INFINITY;
        D.slab_max[a] = -INFINITY;
    }
    for (uint32_t m = 0; m < d.n_models; ++m) {
        const pt_model& mo = d.models[m];
        const uint32_t cnt = mo.kind == PT_MODEL_MESH ? mo.tri_count : 1u;
        for (uint32_t t = 0; t < cnt; ++t) {
            for (int a = 0; a < 3; ++a) {
                float lo, hi;
                if (mo.kind == PT_MODEL_MESH) {
                    const float* v = d.triangles + (size_t)(mo.tri_first + t) * 24;
                    lo = fminf(fminf(v[a], v[8 + a]), v[16 + a]);
                    hi = fmaxf(fmaxf(v[a], v[8 + a]), v[16 + a]);
                } else {
                    lo = mo.center[a] - mo.radius;
                    hi = mo.center[a] + mo.radius;
                }
                D.slab_min[a] = fminf(D.slab_min[a], lo);
                D.slab_max[a] = fmaxf(D.slab_max[a], hi);
            }
        }
    }
}

// The grid jobs of a scene whose grids the device builds at upload time: only their parameters are derived here.
void prep_grid_jobs(const pt_scene_desc& d, const GridRule& rule, pt_prep& P) {
    if (rule.cam_res) P.cam_job = camera_grid(d.camera.transform, rule.cam_res, DescJobs{d});
    bool all = rule.lights;   // (no lights at all: vacuously)
    for (uint32_t i = 0; i < d.n_lights && all; ++i) {
        P.light_jobs.push_back(light_grid(d.lights[i].kind, d.lights[i].vec, rule.light_res, DescJobs{d}));
        all = P.light_jobs.back().valid;
    }
    if (!all) P.light_jobs.clear();
    P.all_lights_gridded = all;
}

// PT_OG_HOST=1: the grids built here, by the host builder.
void prep_host_grids(const pt_scene_desc& d, const GridRule& rule, pt_prep& P) {
    // (the camera grid on a thread of its own beside the light grids: every grid is its own count / scan / fill / sort)
    std::future<void> cam_done;
    if (rule.cam_res)
        cam_done = std::async(std::launch::async, [&P, &d, &rule] { P.cam_grid = camera_grid(d.camera.transform, rule.cam_res, HostBuilt{d, "camera"}); });
    Join join_cam{cam_done};
    // lights: all or none (light_grids_build), within the budget as built too
    const double budget = P.src->budget;
    double grid_bytes = 0;
    bool all = rule.lights;   // (no lights at all: vacuously)
    for (uint32_t i = 0; i < d.n_lights && all; ++i) {
        P.light_grids.push_back(light_grid(d.lights[i].kind, d.lights[i].vec, rule.light_res, HostBuilt{d, "light " + std::to_string(i)}));
        const pth_origin_grid& g = P.light_grids.back()->g;
        if (!g.enabled) all = false;
        grid_bytes += 4.0 * g.n_cells + 8.0 * g.n_refs;
        if (grid_bytes > budget) all = false;   // (the lists came out longer than estimated)
    }
    if (cam_done.valid()) {
        cam_done.get();
        if (P.cam_grid && P.cam_grid->g.enabled) {
            grid_bytes += 4.0 * P.cam_grid->g.n_cells + 8.0 * P.cam_grid->g.n_refs;
            if (grid_bytes > budget) all = false;
        }
    }
    if (!all) P.light_grids.clear();
    P.all_lights_gridded = all;
}

// ---- origin grids (host/origin_grid.cpp, csrc/pt_grid.h): camera rays, shadow rays of the lights.  They depend on the
// scene description only, not on the KD-tree: prep_create runs this on a thread of its own BESIDE the KD build (both are
// seconds of multi-threaded host work; setup of config 3: 3.2 -> 2.3 s).  For the one scene of pt_scene_create (`early`) the
// device build follows at once, on this thread.
void prep_grids(const pt_scene_desc& d, uint64_t n_prims, pt_prep& P, EarlyGrids* early) {
    auto t_grid = std::chrono::steady_clock::now();
    static const bool grids_on = [] {
        const char* e = getenv("PT_OG");
        return !(e && *e && atoi(e) == 0);
    }();
    // the byte budget over all grids of the scene and the resolutions it leaves (grid_rule)
    static const double budget = [] {
        const char* e = getenv("PT_OG_BUDGET_GIB");
        const double g = e && *e ? atof(e) : 48.0;
        return (g > 0 ? g : 48.0) * 1073741824.0;
    }();
    static const bool host_grids = [] {
        const char* e = getenv("PT_OG_HOST");
        return e && *e && atoi(e) != 0;
    }();
    const GridRule rule = grid_rule(n_prims, d.n_lights, budget, grids_on);
    P.src->cam_res = rule.cam_res;
    P.src->grids_on = grids_on;
    P.src->budget = budget;
    P.src->device_grids = !host_grids;
    host_grids ? prep_host_grids(d, rule, P) : prep_grid_jobs(d, rule, P);
    P.info.grid_build_seconds = std::chrono::duration<float>(std::chrono::steady_clock::now() - t_grid).count();
    if (early && !host_grids) {
        select_device(early->device);
        int cur = 0;
        HIP_CHECK(hipGetDevice(&cur));
        early->scene.device = cur;
        early->grids = grids_on_device(P, early->scene);
        early->built = true;
    }
}

// The leaf records in leaf-reference order and the small tables.
void prep_leaf_tables(const pt_scene_desc& d, const pth_kdtree& kd, pt_prep& P) {
    const std::vector<float4>& pos = P.pos;
    P.leaf.resize(kd.n_refs * 3);
    for (uint64_t r = 0; r < kd.n_refs; ++r) {
        uint32_t p = kd.refs[r];
        P.leaf[r * 3 + 0] = pos[(size_t)p * 3 + 0];
        P.leaf[r * 3 + 1] = pos[(size_t)p * 3 + 1];
        P.leaf[r * 3 + 2] = pos[(size_t)p * 3 + 2];
    }
    // sRGB -> linear table: (c as f32 / 255.0).powf(2.2) with the host libm (material.rs:137-141)
    for (int c = 0; c < 256; ++c) P.lut[c] = powf((float)c / 255.0f, 2.2f);
    P.lights.resize(d.n_lights);
    for (uint32_t i = 0; i < d.n_lights; ++i) P.lights[i] = dev_light(d.lights[i]);
    P.textures.assign(d.textures, d.textures + d.n_textures);
    P.texels.assign(d.texels, d.texels + d.n_texel_bytes);
}

// The device node layout.  The builder emits DFS order (below child = next node); on the GPU the
// walk is bound by cache-line round trips (a wave waits for the slowest of ~43 scattered node
// fetches), so the nodes are re-laid out in treelets: sibling PAIRS are adjacent (children of a
// node = pair, pair + 1) and the pairs of a 4-level subtree are packed consecutively, so that
// one 128-byte line serves up to four steps of a walk.  Node words: interior (split,
// pair << 2 | axis), leaf (first record, n << 2 | 3) as before.
// Returns the device slot of every builder (DFS) node number.
std::vector<uint32_t> prep_treelets(const pth_kdtree& kd, pt_prep& P) {
    std::vector<pth_kd_node>& tre = P.nodes;
    tre.assign(std::max<uint64_t>(kd.n_nodes, 1) + 1, pth_kd_node{0u, 0u});
    std::vector<uint32_t> new_index(kd.n_nodes, 0xffffffffu);   // builder (DFS) node number -> device slot
    const pth_kd_node* N = kd.nodes;
    const int H = 4;  // treelet height: 2 + 4 + 8 = 14 nodes = 112 B below the treelet root pair
    if (kd.n_nodes == 0) {
        tre[0] = pth_kd_node{0u, 3u};
    } else {
        new_index[0] = 0;
        uint32_t next = 2;  // pairs start at even indices; slot 1 pads the root
        std::vector<uint32_t> cluster_roots{0}, frontier, level;
        size_t cr = 0;
        while (cr < cluster_roots.size()) {
            level.assign(1, cluster_roots[cr++]);
            for (int depth = 0; depth < H && !level.empty(); ++depth) {
                frontier.clear();
                for (uint32_t n : level) {
                    if ((N[n].w1 & 3u) == 3u) continue;
                    uint32_t below = n + 1, above = N[n].w1 >> 2;
                    new_index[below] = next;
                    new_index[above] = next + 1;
                    next += 2;
                    frontier.push_back(below);
                    frontier.push_back(above);
                }
                level.swap(frontier);
            }
            // whatever is left at the bottom of this treelet starts new treelets
            for (uint32_t n : level)
                if ((N[n].w1 & 3u) != 3u) cluster_roots.push_back(n);
        }
        if (next > tre.size()) tre.resize(next);
        if (next >= (1u << 29)) fail(PT_ERR_UNSUPPORTED, "KD-tree has too many nodes");
        for (uint64_t n = 0; n < kd.n_nodes; ++n) {
            pth_kd_node nd = N[n];
            if ((nd.w1 & 3u) != 3u) nd.w1 = (new_index[n + 1] << 2) | (nd.w1 & 3u);
            tre[new_index[n]] = nd;
        }
        tre[1] = pth_kd_node{0u, 3u};
    }
    return new_index;
}

// The entry lists (trav_enter, csrc/pt_wavefront.h).  A path's next ray starts ON the primitive it just hit
// (origin = hit point + interpolated normal * 1e-5, mod.rs:266-268), deep inside the tree: of the ~23 nodes such a
// cast visits, the first ~15 are the descent from the root to the small node around its origin - a chain of
// dependent 8-byte fetches during which nothing is decided that the origin's whereabouts do not already say, except
// which far children the ray will come back to.  So every primitive gets its HOME NODE - the deepest node whose box
// holds every origin a hit on the primitive can produce - and the list of the home node's ancestors, root first:
// (split, far child << 3 | near child is the below child << 2 | axis).  The cast reads that list (contiguous, all
// loads in flight together), pushes the far children its ray reaches, and starts walking at the home node.  The
// lists are shared by the primitives of a home node (a few MB in all).  Nothing here is load-bearing for
// correctness: the cast checks that its origin lies on the near side of every listed plane and starts at the root
// otherwise, so the region below is an estimate that only has to be right most of the time.
void prep_entry_lists(const pt_scene_desc& d, const pth_kdtree& kd, const std::vector<uint32_t>& new_index, uint64_t n_prims, pt_prep& P) {
    P.prim_entry.assign(n_prims, 0u);
    P.entry_lists.clear();
    if (kd.n_nodes > 0 && n_prims > 0) {
        const pth_kd_node* N = kd.nodes;
        double ext = 0;
        for (int a = 0; a < 3; ++a)
            ext = std::max({ext, (double)fabsf(kd.bounds_min[a]), (double)fabsf(kd.bounds_max[a]), (double)fabsf(d.camera.transform[12 + a])});
        const float eps = (float)(2.5e-7 * std::max(ext, 1e-3));   // ~2 ulps of the largest coordinate: the rounding of o + d * t
        std::unordered_map<uint32_t, uint32_t> word_of_home;     // home node (builder numbering) -> entry word
        uint32_t path[PT_KD_STACK + 1];
        uint64_t q = 0;
        for (uint32_t m = 0; m < d.n_models; ++m) {
            const pt_model& mo = d.models[m];
            const uint32_t cnt = mo.kind == PT_MODEL_MESH ? mo.tri_count : 1u;
            for (uint32_t t = 0; t < cnt; ++t, ++q) {
                float lo[3], hi[3];
                for (int a = 0; a < 3; ++a) {
                    if (mo.kind == PT_MODEL_MESH) {
                        const float* v = d.triangles + (size_t)(mo.tri_first + t) * 24;
                        const float nl = fminf(fminf(v[3 + a], v[11 + a]), v[19 + a]), nh = fmaxf(fmaxf(v[3 + a], v[11 + a]), v[19 + a]);
                        lo[a] = fminf(fminf(v[a], v[8 + a]), v[16 + a]) + 1.05e-5f * nl - eps;
                        hi[a] = fmaxf(fmaxf(v[a], v[8 + a]), v[16 + a]) + 1.05e-5f * nh + eps;
                    } else {   // a sphere's hits: on the surface, pushed 1e-5 out (entry hit) or in (exit hit, model.rs:49-62)
                        lo[a] = mo.center[a] - mo.radius - 1.05e-5f - eps;
                        hi[a] = mo.center[a] + mo.radius + 1.05e-5f + eps;
                    }
                }
                uint32_t node = 0, depth = 0;
                while (lo[0] == lo[0] && hi[0] == hi[0]) {   // (a NaN region stays at the root)
                    const pth_kd_node nd = N[node];
                    const uint32_t axis = nd.w1 & 3u;
                    if (axis == 3u || depth >= 63u) break;
                    float split;
                    memcpy(&split, &nd.w0, 4);
                    uint32_t next;
                    if (hi[axis] < split) next = node + 1u;            // below child = next node (builder layout)
                    else if (lo[axis] > split) next = nd.w1 >> 2;      // above child
                    else break;
                    path[depth++] = node;
                    node = next;
                }
                auto it = word_of_home.find(node);
                if (it == word_of_home.end()) {
                    uint32_t word = 0u;
                    if (depth > 0) {
                        if (P.entry_lists.size() & 1u) P.entry_lists.push_back(make_uint2(0u, 0u));   // 16-byte aligned lists
                        const uint64_t off = P.entry_lists.size();
                        if (off + depth >= (1ull << 26)) fail(PT_ERR_UNSUPPORTED, "entry lists exceed 2^26 entries");
                        for (uint32_t k = 0; k < depth; ++k) {
                            const uint32_t anc = path[k], child = k + 1 < depth ? path[k + 1] : node;
                            const bool near_below = child == anc + 1u;
                            const uint32_t far_host = near_below ? (N[anc].w1 >> 2) : anc + 1u;
                            P.entry_lists.push_back(make_uint2(N[anc].w0, (new_index[far_host] << 3) | (near_below ? 4u : 0u) | (N[anc].w1 & 3u)));
                        }
                        word = (uint32_t)(off << 6) | depth;
                    }
                    it = word_of_home.emplace(node, word).first;
                }
                P.prim_entry[q] = it->second;
            }
        }
    }
    if (P.entry_lists.size() & 1u) P.entry_lists.push_back(make_uint2(0u, 0u));
    for (int k = 0; k < 8; ++k) P.entry_lists.push_back(make_uint2(0u, 0u));   // (the batched loads of trav_enter read up to 8 entries past a list's start)
}

// The DevScene scalars (the pointers are set per device) and the prep's rows of pt_scene_info.
void prep_scalars(const pt_scene_desc& d, const pth_kdtree& kd, uint64_t n_prims, bool translucent, pt_prep& P) {
    DevScene& D = P.dev;
    D.n_lights = d.n_lights;
    D.n_prims = (uint32_t)n_prims;
    D.n_nodes = (uint32_t)kd.n_nodes;
    D.n_node_slots = (uint32_t)P.nodes.size();
    D.has_translucent = translucent ? 1u : 0u;
    for (int a = 0; a < 3; ++a) {
        float pad = 1e-4f * std::max(fabsf(kd.bounds_min[a]), fabsf(kd.bounds_max[a])) + 1e-5f;
        D.bounds_min[a] = kd.bounds_min[a] - pad;
        D.bounds_max[a] = kd.bounds_max[a] + pad;
    }
    dev_camera(d.camera, D);
    memcpy(D.background, d.background, 12);
    D.light_grid_max_normal2 = max_normal * max_normal;
    P.info.n_prims = n_prims;
    P.info.n_kd_nodes = kd.n_nodes;
    P.info.n_kd_leaves = kd.n_leaves;
    P.info.n_leaf_refs = kd.n_refs;
    P.info.kd_depth = kd.depth;
    P.info.has_translucent = translucent;
    P.info.kd_build_seconds = (float)kd.build_seconds;
}

// `early`: the scene this prep is made for, when there is exactly one (pt_scene_create, EarlyGrids).
void prep_create(const pt_scene_desc& d, pt_prep& P, EarlyGrids* early = nullptr) {
    const bool dbg_setup = getenv("PT_DEBUG_SETUP") != nullptr;
    auto t_sec = std::chrono::steady_clock::now();
    auto section = [&](const char* name) {
        if (!dbg_setup) return;
        auto now = std::chrono::steady_clock::now();
        fprintf(stderr, "[prep] %-28s %.3f s\n", name, std::chrono::duration<double>(now - t_sec).count());
        t_sec = now;
    };
    prep_tables(d, P);
    const uint64_t n_prims = pth_prim_count(&d);
    const bool translucent = prep_primitives(d, n_prims, P);
    prep_unowned(d, P);
    prep_slab_box(d, P.dev);
    if (n_prims >= (1ull << 28)) fail(PT_ERR_UNSUPPORTED, "more than 2^28 primitives");   // (pack_hit's index bits)
    section("primitive arrays, scene box");
    std::future<void> grids_done = std::async(std::launch::async, [&d, &P, n_prims, early] { prep_grids(d, n_prims, P, early); });
    Join join_grids{grids_done};

    // ---- KD-tree
    pth_kdtree kd;
    if (pth_kd_build(&d, &kd) != PT_OK) fail(PT_ERR_INVALID, "KD build failed: %s", pth_last_error());
    std::unique_ptr<pth_kdtree, void (*)(pth_kdtree*)> kd_guard(&kd, pth_kd_free);
    if (kd.depth >= PT_KD_STACK) fail(PT_ERR_UNSUPPORTED, "KD-tree depth %u exceeds the traversal stack", kd.depth);

    section("KD build");
    prep_leaf_tables(d, kd, P);
    section("leaf records, tables");
    const std::vector<uint32_t> new_index = prep_treelets(kd, P);
    section("treelet layout");
    prep_entry_lists(d, kd, new_index, n_prims, P);
    prep_scalars(d, kd, n_prims, translucent, P);
    section("entry lists");
    grids_done.get();   // (rethrows what the grid thread threw)
    section("waiting for the grids");
}

// A mark in the scene's device allocations.  Unless it is released, its destructor frees what the scene has allocated since
// and gives info.device_bytes its value back: a grid that is not to be had, an edit that failed.
struct AllocMark {
    pt_scene& s;
    size_t mark;
    uint64_t bytes;
    bool released = false;
    explicit AllocMark(pt_scene& sc) : s(sc), mark(sc.allocations.size()), bytes(sc.info.device_bytes) {}
    void release() { released = true; }
    ~AllocMark() {
        if (released) return;
        while (s.allocations.size() > mark) {
            (void)hipFree(s.allocations.back());
            s.allocations.pop_back();
        }
        s.info.device_bytes = bytes;
    }
};

// The primitives' footprints (CamGridSource: og_geom, og_words) on a device for its grid builds, freed on every way out.
struct Footprints {
    float* geom = nullptr;
    uint32_t* words = nullptr;
    ~Footprints() {
        for (void* q : {(void*)geom, (void*)words})
            if (q) (void)hipFree(q);
    }
};

// What the kernels read of the grid of header `hdr` whose arrays are on the device.
DevGrid dev_grid_from(const pth_origin_grid& hdr, const uint32_t* cell_off, const uint2* refs) {
    DevGrid out{};
    out.cell_off = cell_off;
    out.refs = refs;
    out.res = hdr.res;
    out.n_global = hdr.n_global;
    out.half_res = 0.5f * (float)hdr.res;
    out.kind = hdr.kind;
    memcpy(out.axis_u, hdr.axis_u, 12);
    memcpy(out.axis_v, hdr.axis_v, 12);
    memcpy(out.axis_w, hdr.axis_w, 12);
    out.u0 = hdr.u0;
    out.v0 = hdr.v0;
    out.cells_per_unit = hdr.cells_per_unit;
    return out;
}

// One origin grid built on the device (csrc/pt_grid_build.h) from the parameters / header of `job`, over the footprints F.
// Returns false, and an empty slot, when the grid is not to be had - too many primitives every ray would have to test, more
// than 2^32 list entries, the byte budget of the scene's grids exceeded (`bytes_used`: what the grids before it took), or the
// device out of memory: the casts it would have served take the KD-tree.  On success the two arrays belong to the scene
// (s.allocations).
bool device_grid_build(pt_scene& s, const pt_prep::GridJob& job, const Footprints& F, const CamGridSource& src, double& bytes_used,
                       GridSlot& out) {
    out = GridSlot{};
    const uint32_t n_prims = (uint32_t)src.og_words.size();
    if (!job.valid || n_prims == 0) return false;
    static const uint32_t max_global = [] {
        const char* e = getenv("PT_OG_MAX_GLOBAL");
        return (uint32_t)(e && *e ? std::max(0, atoi(e)) : 64);
    }();
    const pth::og::GridParams& G = job.params;
    pth_origin_grid hdr = job.hdr;
    const uint64_t n_cells = hdr.n_cells;
    const bool dbg = getenv("PT_DEBUG_SETUP") != nullptr;
    auto t_ph = std::chrono::steady_clock::now();
    auto phase = [&](const char* name) {
        if (!dbg) return;
        (void)hipDeviceSynchronize();
        auto now = std::chrono::steady_clock::now();
        fprintf(stderr, "[device grid %u] %-10s %.4f s\n", hdr.res, name, std::chrono::duration<double>(now - t_ph).count());
        t_ph = now;
    };
    uint32_t *cnt_base = nullptr, *d_glob = nullptr, *d_bsum = nullptr;
    uint2* d_refs = nullptr;
    auto cleanup = [&]() {
        for (void* q : {(void*)cnt_base, (void*)d_glob, (void*)d_bsum, (void*)d_refs})
            if (q) (void)hipFree(q);
        (void)hipGetLastError();
    };
    try {
        const size_t off_bytes = (n_cells + 2) * 4;
        if (bytes_used + (double)off_bytes > src.budget) return false;
        HIP_CHECK(hipMalloc((void**)&cnt_base, off_bytes));
        HIP_CHECK(hipMemsetAsync(cnt_base, 0, off_bytes, 0));
        const uint32_t glob_cap = max_global + 1u;
        HIP_CHECK(hipMalloc((void**)&d_glob, (glob_cap + 2u) * 4));   // [0] counter, [1] longest list, [2 ...] the list
        HIP_CHECK(hipMemsetAsync(d_glob, 0, (glob_cap + 2u) * 4, 0));
        phase("alloc");
        const dim3 pg((n_prims + 3u) / 4u);   // a wavefront per primitive
        hipLaunchKernelGGL((ogb::k_og_raster<0>), pg, dim3(256), 0, 0, G, F.geom, F.words, n_prims, cnt_base + 1, (uint2*)nullptr,
                           d_glob + 2, d_glob, glob_cap);
        HIP_CHECK(hipGetLastError());
        phase("count");
        const uint32_t n_blocks = (uint32_t)((n_cells + OG_SCAN_BLOCK - 1) / OG_SCAN_BLOCK);
        HIP_CHECK(hipMalloc((void**)&d_bsum, (size_t)n_blocks * 4));
        hipLaunchKernelGGL(ogb::k_og_block_sum, dim3(n_blocks), dim3(256), 0, 0, (const uint32_t*)(cnt_base + 1), n_cells, d_bsum);
        HIP_CHECK(hipGetLastError());
        std::vector<uint32_t> glob(glob_cap + 2u), bsum(n_blocks);
        HIP_CHECK(hipMemcpy(glob.data(), d_glob, glob.size() * 4, hipMemcpyDeviceToHost));
        const uint32_t n_global = glob[0];
        hdr.n_global = n_global;
        if (n_global > max_global) {   // (enabled = 0, as the host builder)
            cleanup();
            return false;
        }
        HIP_CHECK(hipMemcpy(bsum.data(), d_bsum, (size_t)n_blocks * 4, hipMemcpyDeviceToHost));
        uint64_t run = n_global;
        for (uint32_t b = 0; b < n_blocks; ++b) {   // exclusive prefix of the block sums, 64-bit
            const uint32_t v = bsum[b];
            if (run > 0xffffffffull) break;
            bsum[b] = (uint32_t)run;
            run += v == 0xffffffffu ? 0x100000000ull : v;   // (a saturated block sum: the grid is given up below)
        }
        const uint64_t total = run;
        if (total > 0xffffffffull || bytes_used + (double)off_bytes + 8.0 * (double)total > src.budget) {
            cleanup();
            return false;
        }
        HIP_CHECK(hipMemcpy(d_bsum, bsum.data(), (size_t)n_blocks * 4, hipMemcpyHostToDevice));
        hipLaunchKernelGGL(ogb::k_og_block_scan, dim3(n_blocks), dim3(256), 0, 0, cnt_base + 1, n_cells, (const uint32_t*)d_bsum);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipMalloc((void**)&d_refs, std::max<uint64_t>(1, total) * 8));
        phase("scan");
        if (n_global) {   // the global block in front: ascending primitive, bound 0 (as the host builder)
            std::vector<uint32_t> g(glob.begin() + 2, glob.begin() + 2 + n_global);
            std::sort(g.begin(), g.end());
            std::vector<uint2> front(n_global);
            for (uint32_t i = 0; i < n_global; ++i) front[i] = make_uint2(src.og_words[g[i]], 0u);
            HIP_CHECK(hipMemcpy(d_refs, front.data(), (size_t)n_global * 8, hipMemcpyHostToDevice));
        }
        hipLaunchKernelGGL((ogb::k_og_raster<1>), pg, dim3(256), 0, 0, G, F.geom, F.words, n_prims, cnt_base + 1, d_refs, d_glob + 2,
                           d_glob, glob_cap);
        HIP_CHECK(hipGetLastError());
        phase("fill");
        HIP_CHECK(hipMemcpy(cnt_base, &n_global, 4, hipMemcpyHostToDevice));   // word 0: where cell 0 starts
        hipLaunchKernelGGL(ogb::k_og_sort, dim3((uint32_t)((n_cells + 255) / 256)), dim3(256), 0, 0, (const uint32_t*)cnt_base, n_cells,
                           d_refs, d_glob + 1);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipMemcpy(&hdr.max_cell_refs, d_glob + 1, 4, hipMemcpyDeviceToHost));   // (also the synchronisation point)
        phase("sort");
        (void)hipFree(d_glob);
        (void)hipFree(d_bsum);
        d_glob = d_bsum = nullptr;
        s.allocations.push_back(cnt_base);
        s.allocations.push_back(d_refs);
        const double bytes = (double)off_bytes + 8.0 * (double)std::max<uint64_t>(1, total);
        bytes_used += bytes;
        hdr.n_refs = total;
        hdr.enabled = 1;
        out.dev = dev_grid_from(hdr, cnt_base, d_refs);
        out.hdr = hdr;
        out.bytes = (uint64_t)bytes;
        return true;
    } catch (const GpuError&) {
        cleanup();
        return false;
    }
}

// The light grids of a scene, built on its device into G: all or none - the shadow queue is consumed by ONE kernel, so the
// grids serve the shadow rays only when EVERY light has one (no lights at all: vacuously).  job(i) gives the parameters of
// light i of n; `all`: whether the lights are to have grids at all; `used`: what the camera grid took of the budget (it
// comes first).  At the first grid that is not to be had, those built are dropped.
template <class Job>
void light_grids_build(pt_scene& s, SceneGrids& G, size_t n, bool all, Job&& job, const Footprints& F, const CamGridSource& src,
                       double used) {
    G.lights.assign(n, GridSlot{});
    AllocMark mark(s);
    for (size_t i = 0; i < n && all; ++i) {
        const pt_prep::GridJob& j = job(i);
        all = device_grid_build(s, j, F, src, used, G.lights[i]);
    }
    if (all) mark.release();
    G.lights_done(all);
}

// Every origin grid of a scene of the prep, built on the device the calling thread has selected (the arrays go to
// s.allocations).  Needs of the prep only what prep_create has ready BEFORE the KD build: the grid jobs and the
// primitives' geometry - so pt_scene_create runs it on a thread of its own beside the KD build.
SceneGrids grids_on_device(const pt_prep& P, pt_scene& s) {
    auto t_grid = std::chrono::steady_clock::now();
    const CamGridSource& src = *P.src;
    SceneGrids G;
    G.headers = true;
    const size_t n_lights = P.light_jobs.size();   // (all of the scene's lights, or none: scene_upload has the slots of a scene without)
    G.lights.assign(n_lights, GridSlot{});
    {
        Footprints F;
        if ((P.cam_job.valid || n_lights) && !src.og_words.empty() && hipMalloc((void**)&F.geom, src.og_geom.size() * 4) == hipSuccess &&
            hipMalloc((void**)&F.words, src.og_words.size() * 4) == hipSuccess) {
            const bool copied = hipMemcpy(F.geom, src.og_geom.data(), src.og_geom.size() * 4, hipMemcpyHostToDevice) == hipSuccess &&
                                hipMemcpy(F.words, src.og_words.data(), src.og_words.size() * 4, hipMemcpyHostToDevice) == hipSuccess;
            double used = 0;
            if (copied) device_grid_build(s, P.cam_job, F, src, used, G.cam);
            light_grids_build(s, G, n_lights, copied && P.all_lights_gridded,
                              [&P](size_t i) -> const pt_prep::GridJob& { return P.light_jobs[i]; }, F, src, used);
        } else {
            (void)hipGetLastError();
            G.lights_done(n_lights == 0 && P.all_lights_gridded);   // (no lights at all: vacuously)
        }
    }
    G.seconds = std::chrono::duration<float>(std::chrono::steady_clock::now() - t_grid).count();
    return G;
}

// The delta_in of the escape masks of a scene (EscBuildParams): PT_SLACK_K x the largest distance a ray of the scene covers
// before it hits anything - the box diagonal, or camera to far corner - plus the rounding of the largest coordinate.
float escape_delta_in(const DevScene& D) {
    double diag2 = 0, cam2 = 0, amax = 0;
    for (int a = 0; a < 3; ++a) {
        const double w = (double)D.bounds_max[a] - D.bounds_min[a], c = D.cam_c3[a];
        const double far = std::max(std::fabs(c - D.bounds_min[a]), std::fabs(c - D.bounds_max[a]));
        diag2 += w * w;
        cam2 += far * far;
        amax = std::max({amax, std::fabs((double)D.bounds_min[a]), std::fabs((double)D.bounds_max[a]), std::fabs(c)});
    }
    const double reach = std::sqrt(std::max(diag2, cam2));
    return (float)((double)PT_SLACK_K * reach + 4.0 * 5.9604645e-8 * amax);
}

// The escape masks of a scene (pt_escape.h), built on its device from the uploaded arrays: one wavefront per primitive.  Blocks
// until they are there (every frame in flight has completed by then).  A device without the memory for them goes without.
void escape_masks_build(pt_scene& s) {
    s.escape_tried = true;
    DevScene& D = s.dev;
    const uint64_t n_prims = D.n_prims;
    auto t_esc = std::chrono::steady_clock::now();
    try {
        AllocMark mark(s);
        HIP_CHECK(hipSetDevice(s.device));
        void* buf = nullptr;
        HIP_CHECK(hipMalloc(&buf, n_prims * 80));
        s.allocations.push_back(buf);
        s.info.device_bytes += n_prims * 80;
        uint32_t* d_stats = nullptr;
        HIP_CHECK(hipMalloc((void**)&d_stats, 16));
        HIP_CHECK(hipMemset(d_stats, 0, 16));
        EscBuildParams E{};
        E.delta_in = escape_delta_in(D);
        E.slop_far = E.delta_in;
        E.alpha_stop = [] { const char* e = getenv("PT_ESCAPE_ALPHA"); return e && *e ? (float)atof(e) : 0.04f; }();
        E.r_near_scale = 2.0f;
        const uint32_t blocks = (uint32_t)std::min<uint64_t>((n_prims + 3) / 4, 256u * 64u);
        hipLaunchKernelGGL(k_escape_build, dim3(blocks), dim3(256), 0, 0, D, E, (float4*)buf, (uint32_t)n_prims, d_stats);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipDeviceSynchronize());
        uint32_t st[4] = {0, 0, 0, 0};
        HIP_CHECK(hipMemcpy(st, d_stats, 16, hipMemcpyDeviceToHost));
        (void)hipFree(d_stats);
        D.escape = (const float4*)buf;
        ++s.escape_generation;
        s.escape_delta = E.delta_in;
        s.info.escape_prims = st[0];
        s.info.escape_clear_fraction = st[0] ? (float)((double)st[1] / (384.0 * st[0])) : 0.f;
        mark.release();
    } catch (const GpuError&) {   // (no memory for them: the casts are simply made)
        D.escape = nullptr;
    }
    s.info.escape_build_seconds = std::chrono::duration<float>(std::chrono::steady_clock::now() - t_esc).count();
    // the counts of the frames rendered so far are upper bounds now (the masks end paths): the next frame counts again
    for (auto& kv : s.frame_state.stats) {
        pt_scene::FrameStats& f = *kv.second;
        f.pending = f.valid = f.planned = f.plan_failed = false;
    }
}

// What pt_scene_get_info reports of the grids, on top of an `out` that counts every other allocation.
void grid_facts(const SceneGrids& G, pt_scene_info& out) {
    out.cam_grid_res = G.cam.hdr.enabled ? G.cam.hdr.res : 0u;
    out.light_grids = G.all_lights ? (uint32_t)G.lights.size() : 0u;
    out.grid_refs = G.cam.hdr.enabled ? G.cam.hdr.n_refs : 0;
    out.device_bytes += G.cam.bytes;
    for (const GridSlot& g : G.lights) {
        out.grid_refs += g.hdr.enabled ? g.hdr.n_refs : 0;
        out.device_bytes += g.bytes;
    }
}

// The scene takes another camera grid / other light grids (an empty slot: none): the old arrays are freed, s.grids and what
// DevScene restates of it change together.  `table`: the new light slots' DevGrid[] on the device (light_grid_table) - the
// edits upload it while they still may fail.  Nothing here fails.
void install_camera_grid(pt_scene& s, const GridSlot& slot) {
    s.release(s.grids.cam.dev.cell_off);
    s.release(s.grids.cam.dev.refs);
    s.grids.cam = slot;
    s.dev.cam_grid = slot.dev;
}

const DevGrid* light_grid_table(pt_scene& s, const std::vector<GridSlot>& lights) {
    std::vector<DevGrid> table(lights.size());
    for (size_t i = 0; i < lights.size(); ++i) table[i] = lights[i].dev;
    return s.upload(table.data(), table.size());
}

void install_light_grids(pt_scene& s, const SceneGrids& from, const DevGrid* table) {
    for (const GridSlot& g : s.grids.lights) {
        s.release(g.dev.cell_off);
        s.release(g.dev.refs);
    }
    if (s.dev.light_grids) {
        s.release(s.dev.light_grids);
        s.info.device_bytes -= std::max<uint64_t>(16, s.grids.lights.size() * sizeof(DevGrid));
    }
    s.grids.lights = from.lights;
    s.grids.all_lights = from.all_lights;
    s.grids.ortho = from.ortho;
    s.dev.light_grids = table;
    s.dev.all_lights_gridded = from.all_lights ? 1u : 0u;
}

// A grid the host built, copied to the scene's device.
GridSlot upload_grid(pt_scene& s, const pth_origin_grid& g) {
    GridSlot out;
    if (!g.enabled) return out;
    const uint64_t before = s.info.device_bytes;
    const uint32_t* cell_off = s.upload(g.cell_off, g.n_cells + 1);
    const uint2* refs = (const uint2*)s.upload(g.refs, std::max<uint64_t>(1, g.n_refs));
    out.bytes = s.info.device_bytes - before;
    s.info.device_bytes = before;   // (the slot has them: grid_facts)
    out.dev = dev_grid_from(g, cell_off, refs);
    out.hdr = g;
    out.hdr.cell_off = nullptr;
    out.hdr.refs = nullptr;
    return out;
}

// PT_OG_HOST=1: the grids of the prep.  They are optional: a device that cannot hold them renders through the KD-tree (the
// light grids go first, then the camera grid) instead of failing the scene.
SceneGrids upload_host_grids(const pt_prep& P, pt_scene& s) {
    SceneGrids G;
    G.lights.assign(P.lights.size(), GridSlot{});
    if (P.cam_grid) {
        try {
            AllocMark mark(s);
            G.cam = upload_grid(s, P.cam_grid->g);
            mark.release();
        } catch (const GpuError&) {
            (void)hipGetLastError();
        }
    }
    bool all = P.all_lights_gridded;
    try {
        AllocMark mark(s);
        for (size_t i = 0; i < P.light_grids.size(); ++i) G.lights[i] = upload_grid(s, P.light_grids[i]->g);
        mark.release();
    } catch (const GpuError&) {
        (void)hipGetLastError();
        all = false;
    }
    G.lights_done(all);
    return G;
}

// Copy a prepared scene to `device`.  `early`: its grids, where pt_scene_create has had them built already.
void scene_upload(const pt_prep& P, int device, pt_scene& s, SceneGrids* early = nullptr) {
    select_device(device);
    int cur = 0;
    HIP_CHECK(hipGetDevice(&cur));
    s.device = cur;
    auto t_up = std::chrono::steady_clock::now();
    s.info = P.info;
    s.info.device_bytes = 0;
    DevScene& D = s.dev;
    D = P.dev;
    D.kd_nodes = (const uint2*)s.upload(P.nodes.data(), P.nodes.size());
    D.leaf_prims = s.upload(P.leaf.data(), P.leaf.size());
    D.prim_attr = s.upload(P.attr.data(), P.attr.size());
    D.prim_pos = s.upload(P.pos.data(), P.pos.size());
    D.entry_lists = s.upload(P.entry_lists.data(), P.entry_lists.size());
    D.prim_entry = s.upload(P.prim_entry.data(), P.prim_entry.size());
    s.host_prim_entry = P.prim_entry;   // (test hook pt_trace_rays_wavefront)
    s.cam_src = P.src;
    s.cam_res = P.src->cam_res;
    D.materials = s.upload(P.model_mat.data(), P.model_mat.size());
    D.textures = s.upload(P.textures.data(), P.textures.size());
    D.texels = s.upload(P.texels.data(), P.texels.size());
    D.srgb_lut = s.upload(P.lut, 256);
    D.lights = s.upload(P.lights.data(), P.lights.size());
    s.host_lights = P.lights;
    // ---- escape masks (pt_escape.h): built on the device from these arrays - not here: when the scene is about to render its
    // THIRD frame (escape_masks_build below).  They take 0.14 s for the 0.5 M primitives of config 3 and 1.3 s for the 4 M of
    // config 5 and return 3 ms and ~0.1 s per frame: a one-shot render (the CLI) is better off without them.
    D.escape = nullptr;
    s.info.escape_build_seconds = 0.f;
    s.info.escape_prims = 0;
    s.info.escape_clear_fraction = 0.f;
    {
        const char* esc_env = getenv("PT_ESCAPE");   // (read per scene: the tests switch it)
        const bool esc_on = !(esc_env && *esc_env && atoi(esc_env) == 0);
        const uint64_t n_prims = P.pos.size() / 3;
        s.escape_wanted = esc_on && n_prims > 0 && n_prims < (1ull << 28);
        const char* after = getenv("PT_ESCAPE_AFTER");   // frames a scene renders without them (0: built for the first frame)
        s.escape_after = after && *after ? (uint32_t)atoi(after) : 2u;
    }
    // (built on this device - a prep is shared by the devices of a multi-GPU host, each builds its own - or uploaded)
    SceneGrids G = early ? std::move(*early) : P.src->device_grids ? grids_on_device(P, s) : upload_host_grids(P, s);
    G.lights.resize(P.lights.size());
    s.grids.headers = G.headers;
    s.info.grid_build_seconds += G.seconds;
    install_camera_grid(s, G.cam);
    install_light_grids(s, G, light_grid_table(s, G.lights));
    s.info.upload_seconds = std::chrono::duration<float>(std::chrono::steady_clock::now() - t_up).count();
}

// ---- live edits of a scene: pt_scene_set_camera, pt_scene_set_lights, pt_scene_set_materials (include/ptgpu.h has the
// contract, DESIGN.md 4c / 4d the state they touch row by row).  Everything that can fail comes first - new grids and tables
// are built beside the old ones - and the scene is changed only afterwards.

// The footprints on the scene's device for the grid builds of an edit, uploaded on first use, with room for the extent
// reductions: the extent source of an edit's grids (light_grid, camera_grid).
struct EditFootprints : Footprints {
    const CamGridSource& src;
    unsigned long long* ext = nullptr;   // 12 words
    bool tried = false, ok = false;
    explicit EditFootprints(const CamGridSource& source) : src(source) {}
    ~EditFootprints() {
        if (ext) (void)hipFree(ext);
    }
    // false: no memory for them (the grids that need them are not to be had, as on a fresh scene in that situation)
    bool ready() {
        if (tried) return ok;
        tried = true;
        if (hipMalloc((void**)&geom, src.og_geom.size() * 4) != hipSuccess || hipMalloc((void**)&words, src.og_words.size() * 4) != hipSuccess ||
            hipMalloc((void**)&ext, 12 * 8) != hipSuccess) {
            (void)hipGetLastError();
            return false;
        }
        HIP_CHECK(hipMemcpy(geom, src.og_geom.data(), src.og_geom.size() * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(words, src.og_words.data(), src.og_words.size() * 4, hipMemcpyHostToDevice));
        ok = true;
        return true;
    }
    static uint32_t blocks(uint32_t n_prims) { return std::min<uint32_t>((n_prims + 255u) / 256u, 4096u); }

    pt_prep::GridJob point(const float o[3], uint32_t res, float ray_offset, float max_dir_len) {
        pt_prep::GridJob job;
        const bool finite = std::isfinite(o[0]) && std::isfinite(o[1]) && std::isfinite(o[2]);
        if (ready()) job.valid = pth::og_params_point_ext(o, res, ray_offset, max_dir_len, finite ? point_extent(o) : 0.0, job.params, job.hdr);
        return job;
    }
    pt_prep::GridJob ortho(const float sd[3], uint32_t res) {
        pt_prep::GridJob job;
        pth::og::GridParams axes;
        if (ready() && pth::og_ortho_axes(sd, axes)) job.valid = pth::og_params_ortho_ext(sd, res, ortho_extent(axes), job.params, job.hdr);
        return job;
    }

    // og_point_extent about `o`: the device's reduction over the footprints (k_og_extent), the unowned triangles on the host
    double point_extent(const float o[3]) {
        const uint32_t n_prims = (uint32_t)src.og_words.size();
        HIP_CHECK(hipMemset(ext, 0, 8));
        hipLaunchKernelGGL(ogb::k_og_extent, dim3(blocks(n_prims)), dim3(256), 0, 0, (const float*)geom, (const uint32_t*)words, n_prims,
                           (double)o[0], (double)o[1], (double)o[2], ext);
        HIP_CHECK(hipGetLastError());
        unsigned long long bits = 0;
        HIP_CHECK(hipMemcpy(&bits, ext, 8, hipMemcpyDeviceToHost));
        double e;
        memcpy(&e, &bits, 8);
        for (size_t i = 0; i < src.unowned.size(); ++i) {   // (triangles no model owns: rare, on the host)
            const double v = std::fabs((double)src.unowned[i] - o[i % 3]);
            if (std::isfinite(v)) e = std::max(e, v);
        }
        return e;
    }

    // params_ortho's extent along the axes of P (k_og_ortho_extent), the unowned triangles on the host
    pth::og::OrthoExtent ortho_extent(const pth::og::GridParams& P) {
        const uint32_t n_prims = (uint32_t)src.og_words.size();
        HIP_CHECK(hipMemset(ext, 0, 12 * 8));
        hipLaunchKernelGGL(ogb::k_og_ortho_extent, dim3(blocks(n_prims)), dim3(256), 0, 0, (const float*)geom, (const uint32_t*)words, n_prims,
                           P.axis_u, P.axis_v, P.axis_w, ext);
        HIP_CHECK(hipGetLastError());
        unsigned long long key[12];
        HIP_CHECK(hipMemcpy(key, ext, sizeof key, hipMemcpyDeviceToHost));
        double m[12];
        for (int i = 0; i < 12; ++i) {   // (og_order_key inverted; 0: no value)
            const unsigned long long b = key[i] == 0 ? 0xfff0000000000000ull : (key[i] >> 63) ? key[i] & 0x7fffffffffffffffull : ~key[i];
            memcpy(&m[i], &b, 8);
        }
        pth::og::OrthoExtent e;
        for (int k = 0; k < 3; ++k) {
            e.lo[k] = -m[k];
            e.hi[k] = m[3 + k];
            e.bmin[k] = -m[6 + k];
            e.bmax[k] = m[9 + k];
        }
        for (size_t i = 0; i + 2 < src.unowned.size(); i += 3)
            pth::og::ortho_extent_grow(e, P.axis_u, P.axis_v, P.axis_w, pth::og::Vec{src.unowned[i], src.unowned[i + 1], src.unowned[i + 2]}, 0.0);
        return e;
    }
};

// The camera grid pt_scene_create would build for camera transform M at resolution cam_res (0: none): camera_grid's rule
// with the extent reduced on the device, the device build of grids_on_device.  An empty slot: no grid, also when the device
// has no memory for it.  A device failure of another kind throws.
GridSlot camera_grid_build(pt_scene& s, EditFootprints& F, const float* M, uint32_t cam_res, double& used) {
    const CamGridSource& src = *s.cam_src;
    GridSlot slot;
    if (src.device_grids && cam_res && !src.og_words.empty()) device_grid_build(s, camera_grid(M, cam_res, F), F, src, used, slot);
    return slot;
}

// What earlier frames left (pt_scene::FrameState).
void drop_frame_state(pt_scene& s) { s.frame_state = pt_scene::FrameState{}; }

void scene_set_camera(pt_scene& s, const pt_camera& cam) {
    HIP_CHECK(hipSetDevice(s.device));
    HIP_CHECK(hipDeviceSynchronize());   // the frames in flight finish with the old camera (and its grid)
    const float* M = cam.transform;

    // ---- the camera grid a fresh scene would have.  PT_OG_HOST=1 (host-built grids): the moved camera goes without.
    AllocMark mark(s);
    GridSlot grid;
    {
        EditFootprints F(*s.cam_src);
        double used = 0;
        grid = camera_grid_build(s, F, M, s.cam_res, used);
        // device_grid_build gives up on any failure; what is not a lack of memory is sticky and shows here
        HIP_CHECK(hipDeviceSynchronize());
    }

    // ---- from here on nothing fails: the scene takes the new camera
    mark.release();
    install_camera_grid(s, grid);
    DevScene& D = s.dev;
    dev_camera(cam, D);
    // ---- escape masks: built with a delta_in at least the new camera's, they stay a proof; otherwise they go, and the
    // PT_ESCAPE_AFTER schedule starts again (a scene whose attempt found no memory tries again too)
    if (D.escape && escape_delta_in(D) > s.escape_delta) {
        s.release(D.escape);
        s.info.device_bytes -= (uint64_t)D.n_prims * 80u;
        D.escape = nullptr;
        ++s.escape_generation;
        s.escape_tried = false;
        s.frames_rendered = 0;
        s.info.escape_build_seconds = 0.f;
        s.info.escape_prims = 0;
        s.info.escape_clear_fraction = 0.f;
    } else if (!D.escape && s.escape_tried) {
        s.escape_tried = false;
        s.frames_rendered = 0;
    }
    drop_frame_state(s);
    // the camera-hit cache was this camera's: the next view starts at an empty prefix (the allocation stays)
    ++s.camera_generation;
    s.hit_cache.mark = 0;
    s.hit1_cache.mark = 0;
    s.cont_cache.mark = 0;
    s.hit2_cache.mark = 0;
    for (pt_scene::FrameCache& fc : s.tail_hits) fc.mark = 0;
}

// pt_scene_set_lights.  The light grids are those grids_on_device builds for the new lights (all or none), their parameters
// from extents reduced on the device; the camera grid is rebuilt only if the new light count changes its resolution.  The
// escape masks stay: they depend on the geometry and the camera only (pt_escape.h).
void scene_set_lights(pt_scene& s, const pt_light* lights, uint32_t n) {
    pth::check_lights(lights, n);
    HIP_CHECK(hipSetDevice(s.device));
    HIP_CHECK(hipDeviceSynchronize());   // the frames in flight finish with the old lights (and their grids)
    const CamGridSource& src = *s.cam_src;
    const uint32_t n_prims = (uint32_t)src.og_words.size();
    const GridRule rule = grid_rule(n_prims, n, src.budget, src.grids_on);
    std::vector<DevLight> dl(n);
    for (uint32_t i = 0; i < n; ++i) dl[i] = dev_light(lights[i]);

    AllocMark mark(s);
    EditFootprints F(src);
    SceneGrids G;   // the grids of the new lights, and the camera's if they change it
    // ---- the camera grid, if a fresh scene with n lights has another resolution for it
    const bool new_cam = src.device_grids && rule.cam_res != s.cam_res;
    double used = (double)s.grids.cam.bytes;   // (grids_on_device: the light grids come after the camera's in the budget)
    if (new_cam) {
        const DevScene& D = s.dev;
        float M[16] = {};
        memcpy(M, D.cam_c0, 12);
        memcpy(M + 4, D.cam_c1, 12);
        memcpy(M + 8, D.cam_c2, 12);
        memcpy(M + 12, D.cam_c3, 12);
        used = 0;
        G.cam = camera_grid_build(s, F, M, rule.cam_res, used);
    }
    // ---- the light grids; PT_OG_HOST=1: none
    light_grids_build(s, G, n, rule.lights && (n == 0 || src.device_grids),
                      [&](size_t i) { return light_grid(lights[i].kind, lights[i].vec, rule.light_res, F); }, F, src, used);
    HIP_CHECK(hipDeviceSynchronize());   // (device_grid_build gives up on any failure: what is not a lack of memory shows here)
    const DevLight* d_lights = s.upload(dl.data(), dl.size());
    const DevGrid* d_grids = light_grid_table(s, G.lights);

    // ---- from here on nothing fails: the scene takes the new lights
    mark.release();
    s.release(s.dev.lights);
    s.info.device_bytes -= std::max<uint64_t>(16, (uint64_t)s.dev.n_lights * sizeof(DevLight));
    install_light_grids(s, G, d_grids);
    if (new_cam) install_camera_grid(s, G.cam);
    s.cam_res = rule.cam_res;
    s.dev.lights = d_lights;
    s.dev.n_lights = n;
    s.host_lights = dl;
    drop_frame_state(s);
}

// The colour-only form of scene_set_lights, for pt_lightmix_capture: dl is the scene's light table with other colours - the
// same count, kinds and vectors.  Grids, camera-grid resolution and the visibility planes depend on those alone (grid_rule,
// light_grid; the planes' key is made of kind and vector, frame_caches), so only the DevLight table is replaced; everything
// else is scene_set_lights' state change: the device is synchronised first and no frame plan carries over.
void scene_set_light_colors(pt_scene& s, const std::vector<DevLight>& dl) {
    HIP_CHECK(hipSetDevice(s.device));
    HIP_CHECK(hipDeviceSynchronize());
    AllocMark mark(s);
    const DevLight* d_lights = s.upload(dl.data(), dl.size());
    mark.release();
    s.release(s.dev.lights);
    s.info.device_bytes -= std::max<uint64_t>(16, (uint64_t)s.dev.n_lights * sizeof(DevLight));
    s.dev.lights = d_lights;
    s.host_lights = dl;
    drop_frame_state(s);
}

// pt_scene_set_materials: the model -> material indices of the description resolve the new table into the per-model copies
// the device reads, in a new buffer; has_translucent selects the ALPHA kernel variants.  Nothing else depends on materials.
void scene_set_materials(pt_scene& s, const pt_material* materials, uint32_t n) {
    const CamGridSource& src = *s.cam_src;
    if (n != src.n_materials) fail(PT_ERR_INVALID, "pt_scene_set_materials: %u materials, the scene has %u", n, src.n_materials);
    pth::check_materials(materials, n, src.textures.data(), (uint32_t)src.textures.size(), src.n_texel_bytes);
    HIP_CHECK(hipSetDevice(s.device));
    HIP_CHECK(hipDeviceSynchronize());   // the frames in flight finish with the old materials
    const size_t n_models = src.model_material.size();
    std::vector<pt_material> mm(n_models);
    bool translucent = false;
    for (size_t m = 0; m < n_models; ++m) {   // (as prep_create)
        mm[m] = materials[src.model_material[m]];
        if (mm[m].opacity != 1.0f || mm[m].tex_opacity >= 0) translucent = true;
    }
    AllocMark mark(s);
    const pt_material* d_mat = s.upload(mm.data(), mm.size());
    mark.release();
    s.release(s.dev.materials);
    s.info.device_bytes -= std::max<uint64_t>(16, n_models * sizeof(pt_material));
    s.dev.materials = d_mat;
    s.dev.has_translucent = translucent ? 1u : 0u;
    s.info.has_translucent = translucent;
    ++s.material_generation;
    drop_frame_state(s);
}

hipEvent_t get_event(pt_scene& s, size_t i) {
    while (s.events.size() <= i) {
        hipEvent_t e;
        HIP_CHECK(hipEventCreate(&e));
        s.events.push_back(e);
    }
    return s.events[i];
}

// ------------------------------------------------------------------ render options
// The render path's environment knobs (runtime knobs).  One parser per type: unset or empty gives the default.
double env_num(const char* e, double def) { return e && *e ? atof(e) : def; }
int env_int(const char* e, int def) { return e && *e ? atoi(e) : def; }
bool env_bool(const char* e, bool def) { return e && *e ? atoi(e) != 0 : def; }

// Read once per process (render_env).
struct RenderEnv {
    // PT_TILE_ORDER=morton: the wavefront integrator visits the local tiles along a Z curve over the tile grid instead of row by row
    bool morton;
    uint64_t staging_bytes;   // PT_STAGING_GIB: staging budget (radiance 12 B + RNG block 64 B per work item [+ queues]); 32 GiB of 288 GB
    // PT_WF_CHUNK: the most work items one pass over the bounces may take, whatever the budgets of the frame plan allow
    // (every extra chunk repeats the ~13 persistent launches and their drain phases: 60.9 ms against 63.0 ms for two chunks
    // of 128 Mi - round 2)
    uint32_t wf_chunk;
    bool overlap;   // PT_WF_OVERLAP: shadow(b) on a side stream beside trace(b+1); 0 serialises
    // PT_WF_REFILL: idle lanes that trigger a refill of a persistent wavefront.  Round 3, after the split shade pass and the
    // slack change (config 3, trace stage): 2 / 4 / 6 / 8 / 12 / 16 / 24 / 32 -> 13.36 / 13.31 / 13.32 / 13.31 / 13.41 /
    // 13.57 / 13.98 / 14.63 ms (16 was round 1's optimum)
    uint32_t refill;
    // PT_WF_WALK: node steps per walking phase; 0 = default: 20 for the coherent camera rays (bounce 0 on the KD-tree), 16
    // for the incoherent rays of the later bounces (render_chunk)
    uint32_t walk;
    // PT_WF_SPLIT: the shade pass of bounces >= 1 runs beside k_wf_trace_wide (trace_stage).  Measured (MI355X, config 3;
    // profiles/r03_experiments.txt item 6): frame 34.26 -> 34.14 ms, one shard of eight 5.85 -> 5.69 ms - the two kernels
    // slow each other down (beside the 4 workgroups per CU of k_wf_trace_wide a SIMD has registers for one shade wavefront
    // instead of four), so only part of the shorter one is hidden.
    bool split;
    // PT_WF_EXACT (clamped to 0..2): k_wf_trace / k_wf_shadow hand the rays their walker's slack does not cover to
    // k_wf_trace_exact / k_og_shadow_offgrid (csrc/pt_integrator.h, slop model).  0 is for A/B measurements of what that
    // costs only: the capped walk.  1: k_wf_trace lists them when it fetches them, k_wf_trace_exact runs behind it (beside
    // the shade pass over the queue); 2: k_wf_shade lists them when it makes the rays, k_wf_trace_exact runs beside k_wf_trace.
    uint32_t exact;
    uint32_t exact_blocks;   // PT_WF_EXACT_BLOCKS: workgroups per 8 CUs of k_wf_trace_exact beside k_wf_trace (PT_WF_EXACT=2)
    uint32_t defer;          // PT_WF_DEFER: k_wf_trace: age (loop iterations) at which a cast leaves a drained wavefront
    // PT_WF_SORT: coherence sorting of the survivors by direction octant: measured (MI355X, config 3) trace of bounce 1
    // 9.50 -> 9.25 ms, but the bounce-0 kernel 19.0 -> 20.2 ms: off by default
    uint32_t sort;
    // PT_WF_ENTRY=1: casts of bounces >= 1 start at the home node of the primitive their ray leaves (trav_enter).
    // Measured (profiles/r03_experiments.txt item 2): 31 % fewer node visits, the same time - off by default
    uint32_t entry;
    uint32_t refill_shadow, walk_shadow;   // PT_WF_REFILL_SHADOW, PT_WF_WALK_SHADOW: k_wf_shadow's (0: k_wf_trace's)
    bool side_priority;   // PT_WF_SIDE_PRIORITY=0: the streams of k_wf_trace_wide and k_wf_trace_exact at default priority
    // PT_SHADE_BLOCKS_B0, PT_SHADE_BLOCKS: k_wf_shade's workgroups per CU in the grid.  The kernel's loops are grid-stride,
    // but a grid of just the resident workgroups (3 per CU) keeps the whole chip on ONE window of the image at a time -
    // everybody in the ChaCha-bound background together, then everybody waiting for casts into the model together.  Many
    // more workgroups than are resident, each with a short loop, mix the two (and balance the end): bounce-0 kernel of
    // config 3, 3 / 16 / 64 / 256 / 1024 / 4096 workgroups per CU: 20.9 / 17.3 / 16.1 / 15.5 / 15.4 / 16.4 ms; the later
    // bounces (queues of unknown, shrinking length: every extra workgroup is a dispatch that may find nothing) are best at 32
    // (16 / 32 / 64 / 128: frame 37.6 / 36.2 / 36.2 / 36.2 ms, one shard of eight 5.97 / 5.92 / 6.03 / 6.13 ms).
    uint32_t shade_blocks_b0, shade_blocks;
    bool fuse_rng;   // PT_OG_FUSE_RNG: the fused bounce-0 kernel computes the ChaCha block itself (GRID 3)
    // PT_OG_INLINE_ALL: shadow casts inside the shade kernel at every bounce (bounces >= 1 otherwise keep the shade kernel
    // lean and cast their shadow rays in k_og_shadow: measured faster)
    bool inline_all;
    // PT_OG_INLINE_AUTO: ... and at the bounces where the frame plan found (nearly) every ray reaching a lit surface
    // (PT_OG_INLINE_ALL=1 in the closed room: +6.6 %; in an open scene: -6 %)
    bool inline_auto;
    uint32_t ogs_blocks;   // PT_OGS_BLOCKS: workgroups per CU of k_og_shadow's grid-stride launch
    bool plan_skip;        // PT_PLAN_SKIP=0: the bounces behind a chunk's last ray are launched too
    bool cam_cull;         // PT_CAM_CULL=0: no camera-grid cull (camera_cull)
    bool plan_debug;       // PT_PLAN_DEBUG: the frame plan on stderr when it is made
    bool debug_times, debug_hist, debug_stamps;   // PT_DEBUG_TIMES, PT_DEBUG_HIST, PT_DEBUG_STAMPS: set (even empty) = on
};

const RenderEnv& render_env() {
    static const RenderEnv env = [] {
        RenderEnv r;
        const char* order = getenv("PT_TILE_ORDER");
        r.morton = order && !strcmp(order, "morton");
        r.staging_bytes = (uint64_t)(env_num(getenv("PT_STAGING_GIB"), 32.0) * 1024.0 * 1024.0 * 1024.0);
        r.wf_chunk = (uint32_t)env_num(getenv("PT_WF_CHUNK"), 320.0 * 1024 * 1024);
        r.overlap = env_bool(getenv("PT_WF_OVERLAP"), true);
        r.refill = (uint32_t)env_int(getenv("PT_WF_REFILL"), 8);
        r.walk = (uint32_t)env_int(getenv("PT_WF_WALK"), 0);
        r.split = env_bool(getenv("PT_WF_SPLIT"), true);
        r.exact = (uint32_t)std::min(2, std::max(0, env_int(getenv("PT_WF_EXACT"), 1)));
        r.exact_blocks = (uint32_t)env_int(getenv("PT_WF_EXACT_BLOCKS"), 4);
        r.defer = (uint32_t)env_int(getenv("PT_WF_DEFER"), 16);
        r.sort = (uint32_t)env_int(getenv("PT_WF_SORT"), 0);
        r.entry = env_bool(getenv("PT_WF_ENTRY"), false) ? 1u : 0u;
        r.refill_shadow = (uint32_t)env_int(getenv("PT_WF_REFILL_SHADOW"), 0);
        r.walk_shadow = (uint32_t)env_int(getenv("PT_WF_WALK_SHADOW"), 12);
        r.side_priority = env_bool(getenv("PT_WF_SIDE_PRIORITY"), true);
        r.shade_blocks_b0 = (uint32_t)env_int(getenv("PT_SHADE_BLOCKS_B0"), 256);
        r.shade_blocks = (uint32_t)env_int(getenv("PT_SHADE_BLOCKS"), 32);
        r.fuse_rng = env_bool(getenv("PT_OG_FUSE_RNG"), true);
        r.inline_all = env_int(getenv("PT_OG_INLINE_ALL"), 0) != 0;
        r.inline_auto = env_bool(getenv("PT_OG_INLINE_AUTO"), true);
        r.ogs_blocks = (uint32_t)env_int(getenv("PT_OGS_BLOCKS"), 16);
        r.plan_skip = env_bool(getenv("PT_PLAN_SKIP"), true);
        r.cam_cull = env_bool(getenv("PT_CAM_CULL"), true);
        r.plan_debug = env_bool(getenv("PT_PLAN_DEBUG"), false);
        r.debug_times = getenv("PT_DEBUG_TIMES") != nullptr;
        r.debug_hist = getenv("PT_DEBUG_HIST") != nullptr;
        r.debug_stamps = getenv("PT_DEBUG_STAMPS") != nullptr;
        return r;
    }();
    return env;
}

// The frame plan's budgets, read per call: tests/test_frame_plan.py and tools/stress_paths.py change them between frames
// of one scene.  First frame 8 GiB: what the CLI pays for in allocation time (path-tracer render of the 500 k-triangle
// scene, 1080p x 128 spp, render_s with 2 / 4 / 8 / 16 / 64 GiB: 0.121 / 0.095 / 0.080 / 0.136-0.29 / 1.69 s - the frame
// itself is 0.04-0.05 s).  Later frames: what their records need, up to 32 GiB - config 3 takes 14.1 GiB (one pass), the
// closed room 31.4 GiB in 2 passes (170.2 ms in 5 passes of 12.7 GiB, 165.8 in 2, 164.5 in one of 51.7 GiB), the KD-tree
// pipeline of config 3 29.7 GiB.
struct QueueEnv {
    double first_gib;      // PT_QUEUE_GIB
    double steady_gib;     // PT_QUEUE_STEADY_GIB (default: the larger of PT_QUEUE_GIB and 32)
    // PT_QUEUE_ONE_PASS_GIB: a batch that fits it as ONE chunk takes it (every extra pass repeats the persistent launches
    // and their drains - the KD-tree pipeline of config 3, 29.7 GiB in one pass: 62.4 ms, in three passes of 16 GiB 75.3 ms)
    double one_pass_gib;
    // PT_QUEUE_RESERVE_GIB: what the queues must leave free (the runtime allocates the kernels' scratch - up to 592 B per
    // lane of every wave slot of the device, per hardware queue: ~1.2 GB - when they are first launched, and dies if it cannot)
    double reserve_gib;
    double test_shrink;    // PT_PLAN_TEST_SHRINK, clamped to 0.01..1 (0: unset)
    bool test_lean;        // PT_B0_LEAN_TEST_FORCE: the lean bounce-0 variant without asking whether the frame is eligible
    bool test_lean1;       // PT_B1_LEAN_TEST_FORCE: the lean shade pass at bounces 1 and 2 wherever the plain fused pass would run
};

// The lean shade pass of bounces 1 and 2 is taken where the counted frame sent fewer than 1 / PT_B1_LEAN_SHARE of the bounce's
// shaded records to the shadow queue: a handed-over record costs both passes
// (a named constant, not a measurement: break-even lies near the lean launch's relative gain, 10-20 % - 1/64 is safely inside)
constexpr uint64_t PT_B1_LEAN_SHARE = 64;
QueueEnv queue_env() {
    QueueEnv q;
    q.first_gib = env_num(getenv("PT_QUEUE_GIB"), 8.0);
    q.steady_gib = env_num(getenv("PT_QUEUE_STEADY_GIB"), std::max(q.first_gib, 32.0));
    q.one_pass_gib = env_num(getenv("PT_QUEUE_ONE_PASS_GIB"), 32.0);
    q.reserve_gib = env_num(getenv("PT_QUEUE_RESERVE_GIB"), 2.0);
    const char* shrink = getenv("PT_PLAN_TEST_SHRINK");
    q.test_shrink = shrink && *shrink ? std::min(1.0, std::max(0.01, atof(shrink))) : 0.0;
    q.test_lean = env_bool(getenv("PT_B0_LEAN_TEST_FORCE"), false);
    q.test_lean1 = env_bool(getenv("PT_B1_LEAN_TEST_FORCE"), false);
    return q;
}

// ------------------------------------------------------------------ one frame (render_device and its stages)
// Runtime switches to template arguments: fn(std::integral_constant<bool, b>...) for the values b of `on`, in order.
template <class F>
void dispatch(F&& fn) {
    fn();
}
template <class F, class... B>
void dispatch(F&& fn, bool on, B... rest) {
    if (on) dispatch([&](auto... t) { fn(std::true_type{}, t...); }, rest...);
    else dispatch([&](auto... t) { fn(std::false_type{}, t...); }, rest...);
}

// What frame_setup derives from the profile, the options and the scene.
struct Frame {
    const RenderEnv& env = render_env();
    pt_profile p{};
    pt_opts o{};
    TileMap tm;
    DevScene dev{};   // the scene as this frame's kernels see it
    const uint32_t* d_tiles = nullptr;
    float* accum = nullptr;
    RenderParams P{};
    bool timing = false, counting = false, exit_times = false;
    DevCounters* gctr = nullptr;   // (counting or exit_times)
    bool wavefront = true;         // the integrator: wavefront (default), or the one-lane-per-pixel megakernel
    bool use_cam_grid = false, use_light_grids = false, alpha = false;
    // bounce 0 as ONE kernel (k_wf_shade<GRID >= 2>: camera cast through the camera grid, shadow casts through the light grids).
    // The camera-grid cull belongs to that kernel: its mask is computed, its wavefronts skip empty blocks and k_accumulate
    // adds the background for their pixels under this one condition (round-3 advisory: three places derived it separately).
    bool bounce0_fused = false;
    uint32_t blocks64 = 0;   // 8x8 pixel blocks of the local tiles
    uint32_t batch = 0;      // samples per pass over the image
    // a tile-list frame (pt_render_tiles): the tile map is the caller's list, the outputs are packed in list order; it leaves the
    // scene's steady state - plans, frame caches, the count of frames before the escape masks - as it found it
    bool tile_list = false;
    // a window frame (pt_render_window): the samples [win_s0, win_s1) of the frame's enumeration, the sums carried
    // in from the caller's buffers where win_s0 > 0; like a tile-list frame it keeps out of the scene's steady state
    bool window = false;
    uint32_t win_s0 = 0, win_s1 = 0;
    bool detached() const { return tile_list || window; }   // a first frame every time: no plan, no frame cache
    uint32_t first_sample() const { return window ? win_s0 : 0u; }
    uint32_t end_sample() const { return window ? win_s1 : p.samples; }
};

// The tiles of a tile-list frame: global tile numbers, strictly ascending.
struct TileList {
    const uint32_t* tiles;
    uint32_t n;
};

// The samples [s0, s1) of a window frame, 0 <= s0 < s1 <= profile.samples.
struct SampleWindow {
    uint32_t s0, s1;
};

// The words of a frame's tile table: the packed offset of every local tile, their global tile numbers (tile_k_base), then -
// morton - the order in which the wavefront integrator visits the local tiles
std::vector<uint32_t> tile_table_words(const TileMap& tm, bool morton) {
    std::vector<uint32_t> table(tm.offsets);
    table.insert(table.end(), tm.tiles.begin(), tm.tiles.end());
    if (morton) {
        auto spread = [](uint32_t v) {   // bits of v to the even positions
            uint64_t x = v;
            x = (x | (x << 16)) & 0x0000ffff0000ffffull;
            x = (x | (x << 8)) & 0x00ff00ff00ff00ffull;
            x = (x | (x << 4)) & 0x0f0f0f0f0f0f0f0full;
            x = (x | (x << 2)) & 0x3333333333333333ull;
            x = (x | (x << 1)) & 0x5555555555555555ull;
            return x;
        };
        std::vector<std::pair<uint64_t, uint32_t>> order(tm.n_local_tiles);
        for (uint32_t lt = 0; lt < tm.n_local_tiles; ++lt) {
            const uint32_t k = tm.tiles[lt];
            order[lt] = {spread(k % tm.tiles_x) | (spread(k / tm.tiles_x) << 1), lt};
        }
        std::sort(order.begin(), order.end());
        for (auto& e : order) table.push_back(e.second);
    }
    return table;
}

// The tile table of a sharded or Morton-ordered frame (cached per configuration: no host sync in steady state): the packed
// offset of every local tile, their global tile numbers (tile_k_base), then - PT_TILE_ORDER=morton - the order in which
// the wavefront integrator visits the local tiles
const uint32_t* tile_table(pt_scene& s, const pt_profile& p, const pt_opts& o, const TileMap& tm, bool morton) {
    auto key = std::make_tuple(p.width, p.height, o.shard_rank, o.shard_count, o.tile_w, o.tile_h);
    auto found = s.tile_tables.find(key);
    if (found == s.tile_tables.end()) {
        if (s.tile_tables.size() >= 256) {   // (a caller cycling through hundreds of configurations: start over, idle)
            HIP_CHECK(hipDeviceSynchronize());
            s.tile_tables.clear();
        }
        const std::vector<uint32_t> table = tile_table_words(tm, morton);
        auto buf = std::make_unique<DeviceBuffer>();
        buf->ensure(table.size() * 4);
        HIP_CHECK(hipMemcpy(buf->p, table.data(), table.size() * 4, hipMemcpyHostToDevice));   // (a fresh buffer: nobody reads it yet)
        found = s.tile_tables.emplace(key, std::move(buf)).first;
    }
    return (const uint32_t*)found->second->p;
}

// Validation, the tile map, the escape masks, the counters, RenderParams, the pipeline, the sample batch and its staging
// area.  false: this rank has no pixels.  list: a tile-list frame's tiles (everything such a frame refuses is refused before
// any device work; then it waits for the device - its table and its statistics slot are rewritten in place).
bool frame_setup(pt_scene& s, const pt_profile& p, const pt_opts* opts_in, void* d_accum, hipStream_t stream, Frame& f,
                 const TileList* list = nullptr, const SampleWindow* win = nullptr) {
    pt_opts& o = f.o;
    normalise_opts(p, opts_in, o);
    if (p.samples == 0) fail(PT_ERR_INVALID, "profile.samples must be > 0");
    if (p.brdf != PT_BRDF_COOK_TORRANCE) fail(PT_ERR_INVALID, "unknown brdf %d", p.brdf);
    if (p.tonemap < 0 || p.tonemap > 2) fail(PT_ERR_INVALID, "unknown tonemap %d", p.tonemap);
    f.tile_list = list != nullptr;
    if (win) {
        if (win->s0 >= win->s1 || win->s1 > p.samples)
            fail(PT_ERR_INVALID, "pt_render_window: the window [%u, %u) of a frame of %u samples", win->s0, win->s1, p.samples);
        if (!d_accum) fail(PT_ERR_INVALID, "pt_render_window: a window needs the accum buffer (its sums are carried there)");
        f.window = true;
        f.win_s0 = win->s0;
        f.win_s1 = win->s1;
    }
    if (list) {
        if (p.bounces > 4096u) fail(PT_ERR_INVALID, "profile.bounces %u is out of range (at most 4096)", p.bounces);
        f.tm = make_tile_list_map("pt_render_tiles", p, o, list->tiles, list->n);
    }
    HIP_CHECK(hipSetDevice(s.device));
    f.p = p;
    if (!list) f.tm = make_tile_map(p, o, o.shard_rank);
    const TileMap& tm = f.tm;
    if (tm.n_local == 0) return false;
    // escape masks: from the scene's (escape_after + 1)th frame of the default pipeline on (scene_upload has the reason)
    if (!f.detached() && s.escape_wanted && !s.escape_tried && !(o.flags & (PT_FLAG_NO_GRIDS | PT_FLAG_MEGAKERNEL))) {
        if (s.frames_rendered >= s.escape_after) escape_masks_build(s);
        ++s.frames_rendered;
    }
    // the KD-tree pipeline (PT_FLAG_NO_GRIDS) - the cross-check of the parity tests - knows no escape masks either
    f.dev = s.dev;
    if (o.flags & PT_FLAG_NO_GRIDS) f.dev.escape = nullptr;
    uint32_t tile_order_base = 0, tile_k_base = 0;
    // (the tile-list frame before this one may still read the table; the detached frame before this one may still write the
    // statistics slot these frames share)
    if (f.detached()) HIP_CHECK(hipDeviceSynchronize());
    if (list) {
        const std::vector<uint32_t> table = tile_table_words(tm, f.env.morton);
        s.tile_list_table.ensure(table.size() * 4);
        HIP_CHECK(hipMemcpy(s.tile_list_table.p, table.data(), table.size() * 4, hipMemcpyHostToDevice));
        f.d_tiles = (const uint32_t*)s.tile_list_table.p;
    } else if (o.shard_count > 1 || f.env.morton) {
        f.d_tiles = tile_table(s, p, o, tm, f.env.morton);
    }
    if (f.d_tiles) {
        tile_k_base = (uint32_t)tm.offsets.size();
        if (f.env.morton) tile_order_base = (uint32_t)(tm.offsets.size() + tm.tiles.size());
    }
    f.accum = (float*)d_accum;
    if (!f.accum) {
        s.accum_scratch.ensure(tm.n_local * 12);
        f.accum = (float*)s.accum_scratch.p;
    }
    f.timing = o.flags & PT_FLAG_TIMING;
    f.counting = o.flags & PT_FLAG_COUNTERS;
#ifdef WF_EXIT_TIMES
    f.exit_times = true;    // diagnostic build: the stamps are taken by the plain (non-counting) kernels too
#endif
    if (f.counting || f.exit_times) {
        s.counter_buf.ensure(sizeof(DevCounters));
        HIP_CHECK(hipMemsetAsync(s.counter_buf.p, 0, sizeof(DevCounters), stream));
#ifdef WF_EXIT_TIMES
        HIP_CHECK(hipMemsetAsync(&((DevCounters*)s.counter_buf.p)->launch_start, 0xff, sizeof(((DevCounters*)nullptr)->launch_start), stream));
#endif
        f.gctr = (DevCounters*)s.counter_buf.p;
    }

    RenderParams& P = f.P;
    P.width = p.width;
    P.height = p.height;
    P.samples = p.samples;
    P.bounces = p.bounces;
    P.tonemap = p.tonemap;
    P.shard_rank = o.shard_rank;
    P.shard_count = list ? 2u : o.shard_count;   // (what the kernels read of it: > 1 - the outputs are packed by the tile table)
    P.tile_w = o.tile_w;
    P.tile_h = o.tile_h;
    P.tiles_x = tm.tiles_x;
    P.tiles_y = tm.tiles_y;
    P.n_local = (uint32_t)tm.n_local;
    P.tile_order_base = tile_order_base;
    P.tile_k_base = tile_k_base;
    pt_fastdiv_make((o.tile_w >> 3) * (o.tile_h >> 3), P.div_tile_blocks);
    pt_fastdiv_make(o.tile_w >> 3, P.div_tile_cols);
    pt_fastdiv_make(tm.tiles_x, P.div_tiles_x);

    f.wavefront = !(o.flags & PT_FLAG_MEGAKERNEL);
    // the 16-bit draw index / bounce fields of the queue records, the per-bounce counter table
    if (p.bounces > 4096u) fail(PT_ERR_INVALID, "profile.bounces %u is out of range (at most 4096)", p.bounces);
    f.use_cam_grid = !(o.flags & PT_FLAG_NO_GRIDS) && s.dev.cam_grid.res != 0;
    f.use_light_grids = !(o.flags & PT_FLAG_NO_GRIDS) && s.dev.all_lights_gridded != 0;
    f.bounce0_fused = f.use_cam_grid && f.use_light_grids;
    f.blocks64 = tm.n_local_tiles * (o.tile_w / 8u) * (o.tile_h / 8u);
    if (s.n_cu == 0) HIP_CHECK(hipDeviceGetAttribute(&s.n_cu, hipDeviceAttributeMultiprocessorCount, s.device));
    f.batch = o.sample_batch ? o.sample_batch : p.samples;
    if (f.window) f.batch = std::min(f.batch, f.win_s1 - f.win_s0);
    f.alpha = s.dev.has_translucent != 0;
    if (f.wavefront) {
        uint64_t per_sample = tm.n_local * 12u;
        uint64_t max_batch = std::max<uint64_t>(1, f.env.staging_bytes / std::max<uint64_t>(1, per_sample));
        max_batch = std::min<uint64_t>(max_batch, 0x7fffffffull / ((uint64_t)f.blocks64 * 64u));
        if (max_batch == 0) fail(PT_ERR_UNSUPPORTED, "image too large for one sample batch");
        f.batch = (uint32_t)std::min<uint64_t>(f.batch, max_batch);
        s.staging_buf.ensure((size_t)f.batch * tm.n_local * 12);
    }
    return true;
}

// The wavefront integrator's chunking and queues for one frame.
struct WfFrame {
    pt_scene::FrameStats* fs = nullptr;   // the statistics (and plan) of this frame's configuration
    uint64_t items_per_batch = 0;         // work items of a whole sample batch
    uint32_t max_items = 0;               // the most work items of one chunk (PT_WF_CHUNK)
    size_t lights = 1;
    bool rng_one_plane = false;   // the fused bounce-0 kernel keeps words 0-3 of the items' ChaCha blocks in registers
    uint64_t per_item = 0;        // bytes per work item when nothing is known (every queue as long as the chunk)
    uint32_t cap_a = 0;           // the chunk of the first frame: what fits the first-frame budget
    uint32_t cap = 0;             // work items per chunk
    // capacities (records) of what is indexed by a queue position: the two path queues, the hit records (+ the alpha walk's
    // draw counts), the shadow records (+ contrib planes, off-grid list), the exact lists
    uint32_t cap_q[2] = {0, 0}, cap_h = 0, cap_s = 0, cap_e = 0;
    std::vector<uint8_t> inline_at;   // bounces >= 1 whose shadow casts run inside the shade kernel
    bool planned = false;             // the capacities are the plan's (false: a first frame's)
    bool multi_chunk = false;
    uint32_t stats_slots = 0;   // lines of this frame's statistics (0: none taken)
    // per chunk of the plan: the last bounce that has a ray (later ones are not launched); nullptr: every bounce
    const std::vector<uint32_t>* plan_last = nullptr;
    const uint32_t* block_empty = nullptr;     // the camera-grid cull table (nullptr: no cull in this frame)
    // the scene's frame caches this frame uses (frame_caches; nullptr: not in use): the words, keyed to this frame's
    // enumeration, the camera hits, keyed to its view, the shadow visibility, keyed to its view and lights
    pt_scene::FrameCache *rng_cache = nullptr, *hit_cache = nullptr, *vis_cache = nullptr;
    // the hits of the bounces that have a cache of them (hit1_cache, hit2_cache), keyed to the frame's view and material
    // table: by bounce (entry 0 stays empty - the camera hits are the bounce-0 kernel's).  Bounces 3-5: pt_scene::tail_hits.
    struct BounceHits {
        pt_scene::FrameCache* cache = nullptr;
        uint32_t holes = 0;                      // PT_HIT1_CACHE_HOLES / PT_HIT2_CACHE_HOLES / PT_TAIL_HIT_CACHE_HOLES (study switches, read per frame)
        unsigned long long* unknown = nullptr;   // the casts the loading launches left to k_wf_trace_exact (on the device)
    };
    static constexpr uint32_t HIT_BOUNCES = pt_scene::HIT_BOUNCES;
    BounceHits bounce_hits[HIT_BOUNCES];
    // the shadow visibility of the bounces that have a cache of it, by bounce (entry 1: pt_scene::vis1_cache; 2-4: pt_scene::tail_vis),
    // and whether that bounce's shade pass adds the lights of known visibility itself (PT_VIS1_FUSED; 2-4: PT_TAIL_VIS_FUSED)
    pt_scene::FrameCache* bounce_vis[HIT_BOUNCES] = {};
    bool vis_fused[HIT_BOUNCES] = {};
    // the device counters of the fused shade launches of bounce b: behind the next bounce's counter of unknown casts
    unsigned long long* fused_ctr(uint32_t b) const { return b + 1u < HIT_BOUNCES ? bounce_hits[b + 1u].unknown : nullptr; }
    // PT_HIT1_FUSED (read per frame; 0: off): the bounce-0 kernel of a chunk that loads camera hits, visibility and bounce-1
    // hits reads the bounce-1 plane itself (k_wf_shade_hits<.. | SB_NEXT>) - no k_wf_hits_load at bounce 1
    bool hit1_fused = true;
    // the bounce-0 continuations (pt_scene::cont_cache), keyed like the bounce-1 hits; nullptr: not in use
    pt_scene::FrameCache* cont_cache = nullptr;
    // PT_CONT_ESCAPE (read per frame): the loading launches use the escape test's recorded answer where the scene's masks are
    // those the records were stored under
    bool cont_escape = false;
    // PT_B0_LEAN (read per frame): the loading bounce-0 launches of this frame take the lean variant (lean_frame);
    // lean_forced: the test hook PT_B0_LEAN_TEST_FORCE - they take it whatever the counts said
    bool lean = false, lean_forced = false;
    // PT_B1_LEAN (read per frame): the plain fused shade pass of bounce b (1 or 2) takes the lean variant with its list pass
    // (lean_frame); b1_lean_forced: the test hook PT_B1_LEAN_TEST_FORCE - it does whatever the counts said
    bool b1_lean[3] = {false, false, false}, b1_lean_forced = false;
    // PT_VIS1_FUSED (default 1), PT_HIT2_FUSED (default 0; both read per frame): the bounce-1 shade pass of a chunk whose batch has visibility bytes
    // adds the lights of known visibility itself (k_wf_shade_fused<SB_VIS1>); ... and, where the chunk loads its bounce-2 hits, reads
    // that plane itself too (<SB_VIS1 | SB_NEXT1>, the first switch on as well) - no k_wf_hits_load at bounce 2.  hits_next_wanted: this
    // frame may take the second, so queue_buffers provides WfPipe::hits_next
    bool hit2_fused = false, hits_next_wanted = false;   // (PT_VIS1_FUSED: vis_fused[1])
    uint32_t stats_line = 0, chunk_slot = 0;   // the frame's progress through its chunks
};

// Counts per (batch, chunk of fs.cap_items items) -> the plan: m consecutive chunks become one, every buffer as long as the
// largest group's counts need; the largest m whose buffers fit the steady budget
bool make_plan(pt_scene::FrameStats& fs, const Frame& f, const WfFrame& wf, const QueueEnv& qe) {
    const uint32_t ca = fs.cap_items, lv = fs.levels;
    const uint64_t items_per_batch = wf.items_per_batch;
    std::vector<std::vector<uint32_t>> batches;   // slots of each batch, in order
    for (uint32_t k = 0; k < fs.n_slots; ++k) {
        if (fs.first_item_of_slot[k] == 0u) batches.emplace_back();
        if (batches.empty()) return false;
        batches.back().push_back(k);
    }
    if (batches.empty() || ca == 0) return false;
    uint32_t m_max = 1;
    for (auto& bt : batches) m_max = std::max<uint32_t>(m_max, (uint32_t)bt.size());
    // (PT_WF_CHUNK caps a chunk; a batch that may be one chunk needs no multiple of ca)
    m_max = std::min<uint32_t>(m_max, (uint64_t)wf.max_items >= items_per_batch ? (uint32_t)((items_per_batch + ca - 1u) / ca) : std::max(1u, wf.max_items / ca));
    // by the number of passes over a batch: m = the fewest first-frame chunks per pass that make that many passes, so the
    // passes come out even (nine chunks in three passes: 3 + 3 + 3, not 4 + 4 + 1 at a third more memory)
    uint32_t s_max = 1;
    for (auto& bt : batches) s_max = std::max<uint32_t>(s_max, (uint32_t)bt.size());
    uint32_t m_prev = 0;
    for (uint32_t n_pass = 1; n_pass <= s_max; ++n_pass) {
        const uint32_t m = (s_max + n_pass - 1u) / n_pass;
        if (m > m_max || m == m_prev) continue;
        m_prev = m;
        uint64_t q1 = 0, q0 = 0, hh = 0, ss = 0, ee = 0;
        std::vector<uint64_t> tot_q(lv, 0), tot_s(lv, 0);
        std::vector<uint32_t> last;
        for (auto& bt : batches)
            for (size_t g0 = 0; g0 < bt.size(); g0 += m) {
                last.push_back(0u);
                for (uint32_t b = 0; b < lv; ++b) {
                    uint64_t nq = 0, ns = 0, ne = 0;
                    for (size_t k = g0; k < std::min(bt.size(), g0 + m); ++k) {
                        const uint32_t* row = fs.host + ((size_t)bt[k] * lv + b) * 4;
                        nq += row[0];
                        ns += row[1];
                        ne += row[2];
                    }
                    tot_q[b] += nq;
                    tot_s[b] += ns;
                    if (b >= 1 && nq != 0) last.back() = b;
                    if (b >= 1) {   // (queue b lives in queue[b & 1]; the hits of its casts by queue position)
                        uint64_t& q = (b & 1u) ? q1 : q0;
                        q = std::max(q, nq);
                        hh = std::max(hh, nq);
                    }
                    ss = std::max(ss, ns);
                    ee = std::max(ee, ne);
                }
            }
        const uint64_t items = std::min<uint64_t>((uint64_t)ca * m, items_per_batch);
        if (!f.bounce0_fused) hh = std::max(hh, items);   // the casts of bounce 0 too: hits and draw counts by work item
        auto pad = [](uint64_t n) { return (std::max<uint64_t>(n, 1024) + 1023) & ~1023ull; };
        q0 = pad(q0), q1 = pad(q1), hh = pad(hh), ss = pad(ss), ee = pad(ee);
        const uint64_t bytes = 68u * (q0 + q1) + 20u * hh + (f.alpha ? 4u * hh : 0u) + (64u + 16u * wf.lights + 4u) * ss + 16u * ee +
                               (wf.rng_one_plane ? 16u : (f.env.overlap && items < items_per_batch) ? 64u : 32u) * items;   // (two copies: the next chunk's are made ahead)
        const bool fits = bytes <= (uint64_t)(qe.steady_gib * 1073741824.0) ||
                          (items >= items_per_batch && bytes <= (uint64_t)(qe.one_pass_gib * 1073741824.0));
        if ((fits || m == 1) && std::max({q0, q1, hh, ss, ee, items}) < 0xffffffffull) {
            fs.plan_cap = (uint32_t)items;
            fs.plan_q[0] = (uint32_t)q0;
            fs.plan_q[1] = (uint32_t)q1;
            fs.plan_h = (uint32_t)hh;
            fs.plan_s = (uint32_t)ss;
            fs.plan_e = (uint32_t)ee;
            // shadow casts inside the shade kernel where (nearly) every ray of a bounce reaches a lit surface
            fs.plan_inline.assign(f.p.bounces + 2, 0);
            if (f.env.inline_auto && f.use_light_grids)
                for (uint32_t b = 1; b < lv && b < fs.plan_inline.size(); ++b) fs.plan_inline[b] = tot_q[b] > 0 && tot_s[b] * 10 >= tot_q[b] * 6;
            fs.plan_last = last;
            fs.plan_fresh = true;
            if (f.env.plan_debug) {
                fprintf(stderr, "[ptgpu] frame plan: %u chunks of %u -> 1 of %llu items; queues %llu / %llu, hits %llu, shadow %llu, exact %llu records; %.3f GiB\n",
                        m, ca, (unsigned long long)items, (unsigned long long)q0, (unsigned long long)q1, (unsigned long long)hh,
                        (unsigned long long)ss, (unsigned long long)ee, bytes / 1073741824.0);
                for (uint32_t b = 0; b < lv; ++b)
                    fprintf(stderr, "[ptgpu]   bounce %u: %llu rays, %llu shadow records%s\n", b, (unsigned long long)tot_q[b],
                            (unsigned long long)tot_s[b], b < fs.plan_inline.size() && fs.plan_inline[b] ? " (inline)" : "");
            }
            return true;
        }
    }
    return false;
}

// The frame plan.  A frame is a pure function of (scene, profile, options) - the seeds are the pixels' - so the counts of
// a configuration's first frame are those of every later one: the first frame runs in chunks small enough for a fixed
// budget with every queue as long as the chunk, the later ones get queues as long as the records that exist.  Collects
// the counts of an earlier frame if they have arrived and returns this frame's chunking and capacities.
WfFrame frame_plan(pt_scene& s, const Frame& f, const QueueEnv& qe) {
    const pt_profile& p = f.p;
    const pt_opts& o = f.o;
    WfFrame wf;
    wf.items_per_batch = (uint64_t)f.blocks64 * 64u * f.batch;
    if (s.trace_blocks == 0) {
        int a = 0, b = 0, c = 0, d = 0;
        HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&a, k_wf_trace<false, false, false>, WF_THREADS, 0));
        HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&b, k_wf_trace<true, false, false>, WF_THREADS, 0));
        HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&c, k_wf_shadow<false, false>, WF_THREADS, 0));
        HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&d, k_wf_shadow<true, false>, WF_THREADS, 0));
        s.trace_blocks = std::max(1, f.alpha ? b : a) * s.n_cu;
        s.shadow_blocks = std::max(1, f.alpha ? d : c) * s.n_cu;
    }
    s.pipe.ctr.ensure(sizeof(WfCounters) * (p.bounces + 3));
    wf.lights = std::max(1u, s.dev.n_lights);
    wf.rng_one_plane = f.env.fuse_rng && f.bounce0_fused;
    // two path queues of 64 B (+ the entry word), 20 B hit, 64 B shadow record + 16 B per light, the RNG plane(s), draws,
    // off-grid and exact lists
    wf.per_item = 68u * 2u + 20u + 64u + 16u * wf.lights + (wf.rng_one_plane ? 16u : 32u) + (f.alpha ? 4u : 0u) + 4u + 16u;
    wf.max_items = (uint32_t)std::min<uint64_t>(wf.items_per_batch, std::max<uint32_t>(64u, f.env.wf_chunk & ~63u));
    const std::vector<uint64_t> stat_key = {p.width, p.height, p.samples, p.bounces, (uint64_t)p.brdf,
                                            o.flags & (PT_FLAG_NO_GRIDS | PT_FLAG_MEGAKERNEL | PT_FLAG_COUNTERS), (uint64_t)f.bounce0_fused, o.shard_rank, o.shard_count, o.tile_w, o.tile_h, f.batch, (uint64_t)wf.max_items};
    wf.cap_a = (uint32_t)std::min<uint64_t>(wf.max_items, std::max<uint64_t>(1u << 20, (uint64_t)(qe.first_gib * 1073741824.0) / wf.per_item) & ~63ull);
    if (s.wf_cap_ok) wf.cap_a = std::min(wf.cap_a, s.wf_cap_ok);
    if (f.detached()) {
        // a first frame, every time: no plan is read or made, and no key another frame can meet is touched.  (frame_setup
        // waited for the device: the counts of the tile-list frame before are home, nothing refers to the slot's event.)
        if (!s.tile_frame_stats) s.tile_frame_stats = std::make_unique<pt_scene::FrameStats>();
        pt_scene::FrameStats& own = *s.tile_frame_stats;
        own.pending = own.valid = own.planned = own.stats_planned = own.plan_fresh = own.plan_failed = false;
        own.stats_hit_loads = own.plan_hit_loads = 0;
        own.lean = own.stats_lean_ok = false;
        own.b1_lean[0] = own.b1_lean[1] = own.stats_b1_ok = false;
        wf.fs = &own;
        wf.inline_at.assign(p.bounces + 2, 0);
        wf.cap = wf.cap_a;
        wf.cap_q[0] = wf.cap_q[1] = wf.cap_h = wf.cap_s = wf.cap_e = wf.cap;
        return wf;
    }
    auto& stats = s.frame_state.stats;
    if (!stats[stat_key]) {
        if (stats.size() > 64) {   // (a caller cycling through configurations: start over)
            HIP_CHECK(hipDeviceSynchronize());
            stats.clear();
        }
        stats[stat_key] = std::make_unique<pt_scene::FrameStats>();
    }
    pt_scene::FrameStats* fs = wf.fs = stats[stat_key].get();
    if (fs->pending) {
        const hipError_t q = hipEventQuery(fs->done);
        (void)hipGetLastError();   // (hipErrorNotReady is no error)
        if (q == hipSuccess) {
            fs->pending = false;
            bool overflow = false, guard = false;
            // (the lean variant: a clean frame is one none of whose lines saw a cold lane or a bounce-0 shadow record)
            bool clean = fs->planned && fs->stats_planned && fs->stats_lean_ok;
            for (uint32_t k = 0; k < fs->n_slots; ++k) {
                overflow = overflow || fs->host[(size_t)k * fs->levels * 4 + 3] != 0u;
                guard = guard || (fs->host[(size_t)k * fs->levels * 4 + 3] & 2u) != 0u;   // (bit 1: a lean launch met a cold lane)
                clean = clean && fs->cold_words()[k] == 0u && fs->host[(size_t)k * fs->levels * 4 + 1] == 0u;
                if (fs->planned && fs->stats_planned && k < fs->plan_last.size())   // (a ray at a bounce the plan did not launch)
                    for (uint32_t b = fs->plan_last[k] + 1u; b < fs->levels; ++b)
                        overflow = overflow || fs->host[((size_t)k * fs->levels + b) * 4] != 0u;
            }
            fs->lean = clean && !overflow;
            fs->lean_sig = fs->stats_sig;
            // (the lean shade pass of bounces 1 and 2: a handed-over record costs both passes, so the share of records the
            // counted frame sent to the shadow queue must lie well inside the lean launch's relative gain)
            for (uint32_t b = 1; b <= 2u; ++b) {
                uint64_t shadow = 0, shaded = 0;
                for (uint32_t k = 0; k < fs->n_slots && b < fs->levels; ++k) {
                    shadow += fs->shadow_words()[2u * k + (b - 1u)];
                    shaded += fs->host[((size_t)k * fs->levels + b) * 4 + 1];
                }
                fs->b1_lean[b - 1u] = fs->planned && fs->stats_planned && fs->stats_b1_ok && !overflow && shadow * PT_B1_LEAN_SHARE < shaded;
                fs->b1_sig[b - 1u] = fs->stats_b1_sig[b - 1u];
            }
            if (guard) {
                // cannot happen (a configuration goes lean on counts that say no lane needs more): nothing was written for the lane
                ++s.b0_lean_guard_trips;
                fs->valid = fs->planned = false;
                fail(PT_ERR_DEVICE, "internal error: a lean bounce-0 launch met a lane that needs the general variant; the previous "
                                    "frame of this configuration is not to be trusted");
            }
            if (overflow) {
                // cannot happen (the counts of a configuration do not change): a queue sized from them ran full
                fs->valid = fs->planned = false;
                fail(PT_ERR_DEVICE, "internal error: a path queue sized from an earlier frame's counts ran full; the previous frame of "
                                    "this configuration is not to be trusted");
            }
            if (!fs->planned) {
                fs->valid = true;
                fs->planned = make_plan(*fs, f, wf, qe);
                fs->plan_hit_loads = fs->stats_hit_loads;
            }
        }
    }
    wf.planned = fs->planned && !fs->plan_failed;
    wf.inline_at.assign(p.bounces + 2, 0);
    if (wf.planned) {
        wf.cap = fs->plan_cap;
        wf.cap_q[0] = fs->plan_q[0], wf.cap_q[1] = fs->plan_q[1], wf.cap_h = fs->plan_h, wf.cap_s = fs->plan_s, wf.cap_e = fs->plan_e;
        wf.inline_at = fs->plan_inline;
        wf.inline_at.resize(p.bounces + 2, 0);
        // test hook (tests/test_frame_plan.py): a plan that is WRONG - every array shorter than its records - so that what
        // cannot happen does: the kernels must drop the records that do not fit without writing past an array, flag the
        // frame, and the next call of the configuration must say so
        if (qe.test_shrink > 0) {
            const double k = qe.test_shrink;
            for (uint32_t* c : {&wf.cap_q[0], &wf.cap_q[1], &wf.cap_s, &wf.cap_e}) *c = std::max<uint32_t>(64u, (uint32_t)(*c * k));
            wf.cap_h = std::max({(uint32_t)(wf.cap_h * k), wf.cap_q[0], wf.cap_q[1]});
        }
    } else {
        wf.cap = wf.cap_a;
        wf.cap_q[0] = wf.cap_q[1] = wf.cap_h = wf.cap_s = wf.cap_e = wf.cap;
    }
    return wf;
}

// The buffers of wf's capacities.  A device that cannot provide them (shared GPU) gets half-size chunks with every queue as
// long as the chunk, and so on, down to 1 Mi items.
void queue_buffers(pt_scene& s, const Frame& f, const QueueEnv& qe, WfFrame& wf) {
    pt_scene::WfPipe& w = s.pipe;
    const bool alpha = f.alpha;
    const size_t lights = wf.lights;
    const bool give_back = wf.planned && wf.fs->plan_fresh;   // (a new plan gives memory back, once)
    bool grew = false;
    auto fit = [give_back, &grew](DeviceBuffer& b, size_t n) {
        if (give_back && b.bytes > n + n / 4 + (64u << 20)) b.release();
        grew = grew || b.bytes < n;
        return b.try_ensure(n);
    };
    while (true) {
        wf.multi_chunk = (uint64_t)wf.cap < wf.items_per_batch;
        const bool two_rng = !wf.rng_one_plane && wf.multi_chunk && f.env.overlap;
        // (a frame whose every item has room in the word cache needs no plane of its own: render_chunk allocates it should a
        // chunk run uncached after all)
        const bool words_cached = wf.rng_cache && wf.rng_cache->stride == wf.rng_cache->items;
        bool ok = fit(w.queue[0], (size_t)wf.cap_q[0] * 68u) && fit(w.queue[1], (size_t)wf.cap_q[1] * 68u) &&   // (64 B + the entry word)
                  fit(w.hits, (size_t)wf.cap_h * 20u) && fit(w.shadow, (size_t)wf.cap_s * 64u) &&
                  fit(w.contrib, (size_t)wf.cap_s * 16u * lights) && (words_cached || fit(w.rng[0], (size_t)wf.cap * (wf.rng_one_plane ? 16u : 32u))) &&
                  (!two_rng || fit(w.rng[1], (size_t)wf.cap * 32u)) &&
                  (!alpha || fit(w.draws, (size_t)wf.cap_h * 4u)) &&   // RNG draw index of the alpha walk
                  fit(w.offgrid, (size_t)wf.cap_s * 4u) &&   // shadow jobs left to k_og_shadow_offgrid (long normals; rays the wavefront walker does not take)
                  fit(w.exact[0], (size_t)wf.cap_e * 8u) && fit(w.exact[1], (size_t)wf.cap_e * 8u) &&   // casts left to k_wf_trace_exact: queue index + hit word
                  (!wf.hits_next_wanted || fit(w.hits_next, (size_t)wf.cap_q[0] * 20u)) &&   // (queue 2 lives in queue[0])
                  (!f.bounce0_fused || w.block_mask.try_ensure((size_t)f.blocks64 * 4u + 4u + f.tm.n_local)) &&
                  // casts left to k_wf_trace_wide: at most one per lane in flight when the queue runs dry
                  // (4 B the queue index + 20 B a hit + 4 B the progress of the walk: wf_list_* in pt_wavefront.h)
                  (!f.env.defer ||
                   w.deferred.try_ensure((size_t)s.trace_blocks * WF_THREADS * 4u * (alpha ? WF_LIST_WORDS_ALPHA : WF_LIST_WORDS_OPAQUE)));
        if (ok && grew && wf.cap > (1u << 20)) {
            size_t free_b = 0, total_b = 0;
            if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && (double)free_b < qe.reserve_gib * 1073741824.0) ok = false;
            grew = false;
        }
        if (ok) {
            if (wf.planned) wf.fs->plan_fresh = false;
            break;
        }
        for (DeviceBuffer* b : {&w.queue[0], &w.queue[1], &w.hits, &w.shadow, &w.contrib, &w.rng[0], &w.rng[1], &w.draws, &w.offgrid, &w.deferred, &w.exact[0], &w.exact[1], &w.block_mask, &w.hits_next, &w.handover})
            b->release();
        if (wf.planned) {   // (no room for the planned sizes: as a first frame)
            wf.planned = false;
            wf.fs->plan_failed = true;
            wf.cap = wf.cap_a;
        } else {
            if (wf.cap <= (1u << 20))
                fail(PT_ERR_DEVICE, "out of device memory: the path queues need %zu bytes for %u work items", (size_t)wf.cap * wf.per_item, wf.cap);
            wf.cap = std::max<uint32_t>(1u << 20, (wf.cap / 2u) & ~63u);
            s.wf_cap_ok = wf.cap;
        }
        wf.cap_q[0] = wf.cap_q[1] = wf.cap_h = wf.cap_s = wf.cap_e = wf.cap;
        std::fill(wf.inline_at.begin(), wf.inline_at.end(), 0);
    }
    if (f.detached()) return;   // (pt_scene_get_info goes on reporting the last whole frame)
    s.queue_bytes_last = w.queue[0].bytes + w.queue[1].bytes + w.hits.bytes + w.shadow.bytes + w.contrib.bytes + w.rng[0].bytes +
                         w.rng[1].bytes + w.draws.bytes + w.offgrid.bytes + w.exact[0].bytes + w.exact[1].bytes + w.deferred.bytes;
    s.queue_chunk_last = wf.cap;
    s.frame_planned_last = wf.planned ? 1u : 0u;
}

// What differs between the scene's frame caches, apart from their keys and the frames they serve (frame_caches).
struct FrameCacheKind {
    const char *env_switch, *env_gib;   // "0": off; the budget in GiB - both read per frame, the tests switch them
    double default_gib;
    uint32_t item_bytes;
    uint64_t max_items;   // an enumeration of this many items or more is never keyed
    // false: the contents are a prefix written in frame order - a new key starts an empty one once the frames in flight have
    // finished with the old (device sync).  true: the plane is zeroed for a new key, by a memset in stream order behind the
    // last launch that touched it - a device sync only where the allocation changes.  counter[0] counts the memsets.
    bool zeroed;
};
constexpr FrameCacheKind RNG_CACHE = {"PT_RNG_CACHE", "PT_RNG_CACHE_GIB", 16.0, 32u, 1ull << 32, false};   // (W.cap carries the stride: 32 bits)
constexpr FrameCacheKind HIT_CACHE = {"PT_HIT_CACHE", "PT_HIT_CACHE_GIB", 8.0, 16u, ~0ull, false};
constexpr FrameCacheKind VIS_CACHE = {"PT_VIS_CACHE", "PT_VIS_CACHE_GIB", 1.0, 1u, ~0ull, true};
// (zeroed AND a prefix: the memset of a new key also starts an empty prefix - frame_cache_frame resets the mark either way -
// and, there being no device sync, every launch that reads the plane records the event too, not only those that write)
constexpr FrameCacheKind HIT1_CACHE = {"PT_HIT1_CACHE", "PT_HIT1_CACHE_GIB", 8.0, 16u, ~0ull, true};
#ifndef PT_B0_LEAN_DEFAULT
#define PT_B0_LEAN_DEFAULT true   // (the lean bounce-0 variant: profiles/r21_experiments.txt)
#endif
#ifndef PT_B1_LEAN_DEFAULT
#define PT_B1_LEAN_DEFAULT true   // (the lean shade pass of bounces 1 and 2: profiles/r22_experiments.txt)
#endif
#ifndef PT_CONT_ESCAPE_DEFAULT
#define PT_CONT_ESCAPE_DEFAULT true   // (with the records refilled when the masks arrive: profiles/r20_experiments.txt item 2)
#endif
constexpr FrameCacheKind CONT_CACHE = {"PT_CONT_CACHE", "PT_CONT_CACHE_GIB", 8.0, 32u, ~0ull, true};   // (two planes of 16 B)
constexpr FrameCacheKind HIT2_CACHE = {"PT_HIT2_CACHE", "PT_HIT2_CACHE_GIB", 8.0, 16u, ~0ull, true};
constexpr FrameCacheKind VIS1_CACHE = {"PT_VIS1_CACHE", "PT_VIS1_CACHE_GIB", 1.0, 1u, ~0ull, true};
// (the planes of bounces 3-5 and 2-4: one switch and one budget PER PLANE for each group)
constexpr FrameCacheKind TAIL_HIT_CACHE = {"PT_TAIL_HIT_CACHE", "PT_TAIL_HIT_CACHE_GIB", 8.0, 16u, ~0ull, true};
constexpr FrameCacheKind TAIL_VIS_CACHE = {"PT_TAIL_VIS_CACHE", "PT_TAIL_VIS_CACHE_GIB", 1.0, 1u, ~0ull, true};

// One frame cache and this frame, of `items` work items and key `key`: the cache if the frame uses it, keyed to `key`.
// Keying happens when a frame of a key directly follows another of the same - also one that was switched off or not
// eligible - and the budget has room for a stride other than the keyed one.  A frame that is not eligible leaves the
// contents alone.
pt_scene::FrameCache* frame_cache_frame(pt_scene::FrameCache& fc, const FrameCacheKind& kind, const std::vector<uint64_t>& key,
                                        uint64_t items, bool eligible, hipStream_t stream) {
    const bool follows_same = key == fc.last_key;
    fc.last_key = key;
    const double gib = env_num(getenv(kind.env_gib), kind.default_gib);
    if (!env_bool(getenv(kind.env_switch), true) || !(gib > 0.0)) {
        if (fc.buf.p) {
            HIP_CHECK(hipDeviceSynchronize());   // (frames in flight may still use the plane)
            fc.buf.release();
        }
        fc.key.clear();
        fc.items = fc.stride = fc.mark = 0;
        return nullptr;
    }
    if (fc.failed || !eligible) return nullptr;
    const uint64_t stride = std::min<uint64_t>(items, (uint64_t)(gib * 1073741824.0) / kind.item_bytes) & ~63ull;
    if (key != fc.key || stride != fc.stride) {
        if (!follows_same || items >= kind.max_items || stride == 0) return nullptr;
        const size_t bytes = (size_t)stride * kind.item_bytes;
        const bool refit = fc.buf.bytes < bytes || fc.buf.bytes > bytes + (64u << 20);
        if (!kind.zeroed || (refit && fc.buf.p)) HIP_CHECK(hipDeviceSynchronize());   // the frames in flight finish with the old contents
        if (refit) fc.buf.release();
        fc.key.clear();
        fc.items = fc.stride = fc.mark = 0;
        if (!fc.buf.try_ensure(bytes)) {
            fc.failed = true;
            return nullptr;
        }
        if (!fc.ev) HIP_CHECK(hipEventCreateWithFlags(&fc.ev, hipEventDisableTiming));
        if (kind.zeroed) {
            fc.wait_on(stream);   // the launches of the old key on another stream are done with the plane before it is zeroed
            HIP_CHECK(hipMemsetAsync(fc.buf.p, 0, bytes, stream));
            fc.touched(stream);
            ++fc.counter[0];
        }
        fc.key = key;
        fc.items = items;
        fc.stride = stride;
    }
    fc.wait_on(stream);   // a frame on another stream than the last launch that touched the plane
    return &fc;
}

// The scene's frame caches and this frame: one key, extended from cache to cache, and the frames each serves.
void frame_caches(pt_scene& s, const Frame& f, WfFrame& wf, hipStream_t stream) {
    const uint64_t items = (uint64_t)f.blocks64 * 64u * f.p.samples;
    // The words: keyed to an enumeration - everything decode_item and the batch order read.  Frames of the KD-tree pipeline
    // and instrumented frames (PT_FLAG_COUNTERS) derive their words as before and leave the cache alone.
    std::vector<uint64_t> key = {f.p.width, f.p.height, f.p.samples, f.o.shard_rank, f.o.shard_count, f.o.tile_w, f.o.tile_h,
                                 (uint64_t)f.env.morton, f.batch};
    wf.rng_cache = frame_cache_frame(s.rng_cache, RNG_CACHE, key, items, wf.rng_one_plane && !f.counting, stream);
    // The camera hits: the enumeration plus the camera generation and the camera grid's resolution (a new light COUNT may
    // rebuild the grid at another resolution, and with it the cull table that decides which wavefronts store).  The first
    // frame of a view never stores, a camera path never stores and never allocates.  Eligible: opaque, uninstrumented
    // frames of the fused pipeline that read the word cache; any other frame leaves the records alone - those of a scene
    // that turned translucent are still the opaque cast's for that camera.
    key.insert(key.end(), {s.camera_generation, (uint64_t)s.cam_res});
    wf.hit_cache = frame_cache_frame(s.hit_cache, HIT_CACHE, key, items, wf.rng_cache && f.bounce0_fused && !f.alpha && !f.counting, stream);
    // The bounce-1 hits: the camera hits' key plus the material generation - the BRDF at the camera hit makes the ray - and
    // NOT the lights or the bounces.  The first frame after a material edit or a camera move neither loads nor stores, the
    // second zeroes the plane and stores, the third loads; a light orbit loads throughout.  Eligible: the frames the hit
    // cache serves that have a bounce 1; any other frame leaves the records alone.
    // The bounce-2 hits: the same key, the same rules, one bounce later - in use where the bounce-1 hits are and the frame
    // has a bounce 2.  Bounces 3-5 (pt_scene::tail_hits; PT_TAIL_HIT_CACHE, one budget per plane): the same again, each in
    // use where the bounce before it is - a plane switched off, over budget or not to be had takes those behind it out of
    // use.  All planes are keyed, zeroed and stored by the same frame; a frame with more bounces casts bounces >= 6.
    std::vector<uint64_t> key1 = key;
    key1.push_back(s.material_generation);
    // (a counter block: the cache's unknown casts + the counts of the launches that read the plane themselves, pt_scene::hits_unknown)
    auto counter_block = [](DeviceBuffer& b) {
        if (b.p) return;
        b.ensure(128);   // (sixteen uint64: hit1_unknown uses ten)
        HIP_CHECK(hipMemset(b.p, 0, 128));
    };
    {
        bool before = wf.hit_cache != nullptr, holes = false;
        uint32_t loads_all = 0;   // bit b: every item of the frame loads bounce b
        for (uint32_t b = 1; b < WfFrame::HIT_BOUNCES; ++b) {
            const FrameCacheKind& kind = b == 1u ? HIT1_CACHE : b == 2u ? HIT2_CACHE : TAIL_HIT_CACHE;
            const char* env_holes = b == 1u ? "PT_HIT1_CACHE_HOLES" : b == 2u ? "PT_HIT2_CACHE_HOLES" : "PT_TAIL_HIT_CACHE_HOLES";
            WfFrame::BounceHits& bh = wf.bounce_hits[b];
            bh.cache = frame_cache_frame(s.hits_cache(b), kind, key1, items, before && f.p.bounces >= b, stream);
            if (bh.cache) counter_block(s.hits_unknown(b));
            bh.unknown = (unsigned long long*)s.hits_unknown(b).p;
            bh.holes = bh.cache ? (uint32_t)env_num(getenv(env_holes), 0.0) : 0u;
            holes = holes || bh.holes != 0u;
            if (bh.cache && bh.cache->mark >= items) loads_all |= 1u << b;
            before = bh.cache != nullptr;
        }
        // The exact list as long as the queue it indexes where the plan's count of it does not cover this frame: the study
        // switches make every N-th cast of the queue unknown; a plan counted in a frame that loaded a bounce (the shade pass
        // before it listed nothing for that bounce then) does not know the rays a frame that casts it lists - a cache switched
        // off or over budget since.
        if (holes || (wf.planned && (wf.fs->plan_hit_loads & ~loads_all) != 0u)) wf.cap_e = std::max({wf.cap_e, wf.cap_q[0], wf.cap_q[1]});
        wf.hit1_fused = env_bool(getenv("PT_HIT1_FUSED"), true);
    }
    // The bounce-0 continuations: the bounce-1 hits' key, in use in the frames that cache serves - stored by the frame that
    // stores those hits, loaded by the launches that read them in the bounce-0 kernel.  Light edits leave it alone.
    wf.cont_cache = frame_cache_frame(s.cont_cache, CONT_CACHE, key1, items, wf.bounce_hits[1].cache != nullptr, stream);
    wf.cont_escape = env_bool(getenv("PT_CONT_ESCAPE"), PT_CONT_ESCAPE_DEFAULT);
    // The shadow visibility: the hits' key plus the light count and every light's kind and position, bit for bit - not its
    // colour or `tame`, not the materials, not the bounces.  The first frame after a moved light or camera does nothing
    // new, a light orbit or a camera path never zeroes and never allocates; from the keying frame's memset on, every chunk
    // that LOADs its hits and lies below the plane's stride runs the variant that reads the plane and fills in what is
    // unknown.  Eligible: the frames the hit cache serves, with one to four lights; any other frame leaves the bits alone -
    // those of a scene that turned translucent are still the opaque geometry's.
    const size_t light_words = key.size();
    key.push_back(s.host_lights.size());
    for (const DevLight& L : s.host_lights) {
        uint32_t w[4];
        memcpy(w, &L.kind, 4);
        memcpy(w + 1, L.vec, 12);
        key.push_back((uint64_t)w[0] << 32 | w[1]);
        key.push_back((uint64_t)w[2] << 32 | w[3]);
    }
    const bool few_lights = !s.host_lights.empty() && s.host_lights.size() <= 4u;
    wf.vis_cache = frame_cache_frame(s.vis_cache, VIS_CACHE, key, items, wf.hit_cache && few_lights, stream);
    // The bounce-1 shadow visibility: the bounce-1 hits' key plus the same light words.  The first frame after a moved
    // light, a material edit or a camera move does nothing new; from the keying frame's memset on, every chunk whose sample
    // batch lies below the plane's stride and whose bounce-1 shadow records go through k_og_shadow runs the variant that
    // reads the plane and fills in what is unknown (render_chunk).  Eligible: the frames the bounce-1 hit cache serves, with
    // one to four lights, every light with a grid.
    // The shadow visibility of bounces 2-4 (pt_scene::tail_vis; PT_TAIL_VIS_CACHE, one budget per plane): the same key, each
    // plane eligible where that bounce's hit cache is in use.
    // The shade pass of such a bounce that reads these bytes itself (render_chunk; bounce 1: and the bounce-2 records): its
    // counters live behind the next bounce's counter of unknown casts, whether or not that cache is in use
    key1.insert(key1.end(), key.begin() + light_words, key.end());
    const bool tail_fused = env_bool(getenv("PT_TAIL_VIS_FUSED"), true);
    for (uint32_t b = 1; b + 1u < WfFrame::HIT_BOUNCES; ++b) {
        wf.bounce_vis[b] = frame_cache_frame(s.vis_cache_of(b), b == 1u ? VIS1_CACHE : TAIL_VIS_CACHE, key1, items,
                                             wf.bounce_hits[b].cache && few_lights && f.use_light_grids, stream);
        wf.vis_fused[b] = b == 1u ? env_bool(getenv("PT_VIS1_FUSED"), true) : tail_fused;
        if (wf.bounce_vis[b]) counter_block(s.hits_unknown(b + 1u));
        wf.bounce_hits[b + 1u].unknown = (unsigned long long*)s.hits_unknown(b + 1u).p;
    }
    wf.hit2_fused = env_bool(getenv("PT_HIT2_FUSED"), false);   // (measured 0.08 ms slower than the first step alone: off)
    wf.hits_next_wanted = wf.vis_fused[1] && wf.hit2_fused && wf.bounce_vis[1] && wf.bounce_hits[2].cache && !s.grids.ortho;
}

// This frame's counts, one line per (batch, chunk): taken every frame (a few KB) - the first frame's feed the plan, the
// later ones only say whether a queue ran full.  None while an earlier frame's line is still on its way.
void stats_slots(pt_scene& s, const Frame& f, WfFrame& wf) {
    pt_scene::FrameStats* fs = wf.fs;
    const uint32_t levels = f.p.bounces + 3;
    uint32_t n = 0;
    for (uint32_t s0 = f.first_sample(); s0 < f.end_sample(); s0 += f.batch) {
        const uint64_t tot = (uint64_t)f.blocks64 * 64u * std::min(f.batch, f.end_sample() - s0);
        n += (uint32_t)((tot + wf.cap - 1u) / wf.cap);
    }
    if (fs->pending) return;
    if (fs->n_slots != n || fs->levels != levels || !fs->host) {
        if (fs->host) (void)hipHostFree(fs->host);
        fs->host = nullptr;
        HIP_CHECK(hipHostMalloc((void**)&fs->host, pt_scene::FrameStats::host_bytes(n, levels)));   // (+ FrameStats::cold_words, shadow_words)
        fs->n_slots = n;
        fs->levels = levels;
    }
    if (!fs->done) HIP_CHECK(hipEventCreateWithFlags(&fs->done, hipEventDisableTiming));
    fs->cap_items = wf.cap;
    fs->stats_planned = wf.planned;
    fs->stats_hit_loads = 0;
    fs->first_item_of_slot.assign(n, 0u);
    s.stats_dev.ensure(pt_scene::FrameStats::host_bytes(n, levels));
    wf.stats_slots = n;
}

// The lean bounce-0 variant in this frame.  What a configuration's clean count was taken under: the keys and marks of the
// caches the loading bounce-0 launch reads - words, camera hits, visibility, bounce-1 hits, continuations - and the masks'
// generation.  Any scene edit drops the configuration's counts altogether (drop_frame_state), a re-key, a moved mark or new
// masks change the signature: the frames behind it take the general variant until one of them has been counted clean again.
// An unplanned, a counting or a detached frame takes the general variant and ends the configuration's eligibility.
void lean_frame(pt_scene& s, const Frame& f, const QueueEnv& qe, WfFrame& wf) {
    pt_scene::FrameStats* fs = wf.fs;
    if (!fs) return;
    std::vector<uint64_t> sig = {s.escape_generation};
    for (const pt_scene::FrameCache* fc : {wf.rng_cache, wf.hit_cache, wf.vis_cache, wf.bounce_hits[1].cache, wf.cont_cache}) {
        sig.push_back(fc ? 1u + fc->key.size() : 0u);
        if (!fc) continue;
        sig.insert(sig.end(), fc->key.begin(), fc->key.end());
        sig.push_back(fc->mark);
        sig.push_back(fc->stride);
    }
    const bool plain = wf.planned && !f.counting && !f.detached();
    if (!plain) fs->lean = false;
    wf.lean = env_bool(getenv("PT_B0_LEAN"), PT_B0_LEAN_DEFAULT) && plain && fs->lean && fs->lean_sig == sig;
    wf.lean_forced = qe.test_lean;
    // The lean shade pass of bounces 1 and 2 (independent of PT_B0_LEAN): the same signature plus the keys and marks of that
    // bounce's visibility and hit planes.  Eligibility is a matter of speed only - what the lean launch cannot shade it hands
    // to the list pass behind it - so the test hook may force it on any frame.
    const bool b1_on = env_bool(getenv("PT_B1_LEAN"), PT_B1_LEAN_DEFAULT);
    if (!plain) fs->b1_lean[0] = fs->b1_lean[1] = false;
    wf.b1_lean_forced = b1_on && qe.test_lean1;
    for (uint32_t b = 1; b <= 2u; ++b) {
        std::vector<uint64_t> sig_b = sig;
        for (const pt_scene::FrameCache* fc : {(const pt_scene::FrameCache*)wf.bounce_vis[b], (const pt_scene::FrameCache*)wf.bounce_hits[b].cache}) {
            sig_b.push_back(fc ? 1u + fc->key.size() : 0u);
            if (!fc) continue;
            sig_b.insert(sig_b.end(), fc->key.begin(), fc->key.end());
            sig_b.push_back(fc->mark);
            sig_b.push_back(fc->stride);
        }
        wf.b1_lean[b] = b1_on && plain && fs->b1_lean[b - 1u] && fs->b1_sig[b - 1u] == sig_b;
        if (wf.stats_slots) fs->stats_b1_sig[b - 1u] = std::move(sig_b);
    }
    if (wf.b1_lean[1] || wf.b1_lean[2] || wf.b1_lean_forced) {   // (no room for the list: the general pass)
        if (!s.pipe.handover.try_ensure(((size_t)std::max(wf.cap_q[0], wf.cap_q[1]) + WF_HANDOVER_HEAD) * 4u))
            wf.b1_lean[1] = wf.b1_lean[2] = wf.b1_lean_forced = false;
    }
    if (wf.stats_slots) {
        fs->stats_lean_ok = plain;
        fs->stats_b1_ok = plain;
        fs->stats_sig = std::move(sig);
    }
}

// The side streams and the events between them, made by the first frame that needs them.
void side_streams(pt_scene& s, const Frame& f, const WfFrame& wf) {
    pt_scene::WfPipe& w = s.pipe;
    // (the next chunk's RNG planes are produced on the SHADOW stream, idle while a chunk's bounce 0 is traced - not on a stream
    // of their own: a FIFTH stream - the caller's, shadow, wide, exact and that one - makes two of them share one of the
    // device's four hardware queues (ROCm's default), and every launch of the frame then waits ~45 us longer for its turn:
    // config 3, 40.3 -> 41.8 ms a frame with the stream merely existing, config 5 465 -> 508 ms)
    if (wf.multi_chunk && f.env.overlap && !wf.rng_one_plane && !w.ev_rng) {
        HIP_CHECK(hipEventCreateWithFlags(&w.ev_rng, hipEventDisableTiming));
        HIP_CHECK(hipEventCreateWithFlags(&w.ev_chunk, hipEventDisableTiming));
    }
    if (f.env.overlap && !w.side) {
        HIP_CHECK(hipStreamCreateWithPriority(&w.side, hipStreamNonBlocking, 0));
        HIP_CHECK(hipEventCreateWithFlags(&w.ev_shade, hipEventDisableTiming));
        HIP_CHECK(hipEventCreateWithFlags(&w.ev_shadow, hipEventDisableTiming));
    }
    if (f.env.overlap && !w.side_wide) {
        // (high priority: their few workgroups - the long casts of the drain, the casts the wavefront walker does not take -
        // run beside the shade pass over the queue, whose thousands of short workgroups would otherwise take every slot
        // that comes free before them; PT_WF_SIDE_PRIORITY=0: default priority)
        int prio_lo = 0, prio_hi = 0;
        HIP_CHECK(hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi));
        const int prio = f.env.side_priority ? prio_hi : prio_lo;
        HIP_CHECK(hipStreamCreateWithPriority(&w.side_wide, hipStreamNonBlocking, prio));
        HIP_CHECK(hipStreamCreateWithPriority(&w.side_exact, hipStreamNonBlocking, prio));
        HIP_CHECK(hipEventCreateWithFlags(&w.ev_trace, hipEventDisableTiming));
        HIP_CHECK(hipEventCreateWithFlags(&w.ev_wide, hipEventDisableTiming));
        HIP_CHECK(hipEventCreateWithFlags(&w.ev_exact, hipEventDisableTiming));
        HIP_CHECK(hipEventCreateWithFlags(&w.ev_exact_go, hipEventDisableTiming));
    }
}

// The timing events of one frame (PT_FLAG_TIMING): (stage id, first event index) of every timed launch - 0 generate
// 1 trace 2 shade 3 shadow 4 accumulate 5 fused - and the first event index of every fused bounce-0 launch (k_wf_shade<GRID >= 2>).
struct Timeline {
    pt_scene& s;
    bool on;
    hipStream_t stream;   // where the events of the next stage are recorded
    size_t ev = 0;
    uint32_t launches = 0, stage_launches = 0;
    std::vector<std::pair<int, size_t>> marks;
    std::vector<size_t> fused_marks;
    void begin(int stage) {
        if (!on) return;
        marks.emplace_back(stage, ev);
        HIP_CHECK(hipEventRecord(get_event(s, ev++), stream));
    }
    void end() {
        ++stage_launches;
        if (on) HIP_CHECK(hipEventRecord(get_event(s, ev++), stream));
    }
};

// Bounce 0 through the camera grid: the 8x8 pixel blocks no camera ray can hit anything in (k_cam_block_mask) are found
// once per frame; their wavefronts write the background without a ChaCha block or a cast.  PT_CAM_CULL=0: off.
// Returns the table (nullptr: no cull in this frame).
const uint32_t* camera_cull(pt_scene& s, const Frame& f, hipStream_t stream) {
    const uint32_t* block_empty = nullptr;
    if (f.env.cam_cull && f.wavefront && f.bounce0_fused && !f.counting) {
        RenderParams P1 = f.P;
        P1.sample_begin = 0;
        P1.sample_end = 1;
        pt_fastdiv_make(1u, P1.div_batch);
        HIP_CHECK(hipMemsetAsync((uint32_t*)s.pipe.block_mask.p + f.blocks64, 0, 4, stream));
        hipLaunchKernelGGL(k_cam_block_mask, dim3((f.blocks64 * 64u + 255u) / 256u), dim3(256), 0, stream, f.dev, P1, f.d_tiles, f.blocks64,
                           (uint32_t*)s.pipe.block_mask.p, (uint8_t*)((uint32_t*)s.pipe.block_mask.p + f.blocks64 + 1u));
        HIP_CHECK(hipGetLastError());
        block_empty = (const uint32_t*)s.pipe.block_mask.p;
    }
    s.frame_state.mask_blocks = block_empty ? f.blocks64 : 0u;
    return block_empty;
}

// What the stages of one bounce of a chunk launch with.
struct Chunk {
    WfParams W{};
    hipStream_t st_main = nullptr, st_shadow = nullptr;
    uint4* rng_planes = nullptr;
    WfCounters* wctr = nullptr;
    uint32_t b = 0;      // the bounce
    bool prim = false;   // bounce 0: the camera rays, derived in place from the staged screen positions (no queue[0])
    // origin grids (pt_grid.h): 3 / 2 = camera cast + shadow casts inside the shade kernel (bounce 0, both kinds of grid;
    // 3: the kernel computes the ChaCha block itself), 1 = shadow casts inside the shade kernel, 0 = none
    int grid_mode = 0;
    bool cached = false;   // the chunk's words are in the scene's word cache (rng_planes points there): GRID 3 reads them
    // the scene's camera-hit cache (cached chunks only): SB_STORE - the bounce-0 kernel stores the chunk's camera hits at
    // hit_plane, SB_LOAD - it loads them instead of casting, 0 - neither
    int hit_mode = 0;
    uint4* hit_plane = nullptr;
    uint8_t* vis_plane = nullptr;   // the scene's shadow-visibility cache (chunks that load their hits only): the chunk's bytes, or null
    // the scene's caches of later bounces' hits, by bounce (WfFrame::bounce_hits): SB_STORE - k_wf_hits_store behind the bounce
    // writes the chunk's records at `plane`, SB_LOAD - k_wf_hits_load takes the place of the bounce's casts, 0 - neither
    struct BounceHits {
        int mode = 0;
        uint4* plane = nullptr;
    } bounce_hits[WfFrame::HIT_BOUNCES];
    int hits_mode(uint32_t bounce) const { return bounce < WfFrame::HIT_BOUNCES ? bounce_hits[bounce].mode : 0; }
    // the bounce-0 kernel answers the bounce-1 casts from bounce_hits[1].plane itself (k_wf_shade_hits<.. | SB_NEXT>): bounce 1
    // launches no k_wf_hits_load.  next_ctr: the cache's device counters (pt_scene::hit1_unknown)
    bool hit1_fused = false;
    unsigned long long* next_ctr = nullptr;
    // the scene's cache of bounce-0 continuations: SB_CONT_STORE - the bounce-0 kernel stores the chunk's records at cont_plane
    // (plane 1: cont_stride records behind), SB_CONT_LOAD - it loads them instead of sampling the BRDF, 0 - neither
    int cont_mode = 0;
    uint4* cont_plane = nullptr;
    size_t cont_stride = 0;
    uint32_t cont_flags = 0;   // bit 0: the records' escape answers hold for the scene's masks (the loading variant's flag argument)
    bool lean = false;         // the loading launch is the lean variant (k_wf_shade_hits<.. | SB_LEAN>, code 6379)
    // the scene's shadow-visibility caches of bounces 1-4, by bounce: the bytes of the chunk's sample batch, or null (k_og_shadow_vis)
    uint8_t* bounce_vis_plane[WfFrame::HIT_BOUNCES] = {};
    uint8_t* vis_plane_of(uint32_t bounce) const { return bounce < WfFrame::HIT_BOUNCES ? bounce_vis_plane[bounce] : nullptr; }
    // the bounce-1 shade pass reads bounce_vis_plane[1] itself (k_wf_shade_fused<SB_VIS1>), and bounce_hits[2].plane too (| SB_NEXT1): then bounce 2
    // launches no k_wf_hits_load and finds its hits in WfPipe::hits_next.  0: k_wf_shade.  Set at bounce 1, kept for bounce 2
    int b1_fused = 0;
    // this bounce's shade pass is k_wf_shade_fused (bounce 1: b1_fused; bounces 2-4: SB_VIS1, with that bounce's plane); 0: k_wf_shade
    int fused = 0;
    // this bounce's fused pass (SB_VIS1 alone, bounce 1 or 2) is the lean variant, k_wf_shade_fused<SB_VIS1 | SB_LEAN1> (8448), with
    // the list pass of the general body (<SB_VIS1 | SB_HAND>, 16640) behind it
    bool lean1 = false;
    uint4* hits = nullptr;   // the hit plane of this bounce's queue (WfPipe::hits; hits_next: see above), W.hcap records long
    float4 *q_in = nullptr, *q_out = nullptr;
    bool split_shade = false;   // the shade pass in two launches (PT_WF_SPLIT)
};

// The casts of a bounce: the camera rays through the camera grid (k_og_primary), or k_wf_trace with its hand-overs to
// k_wf_trace_exact and k_wf_trace_wide.
void trace_stage(pt_scene& s, const Frame& f, Chunk& c, Timeline& tl) {
    const pt_scene::WfPipe& pipe = s.pipe;
    WfParams& W = c.W;
    const uint32_t b = c.b;
    tl.begin(1);
    if (c.prim && f.use_cam_grid) {   // camera rays: one grid lookup instead of a KD walk (pt_grid_kernels.h)
        dispatch([&](auto alpha, auto count) {
            hipLaunchKernelGGL((k_og_primary<alpha, count>), dim3((W.n_items + 255u) / 256u), dim3(256), 0, c.st_main, f.dev, W, f.d_tiles,
                               (uint4*)pipe.hits.p, (const uint4*)c.rng_planes, (uint32_t*)pipe.draws.p, f.gctr);
        }, f.alpha, f.counting);
        HIP_CHECK(hipGetLastError());
    } else {
        W.defer_age = c.prim ? 0u : f.env.defer;
        // the hand-over list: queue indices, then (split shade pass) the plane of their hits
        const uint32_t list_cap = (uint32_t)s.trace_blocks * WF_THREADS;
        uint4* list_hits = (uint4*)((uint32_t*)pipe.deferred.p + list_cap);
        c.split_shade = f.env.split && W.defer_age != 0u && pipe.side_wide != nullptr;
        W.list_cap = list_cap;
        W.split_deferred = c.split_shade ? 1u : 0u;
        // The casts the wavefront walker does not take (slack_is_capped): one lane each on the grown-box walker.
        // Bounces >= 1: k_wf_shade listed them when it made the rays, so the launch goes out BEFORE the
        // persistent kernel, on a stream of its own, and runs beside it (its few hundred workgroups take
        // their slots first; the persistent grid's last workgroups start as those free up).  Camera rays of
        // the KD-tree pipeline: k_wf_trace lists them, the launch follows it.
        W.exact_handover = f.env.exact ? (c.prim ? 1u : f.env.exact) : 0u;
        // (beside the persistent kernel: a SMALL grid - every workgroup of it takes a slot from k_wf_trace for as
        // long as it runs, and 2048 workgroups held most of the chip for milliseconds: closed room 185 -> 199 ms.
        // PT_WF_EXACT_BLOCKS: workgroups per 8 CUs)
        auto launch_exact = [&](hipStream_t st_exact) {
            const dim3 eg(W.exact_handover == 2u ? std::max(1u, (uint32_t)s.n_cu * f.env.exact_blocks / 8u) : (uint32_t)s.n_cu * 16u);
            dispatch([&](auto count, auto alpha, auto prim) {
                hipLaunchKernelGGL((k_wf_trace_exact<count, alpha, prim>), eg, dim3(WF_EXACT_THREADS), 0, st_exact, f.dev, W, f.d_tiles,
                                   (const float4*)c.q_in, (uint4*)pipe.hits.p, (const uint4*)c.rng_planes, (uint32_t*)pipe.draws.p,
                                   (uint32_t*)pipe.exact[b & 1].p, (const WfCounters*)c.wctr, f.gctr);
            }, f.counting, f.alpha, c.prim);
            HIP_CHECK(hipGetLastError());
        };
        auto exact_pass = [&] {   // beside the shade pass over the queue if that is split off
            if (c.split_shade) {
                HIP_CHECK(hipEventRecord(pipe.ev_exact_go, c.st_main));   // (the shade pass that listed them is done)
                HIP_CHECK(hipStreamWaitEvent(pipe.side_exact, pipe.ev_exact_go, 0));
                launch_exact(pipe.side_exact);
                HIP_CHECK(hipEventRecord(pipe.ev_exact, pipe.side_exact));
            } else {
                launch_exact(c.st_main);
            }
        };
        if (W.exact_handover == 2u) exact_pass();
        dispatch([&](auto alpha, auto count, auto prim) {
            hipLaunchKernelGGL((k_wf_trace<alpha, count, prim>), dim3(s.trace_blocks), dim3(WF_THREADS), 0, c.st_main, f.dev, W, f.d_tiles,
                               c.q_in, (uint4*)pipe.hits.p, (const uint4*)c.rng_planes, (uint32_t*)pipe.draws.p, (uint32_t*)pipe.deferred.p,
                               (uint32_t*)pipe.exact[b & 1].p, c.wctr, f.gctr);
        }, f.alpha, f.counting, c.prim);
        HIP_CHECK(hipGetLastError());
        if (W.exact_handover == 1u) exact_pass();   // behind k_wf_trace
        if (W.defer_age) {   // the casts the drained wavefronts handed over (pt_wavefront.h)
            // split shade pass: on a stream of its own, underneath k_wf_shade's pass over the queue
            hipStream_t st_wide = c.split_shade ? pipe.side_wide : c.st_main;
            // (16 Ki casts per pass; a workgroup without a cast returns at once)
            const uint32_t wide_grid = (uint32_t)s.n_cu * 4u * (WF_WIDE_LANES / 16u > 0u ? WF_WIDE_LANES / 16u : 1u);
            uint4* wide_hits = c.split_shade ? list_hits : (uint4*)pipe.hits.p;
            if (c.split_shade) {
                HIP_CHECK(hipEventRecord(pipe.ev_trace, c.st_main));
                HIP_CHECK(hipStreamWaitEvent(st_wide, pipe.ev_trace, 0));
            }
            dispatch([&](auto count, auto alpha) {
                hipLaunchKernelGGL((k_wf_trace_wide<count, alpha>), dim3(wide_grid), dim3(WF_THREADS), 0, st_wide, f.dev, W, f.d_tiles,
                                   (const float4*)c.q_in, wide_hits, (const uint4*)c.rng_planes, (uint32_t*)pipe.draws.p,
                                   (const uint32_t*)pipe.deferred.p, (const WfCounters*)c.wctr, f.gctr);
            }, f.counting, f.alpha);
            HIP_CHECK(hipGetLastError());
        }
        if (c.split_shade) HIP_CHECK(hipEventRecord(pipe.ev_wide, pipe.side_wide));
    }
    tl.end();
    ++tl.launches;
}

// A bounce of a chunk whose hits one of the scene's hit caches holds (Chunk::bounce_hits, mode SB_LOAD; `unknown`: that cache's
// counter), in place of trace_stage: k_wf_hits_load instead of k_wf_trace and k_wf_trace_wide, then k_wf_trace_exact for the
// items without a record (normally none: the launch finds an empty list and returns).  All on the main stream, the shade pass
// behind them unsplit: nothing is left that a second launch could run beside.  The shade pass before such a bounce listed no
// ray for k_wf_trace_exact (render_chunk), so the list holds the unknown casts alone.  A chunk whose bounce-0 kernel read the
// plane itself (Chunk::hit1_fused, bounce 1): that kernel wrote the words, the hits and the list - k_wf_trace_exact alone.
void hits_load_stage(pt_scene& s, const Frame& f, Chunk& c, Timeline& tl, unsigned long long* unknown) {
    const pt_scene::WfPipe& pipe = s.pipe;
    WfParams& W = c.W;
    const uint32_t b = c.b;
    tl.begin(1);
    W.defer_age = 0u;
    W.list_cap = (uint32_t)s.trace_blocks * WF_THREADS;
    W.split_deferred = 0u;
    W.exact_handover = f.env.exact;
    c.split_shade = false;
    if (!(c.hit1_fused && b == 1u) && !((c.b1_fused & SB_NEXT1) && b == 2u)) {   // (... or whose bounce-1 shade pass did, bounce 2)
        const uint32_t grid = std::max(1u, std::min((uint32_t)s.n_cu * 16u, (W.qcap_in + 255u) / 256u));
        hipLaunchKernelGGL(k_wf_hits_load, dim3(grid), dim3(256), 0, c.st_main, W, (const float4*)c.q_in, c.hits,
                           (uint32_t*)pipe.exact[b & 1].p, c.wctr, (const uint4*)c.bounce_hits[b].plane, unknown);
        HIP_CHECK(hipGetLastError());
    }
    const dim3 eg(f.env.exact == 2u ? std::max(1u, (uint32_t)s.n_cu * f.env.exact_blocks / 8u) : (uint32_t)s.n_cu * 16u);
    hipLaunchKernelGGL((k_wf_trace_exact<false, false, false>), eg, dim3(WF_EXACT_THREADS), 0, c.st_main, f.dev, W, f.d_tiles,
                       (const float4*)c.q_in, c.hits, (const uint4*)c.rng_planes, (uint32_t*)pipe.draws.p,
                       (uint32_t*)pipe.exact[b & 1].p, (const WfCounters*)c.wctr, f.gctr);
    HIP_CHECK(hipGetLastError());
    tl.end();
    ++tl.launches;
}

// Behind a bounce of a chunk that extends the prefix of one of the scene's hit caches (Chunk::bounce_hits, mode SB_STORE): the final
// hits of the bounce's queue to the plane.  On the main stream, before the next bounce's casts rewrite the chunk's hit plane,
// the hand-over list and this bounce's exact list.  Only a chunk's first store is a stage of the timeline (PT_FLAG_TIMING): a
// storing frame comes once per key, and its stage count stays one above a plain frame's whatever the number of planes.
void hits_store_stage(pt_scene& s, const Frame& f, const Chunk& c, Timeline& tl, uint32_t holes, uint64_t g0, bool first) {
    const pt_scene::WfPipe& pipe = s.pipe;
    const WfParams& W = c.W;
    if (first) tl.begin(1);
    const uint32_t grid = std::max(1u, std::min((uint32_t)s.n_cu * 16u, (W.qcap_in + 255u) / 256u));
    hipLaunchKernelGGL(k_wf_hits_store, dim3(grid), dim3(256), 0, c.st_main, W, (const float4*)c.q_in, (const uint4*)pipe.hits.p,
                       (const uint32_t*)pipe.deferred.p, (const uint32_t*)pipe.exact[c.b & 1].p, (const WfCounters*)c.wctr,
                       c.bounce_hits[c.b].plane, holes, holes ? (uint32_t)(g0 % holes) : 0u);
    HIP_CHECK(hipGetLastError());
    if (first) tl.end();
}

// launch(std::integral_constant<int, code>) for a code of one of the shade pass's tables (pt_wavefront.h WF_SHADE_*_CODES):
// every listed variant is instantiated, a code that is not listed is an error.
template <const auto& Codes, size_t I = 0, class F>
void launch_variant(int code, F&& launch) {
    if constexpr (I == std::size(Codes)) fail(PT_ERR_DEVICE, "internal error: no shade kernel for variant %d", code);
    else if (code == Codes[I]) launch(std::integral_constant<int, Codes[I]>{});
    else launch_variant<Codes, I + 1>(code, launch);
}

// k_wf_shade over the bounce's queue (split shade pass: then over the casts k_wf_trace_wide took meanwhile).
void shade_stage(pt_scene& s, const Frame& f, const WfFrame& wf, const Chunk& c, Timeline& tl) {
    const pt_scene::WfPipe& pipe = s.pipe;
    const WfParams& W = c.W;
    const uint32_t b = c.b;
    // shade(b) reads the colours shadow(b-1) patched and refills the shadow queue it consumed
    if (c.st_shadow != c.st_main && b > 0) HIP_CHECK(hipStreamWaitEvent(c.st_main, pipe.ev_shadow, 0));
    // (no more workgroups than the chunk has 256-entry steps)
    uint32_t shade_grid = std::max(1u, std::min((uint32_t)s.n_cu * (c.prim ? f.env.shade_blocks_b0 : f.env.shade_blocks),
                                                (W.n_items + WF_SHADE_THREADS - 1u) / WF_SHADE_THREADS));
    if (tl.on && c.grid_mode >= 2) tl.fused_marks.push_back(tl.ev);
    tl.begin(2);
    const uint4* shade_hits = (const uint4*)c.hits;
    const uint32_t* shade_list = nullptr;
    const uint32_t* block_empty = c.grid_mode >= 2 ? wf.block_empty : nullptr;
    // k_wf_shade<ALPHA, COUNT, PRIMARY, GRID>; GRID + 4: the variants with the orthographic branch for directional lights
    // compiled in.  GRID 2 and 3 cast the camera rays: they exist for PRIMARY only.
    auto launch = [&](auto grid) {
        constexpr int G = decltype(grid)::value;
        auto go = [&](auto alpha, auto count, auto prim) {
            hipLaunchKernelGGL((k_wf_shade<alpha, count, prim, G>), dim3(shade_grid), dim3(WF_SHADE_THREADS), 0, c.st_main, f.dev, W,
                               f.d_tiles, (const float4*)c.q_in, shade_hits, (const uint4*)c.rng_planes, (const uint32_t*)pipe.draws.p,
                               c.q_out, (float4*)pipe.shadow.p, (float4*)pipe.contrib.p, (float*)s.staging_buf.p, shade_list,
                               (const uint32_t*)pipe.exact[b & 1].p, (const uint4*)c.hits, (uint32_t*)pipe.exact[(b + 1) & 1].p,
                               block_empty, c.wctr, f.gctr);
        };
        if constexpr ((G & SB_CACHED) != 0) dispatch([&](auto alpha) { go(alpha, std::false_type{}, std::true_type{}); }, f.alpha);
        else if constexpr ((G & SB_GRID_MASK) >= 2) dispatch([&](auto alpha, auto count) { go(alpha, count, std::true_type{}); }, f.alpha, f.counting);
        else dispatch(go, f.alpha, f.counting, c.prim);
        HIP_CHECK(hipGetLastError());
    };
    // the cached opaque bounce-0 kernel with the camera-hit cache (k_wf_shade_hits): stores the chunk's hits or loads them;
    // SB_VIS, with the shadow-visibility cache (an overload with one parameter more): loads the hits, reads the chunk's
    // visibility bytes and fills in the unknown; SB_NEXT, with the bounce-1 hit cache (three parameters more): answers the
    // survivors' next casts from the chunk's records there; SB_CONT_STORE / SB_CONT_LOAD, with the continuation cache (two
    // parameters more, the loading variant's flags a third): stores the sampled direction and the throughput / loads them
    auto launch_hits = [&](auto grid) {
        constexpr int G = decltype(grid)::value;
        auto go = [&](auto... planes) {
            hipLaunchKernelGGL((k_wf_shade_hits<G>), dim3(shade_grid), dim3(WF_SHADE_THREADS), 0, c.st_main, f.dev, W, f.d_tiles,
                               (const uint4*)c.rng_planes, c.hit_plane, c.q_out, (float4*)pipe.shadow.p, (float4*)pipe.contrib.p,
                               (float*)s.staging_buf.p, (uint32_t*)pipe.exact[(b + 1) & 1].p, block_empty, c.wctr, planes...);
        };
        constexpr int taken = G & SB_PLANES;   // (the overload's plane bits)
        if constexpr (taken == (SB_LOAD | SB_VIS | SB_NEXT | SB_CONT_LOAD)) go(c.vis_plane, (const uint4*)c.bounce_hits[1].plane, (uint4*)pipe.hits.p, c.next_ctr, c.cont_plane, c.cont_stride, c.cont_flags);
        else if constexpr (taken == (SB_LOAD | SB_VIS | SB_CONT_STORE)) go(c.vis_plane, c.cont_plane, c.cont_stride);
        else if constexpr (taken == (SB_STORE | SB_CONT_STORE)) go(c.cont_plane, c.cont_stride);
        else if constexpr (taken == (SB_LOAD | SB_VIS | SB_NEXT)) go(c.vis_plane, (const uint4*)c.bounce_hits[1].plane, (uint4*)pipe.hits.p, c.next_ctr);
        else if constexpr (taken == (SB_LOAD | SB_VIS)) go(c.vis_plane);
        else go();
        HIP_CHECK(hipGetLastError());
    };
    // the bounce-1 shade pass that reads the bounce-1 visibility itself, SB_NEXT1: and the bounce-2 hits (k_wf_shade_fused).  Stream
    // order: the bytes it reads on the main stream were written on the side stream by k_og_shadow_vis of an earlier chunk -
    // the chunk-end join of render_chunk put that behind this launch - or of an earlier frame, which the frame order (and, for a
    // frame on another stream, the cache's event) put there; chunks of one batch touch disjoint slots, and this launch
    // never writes the plane.  Its own k_og_shadow_vis follows it on the side stream (ev_shade) and records the cache's event.
    auto launch_fused = [&](auto grid) {
        constexpr int G = decltype(grid)::value;
        hipLaunchKernelGGL((k_wf_shade_fused<G>), dim3(shade_grid), dim3(WF_SHADE_THREADS), 0, c.st_main, f.dev, W, f.d_tiles,
                           (const float4*)c.q_in, shade_hits, (const uint4*)c.rng_planes, c.q_out, (float4*)pipe.shadow.p,
                           (float4*)pipe.contrib.p, (float*)s.staging_buf.p, shade_list, (const uint32_t*)pipe.exact[b & 1].p,
                           (const uint4*)c.hits, (uint32_t*)pipe.exact[(b + 1) & 1].p, c.wctr, (const uint8_t*)c.bounce_vis_plane[b],
                           (const uint4*)c.bounce_hits[2].plane, (uint4*)pipe.hits_next.p, wf.fused_ctr(b));   // (the planes of SB_NEXT1: bounce 1 only)
        HIP_CHECK(hipGetLastError());
    };
    auto launch_shade = [&] {
        const bool cached_b0 = c.grid_mode == 3 && c.cached;
        if (c.fused && c.lean1) {   // (bounce 1 or 2, SB_VIS1 alone: render_chunk)
            // the lean variant lists what it cannot shade; the general body over that list follows at once - in front of
            // this bounce's k_og_shadow_vis, the ev_shade record and the next bounce's k_wf_hits_load.  Always launched:
            // a small grid that reads the count on the device
            shade_list = (const uint32_t*)pipe.handover.p;
            launch_variant<WF_SHADE_FUSED_CODES>(wf_shade_fused_code((c.fused & SB_NEXT1) != 0, true, false), launch_fused);
            const uint32_t whole = shade_grid;
            shade_grid = std::min(shade_grid, (uint32_t)s.n_cu);
            launch_variant<WF_SHADE_FUSED_CODES>(wf_shade_fused_code(false, false, true), launch_fused);
            shade_grid = whole;
            shade_list = nullptr;
        } else if (c.fused) {   // (bounces 1-4 of a chunk whose batch has that bounce's visibility bytes: render_chunk)
            launch_variant<WF_SHADE_FUSED_CODES>(wf_shade_fused_code((c.fused & SB_NEXT1) != 0, false, false), launch_fused);
        } else if (cached_b0 && c.hit_mode) {
            launch_variant<WF_SHADE_HITS_CODES>(wf_shade_hits_code(s.grids.ortho, c.hit_mode, c.vis_plane != nullptr, c.hit1_fused, c.cont_mode, c.lean), launch_hits);
        } else {
            launch_variant<WF_SHADE_CODES>(wf_shade_code(c.grid_mode, s.grids.ortho, cached_b0), launch);
        }
    };
    launch_shade();
    if (c.split_shade) {
        // ... and the casts that were with k_wf_trace_wide meanwhile: the hand-over list (at most one entry per
        // lane of the trace grid; usually a few thousand - a launch that finds an empty list returns)
        HIP_CHECK(hipStreamWaitEvent(c.st_main, pipe.ev_wide, 0));
        if (W.exact_handover) HIP_CHECK(hipStreamWaitEvent(c.st_main, pipe.ev_exact, 0));
        shade_hits = (const uint4*)((const uint32_t*)pipe.deferred.p + W.list_cap);
        shade_list = (const uint32_t*)pipe.deferred.p;
        shade_grid = std::min(shade_grid, (uint32_t)s.n_cu);
        launch_shade();
    }
    tl.end();
}

// The shadow casts the shade pass left in the shadow queue: on the side stream, beside the next bounce's trace.
void shadow_stage(pt_scene& s, const Frame& f, const Chunk& c, Timeline& tl) {
    const pt_scene::WfPipe& pipe = s.pipe;
    // (inline casts leave at most a few records in the shadow queue: that launch stays on the main stream,
    // behind a persistent trace grid on another stream it would wait milliseconds for a free slot)
    const hipStream_t st_shadow = c.grid_mode != 0 ? c.st_main : c.st_shadow;
    if (st_shadow != c.st_main) {
        HIP_CHECK(hipEventRecord(pipe.ev_shade, c.st_main));
        HIP_CHECK(hipStreamWaitEvent(st_shadow, pipe.ev_shade, 0));
    }
    tl.stream = st_shadow;
    tl.begin(3);
    WfParams Ws = c.W;
    if (f.env.refill_shadow) Ws.refill_min = std::min(64u, f.env.refill_shadow);
    if (f.env.walk_shadow) Ws.walk_steps = f.env.walk_shadow;
    // what is left to k_og_shadow_offgrid: surfaces with a normal too long for the grids' margin, the rays the wavefront
    // walker does not take (normally none, or a few per mille: the launch finds an empty queue and returns)
    auto offgrid = [&](auto list, uint32_t grid) {
        constexpr bool LIST = decltype(list)::value;
        dispatch([&](auto count) {
            hipLaunchKernelGGL((k_og_shadow_offgrid<count, LIST>), dim3(grid), dim3(256), 0, st_shadow, f.dev, Ws, (const float4*)pipe.shadow.p,
                               (const float4*)pipe.contrib.p, c.q_out, (float*)s.staging_buf.p, (uint32_t*)pipe.offgrid.p, c.wctr, f.gctr);
        }, f.counting);
        HIP_CHECK(hipGetLastError());
    };
    if (c.grid_mode != 0) {
        offgrid(std::false_type{}, (uint32_t)s.n_cu);
    } else if (f.use_light_grids) {   // every light a point light with a grid: plain grid-stride kernel
        const dim3 g((uint32_t)s.n_cu * std::max(1u, f.env.ogs_blocks));
        if (c.vis_plane_of(c.b)) {  // the scene's shadow-visibility cache of this bounce (opaque, uninstrumented frames)
            dispatch([&](auto dirl) {
                hipLaunchKernelGGL((k_og_shadow_vis<dirl>), g, dim3(256), 0, st_shadow, f.dev, Ws, (const float4*)pipe.shadow.p,
                                   (const float4*)pipe.contrib.p, c.q_out, (float*)s.staging_buf.p, (uint32_t*)pipe.offgrid.p, c.wctr,
                                   c.bounce_vis_plane[c.b]);
            }, s.grids.ortho);
        } else {
            dispatch([&](auto alpha, auto count, auto dirl) {
                hipLaunchKernelGGL((k_og_shadow<alpha, count, dirl>), g, dim3(256), 0, st_shadow, f.dev, Ws, (const float4*)pipe.shadow.p,
                                   (const float4*)pipe.contrib.p, c.q_out, (float*)s.staging_buf.p, (uint32_t*)pipe.offgrid.p, c.wctr, f.gctr);
            }, f.alpha, f.counting, s.grids.ortho);
        }
        HIP_CHECK(hipGetLastError());
        offgrid(std::true_type{}, (uint32_t)s.n_cu);
    } else {
        dispatch([&](auto alpha, auto count) {
            hipLaunchKernelGGL((k_wf_shadow<alpha, count>), dim3(s.shadow_blocks), dim3(WF_THREADS), 0, st_shadow, f.dev, Ws, (float4*)pipe.shadow.p,
                               (const float4*)pipe.contrib.p, c.q_out, (float*)s.staging_buf.p, (uint32_t*)pipe.offgrid.p, c.wctr, f.gctr);
        }, f.alpha, f.counting);
        HIP_CHECK(hipGetLastError());
        if (Ws.exact_handover) offgrid(std::true_type{}, (uint32_t)s.n_cu * 4u);   // ... and the jobs k_wf_shadow set aside
    }
    tl.end();
    tl.stream = c.st_main;
    if (st_shadow != c.st_main) HIP_CHECK(hipEventRecord(pipe.ev_shadow, st_shadow));
    else if (c.st_shadow != c.st_main) HIP_CHECK(hipEventRecord(pipe.ev_shadow, c.st_main));   // (keeps the waits below valid)
}

// Work items [base, base + cap) of a sample batch: their RNG planes, then per bounce the trace, shade and shadow stages.
void render_chunk(pt_scene& s, const Frame& f, WfFrame& wf, Timeline& tl, const RenderParams& P, hipStream_t stream,
                  uint32_t base, uint32_t total_items, uint32_t chunk_no) {
    const pt_scene::WfPipe& pipe = s.pipe;
    Chunk c;
    c.st_main = stream;
    c.st_shadow = f.env.overlap ? pipe.side : stream;
    // opaque scenes, several chunks: the RNG planes of chunk c+1 are produced on their own stream while
    // chunk c runs its bounces (k_wf_rng is pure integer ALU work; the traversal kernels leave ~40 % of
    // the issue slots idle and end in a drain phase)
    // both kinds of grid: the bounce-0 kernel computes the ChaCha block itself (GRID 3; PT_OG_FUSE_RNG=0: off)
    const bool fused_rng = wf.rng_one_plane;
    const bool rng_ahead = !fused_rng && f.env.overlap && total_items > wf.cap && pipe.side != nullptr && pipe.ev_rng != nullptr;
    WfParams& W = c.W;
    W.P = P;
    W.item_base = base;
    W.n_items = std::min(wf.cap, total_items - base);
    W.cap = wf.cap;
    W.hcap = wf.cap_h;
    W.scap = wf.cap_s;
    W.ecap = wf.cap_e;
    W.qcap_in = wf.cap_q[0];
    W.qcap_out = wf.cap_q[1];
    W.rng_first_plane = wf.rng_one_plane ? 1u : 0u;
    W.n_mask_blocks = f.blocks64;
    c.rng_planes = (uint4*)pipe.rng[rng_ahead ? (chunk_no & 1u) : 0u].p;
    W.sort_octants = f.env.sort;
    W.use_entry = f.env.entry;
    W.exact_handover = f.env.exact ? 1u : 0u;   // (per bounce in trace_stage: 1 k_wf_trace lists, 2 k_wf_shade listed)
    W.exact_shade_lists = f.env.exact == 2u ? 1u : 0u;
    W.refill_min = std::max(1u, std::min(64u, f.env.refill));
    W.walk_steps = f.env.walk ? f.env.walk : 20u;
    c.wctr = (WfCounters*)pipe.ctr.p;
    HIP_CHECK(hipMemsetAsync(c.wctr, 0, sizeof(WfCounters) * (f.p.bounces + 3), c.st_main));
    // (the counts of the hand-over list, by bounce: a frame that may take the lean shade pass at bounce 1 or 2)
    const bool lean1_frame = (wf.b1_lean[1] || wf.b1_lean[2] || wf.b1_lean_forced) && pipe.handover.p != nullptr;
    if (lean1_frame) HIP_CHECK(hipMemsetAsync(pipe.handover.p, 0, WF_HANDOVER_HEAD * 4u, c.st_main));
    // The scene's frame caches, one prefix in the frame-global item g (chunk boundaries differ between a first frame and a
    // planned one: the prefix does not care); this chunk is [g0, g1)
    const uint64_t g0 = (uint64_t)(P.sample_begin / f.batch) * wf.items_per_batch + base, g1 = g0 + W.n_items;
    // does the chunk read the prefix (wholly below the mark), or extend it (next above the mark, the budget has room for all of it)?
    auto reads = [&](const pt_scene::FrameCache* fc) { return fc && g1 <= fc->mark; };
    auto extends = [&](const pt_scene::FrameCache* fc) { return fc && g1 > fc->mark && g1 <= fc->stride && g0 <= fc->mark; };
    if (fused_rng && (reads(wf.rng_cache) || extends(wf.rng_cache))) {
        // the words: read from the cache, filled first - here on the frame's stream - by the chunk that extends the prefix
        pt_scene::FrameCache& rc = *wf.rng_cache;
        uint4* planes = (uint4*)rc.buf.p + g0;
        if (extends(&rc)) {
            const uint32_t first = (uint32_t)(rc.mark - g0), n = (uint32_t)(g1 - rc.mark);
            tl.begin(0);
            hipLaunchKernelGGL(k_wf_rng_fill, dim3((n + 255u) / 256u), dim3(256), 0, c.st_main, W, f.d_tiles, first, n, planes,
                               (uint32_t)rc.stride);
            HIP_CHECK(hipGetLastError());
            tl.end();
            rc.touched(c.st_main);
            rc.mark = g1;
            ++rc.counter[0];
        }
        c.cached = true;
        c.rng_planes = planes;
        W.cap = (uint32_t)rc.stride;
        W.rng_first_plane = 0u;
    }
    if (c.cached) {
        // the camera hits: loaded by the bounce-0 kernel, or stored by it; anything else casts as before.  The shadow
        // visibility: a chunk that loads its hits and lies wholly below the plane's stride
        c.hit_mode = reads(wf.hit_cache) ? SB_LOAD : extends(wf.hit_cache) ? SB_STORE : 0;
        if (c.hit_mode) c.hit_plane = (uint4*)wf.hit_cache->buf.p + g0;
        if (c.hit_mode == SB_LOAD && wf.vis_cache && g1 <= wf.vis_cache->stride) c.vis_plane = (uint8_t*)wf.vis_cache->buf.p + g0;
    }
    // the later bounces' hits: loaded in place of the bounce's casts, or stored behind them; anything else casts as before
    for (uint32_t b = 1; b < WfFrame::HIT_BOUNCES; ++b) {
        const pt_scene::FrameCache* fc = wf.bounce_hits[b].cache;
        Chunk::BounceHits& bh = c.bounce_hits[b];
        bh.mode = reads(fc) ? SB_LOAD : extends(fc) ? SB_STORE : 0;
        if (bh.mode) bh.plane = (uint4*)fc->buf.p + g0;
        if (bh.mode == SB_LOAD && wf.stats_slots && wf.stats_line < wf.stats_slots) wf.fs->stats_hit_loads |= 1u << b;
    }
    // ... and the bounce-1 hits by the bounce-0 kernel itself, where that loads the camera hits and the visibility too
    c.hit1_fused = wf.hit1_fused && c.hit_mode == SB_LOAD && c.vis_plane != nullptr && c.hits_mode(1u) == SB_LOAD;
    c.next_ctr = wf.bounce_hits[1].unknown;
    // the continuations: loaded by the launch that reads the bounce-1 hits itself where the chunk lies below their mark too;
    // stored by the bounce-0 launch of a chunk whose bounce-1 hits are stored in this frame - one that stores its camera hits,
    // or loads them with the visibility - where the chunk is next above the mark and the budget has room for it
    if (c.hit1_fused && reads(wf.cont_cache)) c.cont_mode = SB_CONT_LOAD;
    else if (c.hits_mode(1u) == SB_STORE && extends(wf.cont_cache) && (c.hit_mode == SB_STORE || (c.hit_mode == SB_LOAD && c.vis_plane))) c.cont_mode = SB_CONT_STORE;
    if (c.cont_mode) {
        c.cont_plane = (uint4*)wf.cont_cache->buf.p + g0;
        c.cont_stride = (size_t)wf.cont_cache->stride;
    }
    // The records' escape answers.  Masks the prefix was not stored under (built or rebuilt since): the part of this chunk below
    // the marks of the camera hits and the continuations is refilled here, in front of the launch that loads it -
    // k_cont_escape_fill, once per record and mask generation; chunks come in frame order, so the refilled part is a prefix too.
    // Masks dropped: nothing to do - no flag without masks.  A translucent scene keys no continuation cache: no launch.
    if (wf.cont_cache && wf.hit_cache && c.cached && wf.cont_escape && f.dev.escape && s.cont_escape_generation != s.escape_generation) {
        if (s.cont_fill_generation != s.escape_generation) {
            s.cont_fill_generation = s.escape_generation;
            s.cont_fill_mark = 0;
        }
        const uint64_t below = std::min({g1, wf.cont_cache->mark, wf.hit_cache->mark});
        if (g0 <= s.cont_fill_mark && below > s.cont_fill_mark) {
            const uint32_t n = (uint32_t)(below - g0);
            // (no stage of the timeline: it comes once per record and mask build, like the build itself)
            hipLaunchKernelGGL(k_cont_escape_fill, dim3(std::max(1u, std::min((uint32_t)s.n_cu * 8u, (n + 255u) / 256u))), dim3(256), 0, c.st_main,
                               f.dev, W, f.d_tiles, (const uint4*)c.rng_planes, (const uint4*)((uint4*)wf.hit_cache->buf.p + g0),
                               (uint4*)wf.cont_cache->buf.p + g0, (size_t)wf.cont_cache->stride, n);
            HIP_CHECK(hipGetLastError());
            wf.cont_cache->touched(c.st_main);
            s.cont_fill_mark = below;
            ++s.cont_fill_launches;
            s.cont_fill_items += n;
        }
        if (s.cont_fill_mark >= wf.cont_cache->mark) s.cont_escape_generation = s.escape_generation;
    }
    if (c.cont_mode == SB_CONT_LOAD && wf.cont_escape && f.dev.escape &&
        (s.cont_escape_generation == s.escape_generation || (s.cont_fill_generation == s.escape_generation && g1 <= s.cont_fill_mark))) {
        c.cont_flags = 1u;
        ++s.cont_flagged_launches;
    }
    // the lean variant: a loading launch without the orthographic branch whose records answer the escape test (or a scene
    // without masks: nobody asks), in a frame of a configuration that was counted clean; a counted frame with any other
    // bounce-0 launch is not a clean one
    {
        const bool answered = c.cont_mode == SB_CONT_LOAD && ((c.cont_flags & 1u) != 0u || !f.dev.escape);
        c.lean = c.cont_mode == SB_CONT_LOAD && !s.grids.ortho && ((wf.lean && answered) || wf.lean_forced);
        if (wf.stats_slots && wf.stats_line < wf.stats_slots && !answered) wf.fs->stats_lean_ok = false;
    }
    // the shadow visibility of bounces 1-4: indexed by the sample's slot in its batch's staging area, which any chunk of the
    // batch may hold - so the whole batch lies below the plane's stride, not the chunk alone
    for (uint32_t b = 1; b < WfFrame::HIT_BOUNCES; ++b) {
        const pt_scene::FrameCache* vc = wf.bounce_vis[b];
        if (!vc) continue;
        const uint64_t batch0 = (uint64_t)(P.sample_begin / f.batch) * wf.items_per_batch;
        const uint64_t batch1 = batch0 + (uint64_t)f.blocks64 * 64u * (P.sample_end - P.sample_begin);
        if (batch1 <= vc->stride) c.bounce_vis_plane[b] = (uint8_t*)vc->buf.p + batch0;
    }
    if (fused_rng && !c.cached && pipe.rng[0].bytes < (size_t)wf.cap * 16u) {   // (queue_buffers left the plane out)
        s.pipe.rng[0].ensure((size_t)wf.cap * 16u);
        c.rng_planes = (uint4*)pipe.rng[0].p;
    }
    if (fused_rng) {
        // (no k_wf_rng launch)
    } else if (!rng_ahead || chunk_no == 0) {
        tl.begin(0);
        hipLaunchKernelGGL(k_wf_rng, dim3((W.n_items + 255u) / 256u), dim3(256), 0, c.st_main, f.dev, W, f.d_tiles, c.rng_planes);
        HIP_CHECK(hipGetLastError());
        tl.end();
    } else {
        HIP_CHECK(hipStreamWaitEvent(c.st_main, pipe.ev_rng, 0));  // produced underneath the previous chunk
    }
    if (rng_ahead && base + wf.cap < total_items) {
        // the other copy was last read by chunk c-1, which has completed on st_main by now
        WfParams Wn = W;
        Wn.item_base = base + wf.cap;
        Wn.n_items = std::min(wf.cap, total_items - Wn.item_base);
        HIP_CHECK(hipEventRecord(pipe.ev_chunk, c.st_main));
        HIP_CHECK(hipStreamWaitEvent(pipe.side, pipe.ev_chunk, 0));
        tl.stream = pipe.side;
        tl.begin(0);
        hipLaunchKernelGGL(k_wf_rng, dim3((Wn.n_items + 255u) / 256u), dim3(256), 0, pipe.side, f.dev, Wn, f.d_tiles,
                           (uint4*)pipe.rng[(chunk_no + 1u) & 1u].p);
        HIP_CHECK(hipGetLastError());
        tl.end();
        tl.stream = c.st_main;
        HIP_CHECK(hipEventRecord(pipe.ev_rng, pipe.side));
    }
    // (the plan knows where this chunk's last ray ends: the launches of the bounces behind it - ~85 us each for nothing -
    // are not made; PT_PLAN_SKIP=0: all of them)
    const uint32_t b_end = (wf.plan_last && wf.chunk_slot < wf.plan_last->size()) ? std::min(f.p.bounces, (*wf.plan_last)[wf.chunk_slot]) : f.p.bounces;
    ++wf.chunk_slot;
    bool stored = false;   // a store of this chunk has been launched
    for (uint32_t b = 0; b <= b_end; ++b) {
        W.bounce = b;
        W.qcap_in = wf.cap_q[b & 1u];          // (queue b lives in pipe.queue[b & 1])
        W.qcap_out = wf.cap_q[(b + 1u) & 1u];
        // (node steps per walking phase: 12 until the escape masks took the short casts out of the queues; re-swept on the rays that
        // are left - 12 / 14 / 16 / 18: config 3 40.3-40.8 / 40.3-40.4 / 39.7-39.8 / 39.8-40.0 ms, closed room 173.9 -> 171.4)
        W.walk_steps = f.env.walk ? f.env.walk : (b == 0 ? 20u : 16u);
        c.b = b;
        c.q_in = (float4*)pipe.queue[b & 1].p;
        c.q_out = (float4*)pipe.queue[(b + 1) & 1].p;
        c.prim = b == 0;
        // (bounces >= 1: shadow casts inline with PT_OG_INLINE_ALL, or where the frame plan found (nearly) every ray of the
        // bounce reaching a lit surface)
        c.grid_mode = (c.prim && f.bounce0_fused) ? (fused_rng ? 3 : 2)
                                                  : (f.use_light_grids && (f.env.inline_all || (b < wf.inline_at.size() && wf.inline_at[b])) ? 1 : 0);
        c.split_shade = false;
        // Bounce 1 of a chunk whose batch has visibility bytes, its shadow records going through k_og_shadow_vis (an opaque,
        // uninstrumented frame with light grids: the cache serves no other): the shade pass adds the lights whose bits are
        // known itself; ... and, where the chunk loads its bounce-2 hits, answers its survivors' casts from that plane.  A
        // scene with the orthographic branch takes k_wf_shade, and so does a frame with a sorting option (PT_WF_SORT): the
        // kernel keeps its counts in the LDS row those options write.
        // Bounces 2-4 with a plane of their own: the same pass (SB_VIS1 alone: the next hits are k_wf_hits_load's), with that
        // bounce's bytes and a counter block of that bounce's own (WfFrame::fused_ctr).
        c.fused = 0;
        if (b < WfFrame::HIT_BOUNCES && wf.vis_fused[b] && c.vis_plane_of(b) && c.grid_mode == 0 && f.use_light_grids && !f.alpha && !f.counting && !s.grids.ortho && f.env.sort == 0u)
            c.fused = SB_VIS1 | ((b == 1u && wf.hit2_fused && c.hits_mode(2u) == SB_LOAD && pipe.hits_next.bytes >= (size_t)W.qcap_out * 20u) ? SB_NEXT1 : 0);
        if (b == 1u) c.b1_fused = c.fused;
        // (the hits of bounce 2 in such a chunk: a plane of their own, as long as the queue)
        c.hits = (b == 2u && (c.b1_fused & SB_NEXT1)) ? (uint4*)pipe.hits_next.p : (uint4*)pipe.hits.p;
        W.hcap = (b == 2u && (c.b1_fused & SB_NEXT1)) ? W.qcap_in : wf.cap_h;
        // (a chunk that loads the next bounce's hits: the rays k_wf_trace would leave to k_wf_trace_exact have records like any
        // other, so this bounce's shade pass lists none of them - the exact list of the next bounce is k_wf_hits_load's, for
        // the items without one)
        W.exact_shade_lists = (f.env.exact == 2u && c.hits_mode(b + 1u) != SB_LOAD) ? 1u : 0u;
        const int hits_mode = c.hits_mode(b);
        if (hits_mode == SB_LOAD) {
            hits_load_stage(s, f, c, tl, wf.bounce_hits[b].unknown);
            wf.bounce_hits[b].cache->touched(c.st_main);   // (no device sync before the plane is zeroed for a new key: the readers count)
            ++wf.bounce_hits[b].cache->counter[2];
        } else if (c.grid_mode < 2) {
            trace_stage(s, f, c, tl);   // (grid_mode >= 2: k_wf_shade casts the camera rays itself)
        }
        // The lean variant of the plain fused pass, bounces 1 and 2 (lean_frame: the counts say that next to no record of this
        // bounce needs the shadow queue, or the test hook): a matter of speed only - the list pass shades what it leaves.
        // (Not where the shade pass is split in two launches: the second one has a list of its own.)
        c.lean1 = lean1_frame && c.fused == SB_VIS1 && (b == 1u || b == 2u) && W.exact_shade_lists == 0u && !c.split_shade &&
                  (wf.b1_lean[b] || wf.b1_lean_forced) && pipe.handover.bytes >= ((size_t)W.qcap_in + WF_HANDOVER_HEAD) * 4u;
        shade_stage(s, f, wf, c, tl);
        if (c.prim && c.hit_mode == SB_STORE) {   // the records are behind this launch: the prefix grows by the chunk
            wf.hit_cache->touched(c.st_main);
            wf.hit_cache->mark = g1;
            ++wf.hit_cache->counter[0];
        } else if (c.prim && c.hit_mode == SB_LOAD) {
            ++wf.hit_cache->counter[1];
            if (c.hit1_fused) {   // (the bounce-1 plane is read here: its event and its count of loads follow at bounce 1)
                wf.bounce_hits[1].cache->touched(c.st_main);
                ++s.hit1_fused_launches;
            }
            if (c.vis_plane) {   // (any such launch may write the plane)
                wf.vis_cache->touched(c.st_main);
                ++wf.vis_cache->counter[1];
            }
        }
        if (c.prim && c.cont_mode == SB_CONT_STORE) {   // the records are behind this launch: the prefix grows by the chunk
            wf.cont_cache->touched(c.st_main);
            // (the masks this launch evaluated the escape test with: one generation for the whole prefix, or none)
            s.cont_escape_generation = (wf.cont_cache->mark == 0 || s.cont_escape_generation == s.escape_generation) ? s.escape_generation : 0;
            wf.cont_cache->mark = g1;
            ++wf.cont_cache->counter[1];
        } else if (c.prim && c.cont_mode == SB_CONT_LOAD) {   // (no device sync before the planes are zeroed for a new key: the readers count)
            wf.cont_cache->touched(c.st_main);
            ++wf.cont_cache->counter[2];
            ++(c.lean ? s.b0_lean_launches : s.b0_general_launches);
        }
        if (c.fused && (b == 1u || b == 2u)) ++(c.lean1 ? s.b1_lean_launches[b - 1u] : s.b1_general_launches);
        if (c.fused) {
            ++s.fused_launches(b);   // (by bounce: b1_fused_launches counts bounce 1's alone)
            if (c.fused & SB_NEXT1) wf.bounce_hits[2].cache->touched(c.st_main);   // (read here: its count of loads follows at bounce 2)
        }
        shadow_stage(s, f, c, tl);
        if (c.vis_plane_of(b) && c.grid_mode == 0) {   // (k_og_shadow_vis, on the side stream; any such launch may write the plane)
            wf.bounce_vis[b]->touched(c.st_shadow);
            ++wf.bounce_vis[b]->counter[1];
        }
        if (hits_mode == SB_STORE) {   // the records are behind this launch: the prefix grows by the chunk
            hits_store_stage(s, f, c, tl, wf.bounce_hits[b].holes, g0, !stored);
            stored = true;
            wf.bounce_hits[b].cache->touched(c.st_main);
            wf.bounce_hits[b].cache->mark = g1;
            ++wf.bounce_hits[b].cache->counter[1];
        }
    }
    for (uint32_t b = b_end + 1u; b < WfFrame::HIT_BOUNCES; ++b)   // (a chunk without a ray at that bounce: nothing to store)
        if (c.bounce_hits[b].mode == SB_STORE) wf.bounce_hits[b].cache->mark = g1;
    // the next chunk clears the counters and reuses the queues, accumulate reads the staging area:
    // join the side stream
    if (c.st_shadow != c.st_main) HIP_CHECK(hipStreamWaitEvent(c.st_main, pipe.ev_shadow, 0));
    if (wf.stats_slots && wf.stats_line < wf.stats_slots) {   // this chunk's counts: one line of the frame's statistics
        hipLaunchKernelGGL(k_wf_stats, dim3(1), dim3(64u * ((f.p.bounces + 3u + 63u) / 64u)), 0, c.st_main, (const WfCounters*)c.wctr,
                           f.p.bounces + 3u, (uint32_t*)s.stats_dev.p + (size_t)wf.stats_line * (f.p.bounces + 3u) * 4u,
                           (unsigned long long*)s.hit1_unknown.p, (uint32_t*)s.stats_dev.p + (size_t)wf.stats_slots * (f.p.bounces + 3u) * 4u + wf.stats_line,
                           (uint32_t*)s.stats_dev.p + (size_t)wf.stats_slots * ((f.p.bounces + 3u) * 4u + 1u) + 2u * wf.stats_line);
        HIP_CHECK(hipGetLastError());
        wf.fs->first_item_of_slot[wf.stats_line] = base;
        ++wf.stats_line;
    }
}

// After the frame's launches: its counts on their way to the host (read when the next frame is planned), the
// post-processing, timing and counters.
void frame_readout(pt_scene& s, const Frame& f, WfFrame& wf, Timeline& tl, void* d_rgb8, hipStream_t stream) {
    const pt_profile& p = f.p;
    if (wf.stats_slots && wf.stats_line == wf.stats_slots) {
        HIP_CHECK(hipMemcpyAsync(wf.fs->host, s.stats_dev.p, pt_scene::FrameStats::host_bytes(wf.stats_slots, p.bounces + 3u),
                                 hipMemcpyDeviceToHost, stream));
        HIP_CHECK(hipEventRecord(wf.fs->done, stream));
        wf.fs->pending = true;
    }
    const size_t ev_post = tl.ev;
    if (f.timing) HIP_CHECK(hipEventRecord(get_event(s, tl.ev++), stream));
    if (d_rgb8) {
        hipLaunchKernelGGL(k_postprocess, dim3(((uint32_t)f.tm.n_local + 255u) / 256u), dim3(256), 0, stream, f.accum,
                           (uint8_t*)d_rgb8, (uint32_t)f.tm.n_local, f.end_sample(), p.tonemap);
        HIP_CHECK(hipGetLastError());
    }
    if (f.timing) HIP_CHECK(hipEventRecord(get_event(s, tl.ev++), stream));

    if (f.timing || f.counting || f.exit_times) HIP_CHECK(hipStreamSynchronize(stream));
    if (f.timing) {
        pt_timing t{};
        t.launches = tl.launches;
        t.stage_launches = tl.stage_launches;
        float* slot[6] = {&t.generate_ms, &t.trace_ms, &t.shade_ms, &t.shadow_ms, &t.accumulate_ms, &t.integrate_ms};
        for (auto& m : tl.marks) {
            float ms = 0;
            HIP_CHECK(hipEventElapsedTime(&ms, s.events[m.second], s.events[m.second + 1]));
            *slot[m.first] += ms;
            if (f.env.debug_times) fprintf(stderr, "[pt] stage %d  %.3f ms\n", m.first, ms);
        }
        if (f.wavefront) t.integrate_ms = t.trace_ms;  // k_wf_trace launches of the wavefront integrator
        for (size_t m : tl.fused_marks) {
            float ms = 0;
            HIP_CHECK(hipEventElapsedTime(&ms, s.events[m], s.events[m + 1]));
            t.bounce0_ms += ms;
            ++t.bounce0_launches;
        }
        HIP_CHECK(hipEventElapsedTime(&t.postprocess_ms, s.events[ev_post], s.events[ev_post + 1]));
        HIP_CHECK(hipEventElapsedTime(&t.total_ms, s.events[0], s.events[ev_post + 1]));
        s.timing = t;
    }
#ifdef WF_EXIT_TIMES
    {   // diagnostic build: when did the wavefronts of every k_wf_trace launch run out of queue / exit? (us after launch start)
        std::unique_ptr<DevCounters> full(new DevCounters);
        HIP_CHECK(hipMemcpy(full.get(), s.counter_buf.p, sizeof(DevCounters), hipMemcpyDeviceToHost));
        for (int b = 0; b < 8; ++b) {
            std::vector<double> ex, qd;
            for (int w = 0; w < 8192; ++w)
                if (full->wave_exit[b][w]) {
                    ex.push_back((double)(full->wave_exit[b][w] - full->launch_start[b]) / 100.0);
                    if (full->wave_queue_done[b][w]) qd.push_back((double)(full->wave_queue_done[b][w] - full->launch_start[b]) / 100.0);
                }
            if (ex.empty()) continue;
            std::sort(ex.begin(), ex.end());
            std::sort(qd.begin(), qd.end());
            auto q = [](const std::vector<double>& v, double f) { return v.empty() ? 0.0 : v[std::min(v.size() - 1, (size_t)(f * v.size()))]; };
            fprintf(stderr, "[pt] trace bounce %d: %zu waves | queue exhausted (us) p1 %.0f p50 %.0f p99 %.0f max %.0f | exit p1 %.0f p10 %.0f p50 %.0f p90 %.0f p99 %.0f p99.9 %.0f max %.0f\n",
                    b, ex.size(), q(qd, 0.01), q(qd, 0.5), q(qd, 0.99), qd.empty() ? 0.0 : qd.back(), q(ex, 0.01), q(ex, 0.1), q(ex, 0.5), q(ex, 0.9), q(ex, 0.99), q(ex, 0.999), ex.back());
        }
    }
#endif
    if (f.counting) {
        DevCounters c;
        HIP_CHECK(hipMemcpy(&c, s.counter_buf.p, sizeof c, hipMemcpyDeviceToHost));
        s.counters = pt_counters{c.samples, c.segments, c.shadow_rays, c.nodes_visited, c.tris_tested, c.shaded_hits,
                                 c.rng_draws, c.restarts, c.max_nodes_per_cast, c.casts_over_1k_nodes,
                                 c.trace_nodes, c.trace_tris, c.shadow_skipped, c.bounce0_hits, c.bounce0_shadow_rays,
                                 c.bounce0_tris, c.grid_tris, c.bounce0_cam_tris, c.deferred_casts, c.exact_casts, c.masked_casts, c.bounce0_masked};
        if (f.env.debug_hist) {   // casts of k_wf_trace by length (bins of 64 node visits; bin 0 not counted)
            fprintf(stderr, "[pt] cast length histogram (x64 nodes):");
            for (int b = 1; b < 16; ++b) fprintf(stderr, " %llu", c.cast_hist[b]);
            fprintf(stderr, "\n[pt] wide casts %llu: rounds total %llu max %llu | node steps %llu | time per cast (us): mean %.1f max %.1f\n",
                    c.deferred_casts, c.stamps[0], c.stamps[1], c.stamps[3],
                    c.deferred_casts ? (double)c.stamps[5] / 100.0 / (double)c.deferred_casts : 0.0, (double)c.stamps[4] / 100.0);
        }
        if (f.env.debug_stamps)
            fprintf(stderr, "[pt] trace stamps: refill %llu walk %llu leaf %llu complete %llu cycles | walk lanes/step %.1f (%llu steps) | leaf lanes/run %.1f (%llu runs)\n",
                    c.stamps[0], c.stamps[1], c.stamps[2], c.stamps[3], c.stamps[5] ? (double)c.stamps[4] / c.stamps[5] : 0.0,
                    c.stamps[5], c.stamps[7] ? (double)c.stamps[6] / c.stamps[7] : 0.0, c.stamps[7]);
    }
}

// What a frame of the wavefront integrator can hand out besides accum (pt_variance.h): the luminance moments of every
// pixel's samples (n_local x 2 f32) and, for the tests, the staged samples themselves (samples x n_local x 3 f32).
struct FrameTaps {
    float2* moments = nullptr;
    float* samples = nullptr;
};

// One frame of pt_render, pt_render_device and pt_render_gathered; taps: of pt_render_moments and pt_render_samples.
// list: a tile-list frame (pt_render_tiles, pt_film_add_tile_pass).  win: a window frame (pt_render_window) - the batch loop
// runs over its samples only, and the first batch carries the sums d_accum and taps->moments hold unless the window starts at 0.
void render_device(pt_scene& s, const pt_profile& p, const pt_opts* opts_in, void* d_rgb8, void* d_accum,
                   hipStream_t stream, bool allow_preview = false, const FrameTaps* taps = nullptr, const TileList* list = nullptr,
                   const SampleWindow* win = nullptr) {
    Frame f;
    // (a tile-list or window frame refuses before any device work, and frame_setup waits for the device for it)
    if (taps && (list || win) && opts_in && (opts_in->flags & PT_FLAG_MEGAKERNEL)) fail(PT_ERR_UNSUPPORTED, "this pipeline stages no samples");
    if (!frame_setup(s, p, opts_in, d_accum, stream, f, list, win)) return;
    if (taps && !f.wavefront) fail(PT_ERR_UNSUPPORTED, "this pipeline stages no samples");
    const pt_opts& o = f.o;
    WfFrame wf;
    if (f.wavefront) {
        const QueueEnv qe = queue_env();
        wf = frame_plan(s, f, qe);
        // (a tile-list frame enters no cache: every pointer stays null - what a frame launches when every cache is out of use -
        // and no last_key moves, so the next whole frame still follows its predecessor)
        if (!f.detached()) frame_caches(s, f, wf, stream);
        queue_buffers(s, f, qe, wf);
        stats_slots(s, f, wf);
        lean_frame(s, f, qe, wf);
        side_streams(s, f, wf);
        wf.plan_last = (wf.planned && f.env.plan_skip) ? &wf.fs->plan_last : nullptr;
    }
    Timeline tl{s, f.timing, stream};
    wf.block_empty = camera_cull(s, f, stream);
    RenderParams P = f.P;
    for (uint32_t s0 = f.first_sample(); s0 < f.end_sample(); s0 += f.batch) {
        P.sample_begin = s0;
        P.sample_end = std::min(f.end_sample(), s0 + f.batch);
        const uint32_t nb = P.sample_end - P.sample_begin;
        pt_fastdiv_make(nb, P.div_batch);
        if (!f.wavefront) {
            const uint32_t blocks = f.tm.n_local_tiles * (o.tile_w * o.tile_h / 256u);
            tl.begin(5);
            dispatch([&](auto count) {
                hipLaunchKernelGGL((k_render<count>), dim3(blocks), dim3(256), 0, stream, f.dev, P, f.d_tiles, f.accum, f.gctr);
            }, f.counting);
            HIP_CHECK(hipGetLastError());
            tl.end();
            ++tl.launches;
        } else {
            const uint32_t total_items = f.blocks64 * 64u * nb;
            uint32_t chunk_no = 0;
            for (uint32_t base = 0; base < total_items; base += wf.cap, ++chunk_no)
                render_chunk(s, f, wf, tl, P, stream, base, total_items, chunk_no);
            const dim3 acc_grid(((uint32_t)f.tm.n_local + 255u) / 256u);
            const uint8_t* pixel_empty = wf.block_empty ? (const uint8_t*)(wf.block_empty + f.blocks64 + 1u) : (const uint8_t*)nullptr;
            tl.begin(4);
            if (taps && taps->moments)
                hipLaunchKernelGGL(k_accumulate_moments, acc_grid, dim3(256), 0, stream, (const float*)s.staging_buf.p, f.accum,
                                   taps->moments, (uint32_t)f.tm.n_local, nb, s0 == 0 ? 1 : 0, pixel_empty,
                                   s.dev.background[0], s.dev.background[1], s.dev.background[2]);
            else
                hipLaunchKernelGGL(k_accumulate, acc_grid, dim3(256), 0, stream,
                                   (const float*)s.staging_buf.p, f.accum, (uint32_t)f.tm.n_local, nb, s0 == 0 ? 1 : 0,
                                   pixel_empty, s.dev.background[0], s.dev.background[1], s.dev.background[2]);
            HIP_CHECK(hipGetLastError());
            tl.end();
            if (taps && taps->samples) {
                hipLaunchKernelGGL(k_samples_copy, acc_grid, dim3(256), 0, stream, (const float*)s.staging_buf.p, taps->samples,
                                   (uint32_t)f.tm.n_local, nb, s0, pixel_empty, s.dev.background[0], s.dev.background[1],
                                   s.dev.background[2]);
                HIP_CHECK(hipGetLastError());
            }
        }
        if (allow_preview && o.preview && d_rgb8) {
            // viewer feed (mod.rs:133-141): post_processing(pixel / current_sample) of the samples so far
            hipLaunchKernelGGL(k_postprocess, dim3(((uint32_t)f.tm.n_local + 255u) / 256u), dim3(256), 0, stream, f.accum,
                               (uint8_t*)d_rgb8, (uint32_t)f.tm.n_local, P.sample_end, p.tonemap);
            HIP_CHECK(hipGetLastError());
            std::vector<uint8_t> host(f.tm.n_local * 3);
            HIP_CHECK(hipMemcpyAsync(host.data(), d_rgb8, host.size(), hipMemcpyDeviceToHost, stream));
            HIP_CHECK(hipStreamSynchronize(stream));
            o.preview(host.data(), f.tm.n_local, P.sample_end, p.samples, o.preview_user);
        }
        if (o.progress) {
            HIP_CHECK(hipStreamSynchronize(stream));
            o.progress(P.sample_end, p.samples, o.progress_user);
        }
    }
    frame_readout(s, f, wf, tl, d_rgb8, stream);
}

// The render entry points and pt_scene_escape_copy take the scene as const - the C ABI's promise that rendering changes
// nothing a caller described - but a frame fills the scene's caches (buffers, streams, frame statistics, tile tables) and
// builds its escape masks lazily: the one place the const goes.
pt_scene& render_state(const pt_scene* scene) { return const_cast<pt_scene&>(*scene); }

template <class T>
struct Staged {  // host -> device copy of a test-hook input, freed on scope exit
    T* d = nullptr;
    Staged(const T* host, size_t count) {
        HIP_CHECK(hipMalloc((void**)&d, std::max<size_t>(16, count * sizeof(T))));
        if (host && count) HIP_CHECK(hipMemcpy(d, host, count * sizeof(T), hipMemcpyHostToDevice));
    }
    ~Staged() {
        if (d) (void)hipFree(d);
    }
    void fetch(T* host, size_t count) { HIP_CHECK(hipMemcpy(host, d, count * sizeof(T), hipMemcpyDeviceToHost)); }
};

// ------------------------------------------------------------------ denoised previews (pt_denoise.h)
struct DnScratch {   // the planes of pt_denoise_scratch_bytes, each on a 256-byte boundary
    uint64_t xa, xb, u, g, d, total;
};
DnScratch dn_scratch_layout(uint64_t n) {
    auto up = [](uint64_t v) { return (v + 255u) & ~(uint64_t)255u; };
    DnScratch L;
    L.xa = 0;
    L.xb = L.xa + up(16u * n);
    L.u = L.xb + up(16u * n);
    L.g = L.u + up(16u * n);
    L.d = L.g + up(8u * n);
    L.total = L.d + up(12u * n);
    return L;
}

void dn_check_size(const char* who, uint32_t width, uint32_t height) {
    if (!width || !height) fail(PT_ERR_INVALID, "%s: width * height is 0", who);
    if ((uint64_t)width * height >= (1ull << 31)) fail(PT_ERR_INVALID, "%s: image too large", who);
}

void dn_check_params(const char* who, const pt_denoise_params* p) {
    if (!p) fail(PT_ERR_INVALID, "%s: null parameters", who);
    if (p->iterations > 8u) fail(PT_ERR_INVALID, "%s: iterations %u outside 0..8", who, p->iterations);
    if (p->flags & ~(uint32_t)PT_DENOISE_NO_DEMODULATE) fail(PT_ERR_INVALID, "%s: unknown flags 0x%x", who, p->flags);
    if (p->normal_power_log2 > 10u) fail(PT_ERR_INVALID, "%s: normal_power_log2 %u outside 0..10", who, p->normal_power_log2);
    if (p->tonemap < PT_TONEMAP_REINHARD || p->tonemap > PT_TONEMAP_ACES) fail(PT_ERR_INVALID, "%s: unknown tonemap %d", who, p->tonemap);
    if (!(p->sigma_depth > 0.f) || !std::isfinite(p->sigma_depth)) fail(PT_ERR_INVALID, "%s: sigma_depth must be positive and finite", who);
    if (!(p->sigma_color >= 0.f) || !std::isfinite(p->sigma_color)) fail(PT_ERR_INVALID, "%s: sigma_color must be finite and not negative", who);
}

// The passes of step 1 and 2 gather from an LDS tile with a halo (k_dn_pass<1>, <2>): a fifth faster than global gathers at
// 1080p.  PT_DN_LDS=0: every pass from global memory (A/B measurements; the bits are the same).
bool dn_use_lds() {
    const char* e = getenv("PT_DN_LDS");
    return !(e && *e == '0');
}

// The passes of pt_denoise over prepared planes; on return X holds the last pass's output.  ev: an event after every pass.
void dn_passes(uint32_t width, uint32_t height, const pt_denoise_params& p, float4*& X, float4*& Y, const float4* U, const float2* G,
               hipStream_t stream, hipEvent_t* ev, size_t& e) {
    const dim3 grid((width + DN_TILE_W - 1u) / DN_TILE_W, (height + DN_TILE_H - 1u) / DN_TILE_H);
    const bool lds = dn_use_lds();
    for (uint32_t i = 0; i < p.iterations; ++i) {
        DnParams P;
        P.sigma_depth = p.sigma_depth;
        const float sc = p.sigma_color * (1.0f / (float)(1u << i));
        P.sc2 = sc * sc;
        P.npow = p.normal_power_log2;
        P.color_on = p.sigma_color != 0.f;
        const int step = 1 << i;
        if (lds && i == 0) hipLaunchKernelGGL(k_dn_pass<1>, grid, dim3(256), 0, stream, (const float4*)X, U, G, Y, (int)width, (int)height, step, P);
        else if (lds && i == 1) hipLaunchKernelGGL(k_dn_pass<2>, grid, dim3(256), 0, stream, (const float4*)X, U, G, Y, (int)width, (int)height, step, P);
        else hipLaunchKernelGGL(k_dn_pass<0>, grid, dim3(256), 0, stream, (const float4*)X, U, G, Y, (int)width, (int)height, step, P);
        HIP_CHECK(hipGetLastError());
        if (ev) HIP_CHECK(hipEventRecord(ev[e++], stream));
        std::swap(X, Y);
    }
}

// prep, the passes and finish on `stream`; ev (measurement only): 2 + iterations + 1 events recorded between the stages
void denoise_launch(uint32_t width, uint32_t height, uint32_t samples, const pt_denoise_params& p, const float* d_accum,
                    const float4* d_guides, float* d_out_color, uint8_t* d_out_rgb8, uint8_t* d_scratch, hipStream_t stream,
                    hipEvent_t* ev = nullptr) {
    const uint32_t n = width * height, blocks = (n + 255u) / 256u;
    const uint32_t no_demod = p.flags & PT_DENOISE_NO_DEMODULATE;
    size_t e = 0;
    if (ev) HIP_CHECK(hipEventRecord(ev[e++], stream));
    if (p.iterations == 0) {
        hipLaunchKernelGGL(k_dn_finish, dim3(blocks), dim3(256), 0, stream, (const float4*)nullptr, (const float*)nullptr, d_accum,
                           samples, n, no_demod, p.tonemap, d_out_color, d_out_rgb8);
        HIP_CHECK(hipGetLastError());
        if (ev) HIP_CHECK(hipEventRecord(ev[e++], stream));
        return;
    }
    const DnScratch L = dn_scratch_layout(n);
    float4* X = (float4*)(d_scratch + L.xa);
    float4* Y = (float4*)(d_scratch + L.xb);
    float4* U = (float4*)(d_scratch + L.u);
    float2* G = (float2*)(d_scratch + L.g);
    float* D = (float*)(d_scratch + L.d);
    hipLaunchKernelGGL(k_dn_prep, dim3(blocks), dim3(256), 0, stream, d_accum, d_guides, width, height, samples, no_demod, X, U, G, D);
    HIP_CHECK(hipGetLastError());
    if (ev) HIP_CHECK(hipEventRecord(ev[e++], stream));
    dn_passes(width, height, p, X, Y, U, G, stream, ev, e);
    hipLaunchKernelGGL(k_dn_finish, dim3(blocks), dim3(256), 0, stream, (const float4*)X, (const float*)D, d_accum, samples, n, no_demod,
                       p.tonemap, d_out_color, d_out_rgb8);
    HIP_CHECK(hipGetLastError());
    if (ev) HIP_CHECK(hipEventRecord(ev[e++], stream));
}

// The passes of pt_denoise_var over prepared planes, like dn_passes.
void dnv_passes(uint32_t width, uint32_t height, const pt_denoise_params& p, float4*& X, float4*& Y, const float4* U, const float2* G,
                hipStream_t stream, hipEvent_t* ev, size_t& e) {
    const dim3 grid((width + DN_TILE_W - 1u) / DN_TILE_W, (height + DN_TILE_H - 1u) / DN_TILE_H);
    DnvParams P;
    P.sigma_depth = p.sigma_depth;
    P.sigma_lum = p.sigma_color;
    P.npow = p.normal_power_log2;
    for (uint32_t i = 0; i < p.iterations; ++i) {
        hipLaunchKernelGGL(k_dnv_pass, grid, dim3(256), 0, stream, (const float4*)X, U, G, Y,
                           (int)width, (int)height, 1 << i, P);
        HIP_CHECK(hipGetLastError());
        if (ev) HIP_CHECK(hipEventRecord(ev[e++], stream));
        std::swap(X, Y);
    }
}

// The variance-guided filter (pt_variance.h) on the planes of dn_scratch_layout: X / Y carry (x, v), U carries (u, z).
void denoise_var_launch(uint32_t width, uint32_t height, uint32_t samples, const pt_denoise_params& p, const float* d_accum,
                        const float2* d_moments, const float4* d_guides, float* d_out_color, uint8_t* d_out_rgb8,
                        uint8_t* d_scratch, hipStream_t stream, hipEvent_t* ev = nullptr) {
    const uint32_t n = width * height, blocks = (n + 255u) / 256u;
    const uint32_t no_demod = p.flags & PT_DENOISE_NO_DEMODULATE;
    size_t e = 0;
    if (ev) HIP_CHECK(hipEventRecord(ev[e++], stream));
    if (p.iterations == 0) {
        hipLaunchKernelGGL(k_dn_finish, dim3(blocks), dim3(256), 0, stream, (const float4*)nullptr, (const float*)nullptr, d_accum,
                           samples, n, no_demod, p.tonemap, d_out_color, d_out_rgb8);
        HIP_CHECK(hipGetLastError());
        if (ev) HIP_CHECK(hipEventRecord(ev[e++], stream));
        return;
    }
    const DnScratch L = dn_scratch_layout(n);
    float4* X = (float4*)(d_scratch + L.xa);
    float4* Y = (float4*)(d_scratch + L.xb);
    float4* U = (float4*)(d_scratch + L.u);
    float2* G = (float2*)(d_scratch + L.g);
    float* D = (float*)(d_scratch + L.d);
    hipLaunchKernelGGL(k_dnv_prep, dim3(blocks), dim3(256), 0, stream, d_accum, d_moments, d_guides, width, height, samples,
                       no_demod, X, U, G, D);
    HIP_CHECK(hipGetLastError());
    if (ev) HIP_CHECK(hipEventRecord(ev[e++], stream));
    dnv_passes(width, height, p, X, Y, U, G, stream, ev, e);
    // (an invalid pixel carries v = -1 in X.w: k_dn_finish's validity test)
    hipLaunchKernelGGL(k_dn_finish, dim3(blocks), dim3(256), 0, stream, (const float4*)X, (const float*)D, d_accum, samples, n, no_demod,
                       p.tonemap, d_out_color, d_out_rgb8);
    HIP_CHECK(hipGetLastError());
    if (ev) HIP_CHECK(hipEventRecord(ev[e++], stream));
}

// The argument rules of the pt_denoise_var family beyond dn_check_params.
void dnv_check(const char* who, const pt_denoise_params* p, uint32_t width, uint32_t height, uint32_t samples) {
    dn_check_params(who, p);
    if (!(p->sigma_color > 0.f)) fail(PT_ERR_INVALID, "%s: sigma_color (the luminance sigma) must be positive and finite", who);
    dn_check_size(who, width, height);
    if (samples < 2u) fail(PT_ERR_INVALID, "%s: a sample variance needs samples >= 2 (got %u)", who, samples);
}

// Pipelines that stage no samples have no moments: refused before any device work.
void moments_check_opts(const char* who, const pt_opts* opts) {
    if (opts && (opts->flags & PT_FLAG_MEGAKERNEL)) fail(PT_ERR_UNSUPPORTED, "%s: PT_FLAG_MEGAKERNEL stages no samples", who);
}

void guides_launch(const pt_scene& s, uint32_t width, uint32_t height, float4* d_guides, hipStream_t stream) {
    hipLaunchKernelGGL(k_guides, dim3((width * height + 255u) / 256u), dim3(256), 0, stream, s.dev, width, height, d_guides);
    HIP_CHECK(hipGetLastError());
}

}  // namespace

// ------------------------------------------------------------------ light mixer (pt_lightmix.h)
// The planes of one captured view: plane 0 = E, plane 1 + l = D_l, `stride` floats apart on the device.  cudaMalloc-style
// allocations are 256-byte aligned and the stride is a multiple of 64 floats, so every plane starts on a 256-byte boundary.
struct pt_lightmix {
    int device = 0;
    uint32_t n_lights = 0, samples = 0;
    uint64_t n_local = 0, stride = 0, bytes = 0;
    float* planes = nullptr;
    float unit[PT_LIGHTMIX_MAX_LIGHTS] = {};
    ~pt_lightmix() {
        if (planes) (void)hipFree(planes);
    }
    float* plane(uint32_t i) const { return planes + (uint64_t)i * stride; }
};

namespace {

std::unique_ptr<pt_lightmix> lightmix_alloc(int device, uint32_t n_lights, uint32_t samples, uint64_t n_local) {
    auto m = std::make_unique<pt_lightmix>();
    m->device = device;
    m->n_lights = n_lights;
    m->samples = samples;
    m->n_local = n_local;
    m->stride = (3u * n_local + 63u) & ~(uint64_t)63u;
    m->bytes = (uint64_t)(n_lights + 1u) * m->stride * sizeof(float);
    HIP_CHECK(hipMalloc((void**)&m->planes, m->bytes));
    HIP_CHECK(hipMemset(m->planes, 0, m->bytes));   // (the padding behind every plane stays zero)
    return m;
}

uint32_t lightmix_blocks(uint64_t n4) { return (uint32_t)std::min<uint64_t>((n4 + 255u) / 256u, LM_MAX_BLOCKS); }

// Everything pt_lightmix_apply / _device can refuse, before any device work; the factors f[l][ch] = colors[l][ch] / unit[l].
LmFactors lightmix_factors(const char* who, const pt_lightmix* m, const float* colors, int tonemap_type, const void* rgb8,
                           const void* accum) {
    if (!m || (!colors && m->n_lights) || (!rgb8 && !accum)) fail(PT_ERR_INVALID, "%s: null argument", who);
    if (tonemap_type < PT_TONEMAP_REINHARD || tonemap_type > PT_TONEMAP_ACES) fail(PT_ERR_INVALID, "%s: unknown tonemap %d", who, tonemap_type);
    LmFactors F{};
    for (uint32_t l = 0; l < m->n_lights; ++l)
        for (int ch = 0; ch < 3; ++ch) {
            if (!std::isfinite(colors[3 * l + ch])) fail(PT_ERR_INVALID, "%s: colour %d of light %u is not finite", who, ch, l);
            F.f[l][ch] = colors[3 * l + ch] / m->unit[l];
        }
    return F;
}

void lightmix_launch(const pt_lightmix& m, const LmFactors& F, int tonemap_type, uint8_t* d_rgb8, float* d_accum, hipStream_t stream) {
    const uint64_t n_floats = 3u * m.n_local, n4 = (n_floats + 3u) / 4u;
    hipLaunchKernelGGL(k_lightmix_apply, dim3(lightmix_blocks(n4)), dim3(256), 0, stream, (const float*)m.planes, m.stride, m.n_lights,
                       F, n_floats, m.samples, tonemap_type, d_accum, d_rgb8);
    HIP_CHECK(hipGetLastError());
}

// pt_lightmix_capture.  The scene's lights change colour n_lights + 1 times and get their own colours back on every way
// out (scene_set_light_colors: positions, grids and visibility planes are never touched).
std::unique_ptr<pt_lightmix> lightmix_capture(pt_scene& s, const pt_profile& p, const pt_opts* opts_in) {
    pt_opts o;
    normalise_opts(p, opts_in, o);
    o.progress = nullptr;
    o.preview = nullptr;
    if (p.samples == 0) fail(PT_ERR_INVALID, "pt_lightmix_capture: profile.samples must be > 0");
    const std::vector<DevLight> own = s.host_lights;
    const uint32_t n = (uint32_t)own.size();
    if (n > (uint32_t)PT_LIGHTMIX_MAX_LIGHTS) fail(PT_ERR_UNSUPPORTED, "pt_lightmix_capture: %u lights, at most %d", n, (int)PT_LIGHTMIX_MAX_LIGHTS);
    const uint64_t n_local = make_tile_map(p, o, o.shard_rank).n_local;
    if (n_local == 0) fail(PT_ERR_INVALID, "pt_lightmix_capture: this rank has no pixels");
    float unit[PT_LIGHTMIX_MAX_LIGHTS] = {};
    for (uint32_t l = 0; l < n; ++l) {
        const float* c = own[l].color;
        float m = c[0];
        if (c[1] > m) m = c[1];
        if (c[2] > m) m = c[2];
        if (m == 0.f) m = 1.0f;
        if (!std::isfinite(m)) fail(PT_ERR_INVALID, "pt_lightmix_capture: the colour of light %u is not finite", l);
        unit[l] = m;
    }
    HIP_CHECK(hipSetDevice(s.device));
    auto m = lightmix_alloc(s.device, n, p.samples, n_local);
    memcpy(m->unit, unit, sizeof unit);
    struct Restore {   // the scene's own lights, also when a frame fails (a failing restore cannot be reported twice)
        pt_scene& s;
        const std::vector<DevLight>& own;
        bool armed = true;
        ~Restore() {
            if (!armed) return;
            try {
                scene_set_light_colors(s, own);
            } catch (const GpuError&) {
            }
        }
    } restore{s, own};
    for (uint32_t plane = 0; plane <= n; ++plane) {
        std::vector<DevLight> dl = own;
        for (uint32_t l = 0; l < n; ++l) {
            const float v = (plane == l + 1u) ? unit[l] : 0.f;
            dl[l].color[0] = dl[l].color[1] = dl[l].color[2] = v;
            dl[l].tame = fabsf(v) < 1e30f ? 1u : 0u;   // (dev_light)
        }
        scene_set_light_colors(s, dl);
        render_device(s, p, &o, nullptr, m->plane(plane), nullptr);
    }
    const uint64_t n4 = m->stride / 4u;
    for (uint32_t l = 0; l < n; ++l)
        hipLaunchKernelGGL(k_lightmix_diff, dim3(lightmix_blocks(n4)), dim3(256), 0, 0, (float4*)m->plane(l + 1u), (const float4*)m->plane(0), n4);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipDeviceSynchronize());
    restore.armed = false;
    scene_set_light_colors(s, own);   // (on this way out a failure is reported: no object then)
    return m;
}

}  // namespace

// ------------------------------------------------------------------ progressive film (pt_film.h)
// One allocation: the film's accum and moments, the pass buffers of the same strides, the err plane and the two block
// arrays - each on a 256-byte boundary, every stride a multiple of 64 floats, the padding zero.
struct pt_film {
    int device = 0;
    bool has_profile = false;
    pt_profile profile{};
    pt_opts opts{};
    uint64_t n_local = 0, stride_a = 0, stride_m = 0, stride_e = 0, stride_b = 0, bytes = 0;
    uint32_t n_blocks = 0, passes = 0, last_pass_samples = 0;
    uint64_t samples = 0;
    float* base = nullptr;
    float *accum = nullptr, *moments = nullptr, *pass_accum = nullptr, *pass_moments = nullptr, *err = nullptr;
    float *block_sum = nullptr, *block_max = nullptr;
    // The adaptive film.  A film that has taken a tile pass is non-uniform: `count` (n_local u32, allocated by the
    // first tile pass and filled with the uniform total) holds every pixel's samples, and `samples` is the largest of them.
    // Every pass covers whole tiles of the film's own tiling, so a count per tile on the host says the same: tile_count is what
    // the largest and the smallest count and their sum are read from.  `table`: the tile table of the pass being merged;
    // `tile_sum` / `tile_max`: pt_film_tile_noise's arrays (allocated on first use).  A film that never takes a tile pass and
    // is never asked for its tile noise allocates none of this.
    uint32_t* count = nullptr;
    float* tile_sum = nullptr;   // (tile_max = tile_sum + n_tiles)
    DeviceBuffer table;
    std::vector<uint64_t> tile_count;
    uint64_t bytes_adaptive = 0;
    uint32_t tile_passes = 0, last_pass_tiles = 0;   // (last_pass_tiles: of the last pass; 0: a whole frame, or no pass yet)
    // The film filter: the scratch of pt_film_denoise_scratch_bytes and, behind it, a plane of guides - made by the
    // first host call of the pt_film_denoise family, kept by pt_film_reset.
    uint8_t* filter = nullptr;
    uint64_t bytes_filter = 0;
    // A windowed film (pt_film_create_windowed): every pass is a window of ONE enumeration of enum_n samples per
    // pixel, so a pixel at count c holds the sums of the samples [0, c) of pt_render(samples = enum_n).
    bool windowed = false;
    uint32_t enum_n = 0, windows = 0, tile_windows = 0;
    // A shard film (pt_film_create_shard): this rank's tiles of a film that opts.shard_count ranks hold together.
    // tile_count, samples and the pass counters are the WHOLE film's (tile lists are global); the planes hold the own tiles.
    // packed (shard_count > 1): the planes are in packed tile order and the FilmPacked kernels run; base_of[k] is the first
    // packed pixel of tile k (FILM_NOT_OWNED: another rank's), base_dev the same on the device.  A one-rank shard film is in
    // image order, like every unsharded film.
    bool shard = false, packed = false;
    std::vector<uint32_t> base_of;
    DeviceBuffer base_dev;
    bool uniform() const { return count == nullptr; }
    bool owns(uint32_t tile) const { return !packed || base_of[tile] != FILM_NOT_OWNED; }
    ~pt_film() {
        if (filter) (void)hipFree(filter);
        if (base) (void)hipFree(base);
        if (count) (void)hipFree(count);
        if (tile_sum) (void)hipFree(tile_sum);
    }
};

namespace {

std::unique_ptr<pt_film> film_alloc(int device, uint64_t n_local) {
    auto up = [](uint64_t floats) { return (floats + 63u) & ~(uint64_t)63u; };
    auto f = std::make_unique<pt_film>();
    f->device = device;
    f->n_local = n_local;
    f->n_blocks = (uint32_t)((n_local + 255u) / 256u);
    f->stride_a = up(3u * n_local);
    f->stride_m = up(2u * n_local);
    f->stride_e = up(n_local);
    f->stride_b = up(f->n_blocks);
    const uint64_t floats = 2u * (f->stride_a + f->stride_m) + f->stride_e + 2u * f->stride_b;
    f->bytes = floats * sizeof(float);
    HIP_CHECK(hipMalloc((void**)&f->base, f->bytes));
    HIP_CHECK(hipMemset(f->base, 0, f->bytes));   // (the padding behind every plane stays zero)
    float* p = f->base;
    f->accum = p, p += f->stride_a;
    f->moments = p, p += f->stride_m;
    f->pass_accum = p, p += f->stride_a;
    f->pass_moments = p, p += f->stride_m;
    f->err = p, p += f->stride_e;
    f->block_sum = p, p += f->stride_b;
    f->block_max = p;
    return f;
}

uint32_t film_merge_blocks(const pt_film& f) {
    return (uint32_t)std::min<uint64_t>((std::max(f.stride_a, f.stride_m) / 4u + 255u) / 256u, FILM_MAX_BLOCKS);
}

void film_check_noise_args(const char* who, float lum_floor, double target) {
    if (!(lum_floor > 0.f) || !std::isfinite(lum_floor)) fail(PT_ERR_INVALID, "%s: lum_floor must be positive and finite", who);
    if (!(target >= 0.0) || !std::isfinite(target)) fail(PT_ERR_INVALID, "%s: target must be finite and not negative", who);
}

// What pt_film_add_pass and pt_film_add_planes refuse, before any device work.
void film_check_samples(const char* who, const pt_film* film, uint32_t samples) {
    if (film->windowed) fail(PT_ERR_INVALID, "%s: a windowed film takes windows only (pt_film_add_window)", who);
    if (samples < 1u) fail(PT_ERR_INVALID, "%s: a pass needs samples >= 1", who);
    if (film->passes && (uint64_t)samples < 2u * (uint64_t)film->last_pass_samples)
        fail(PT_ERR_INVALID, "%s: a pass of %u samples after one of %u (at least twice as many: an equal pass would repeat its seeds)",
             who, samples, film->last_pass_samples);
    if (film->samples + samples > (uint64_t)PT_FILM_MAX_SAMPLES)
        fail(PT_ERR_INVALID, "%s: %llu samples in all, at most %u", who, (unsigned long long)(film->samples + samples),
             (unsigned)PT_FILM_MAX_SAMPLES);
}
void film_check_pass(const char* who, const pt_film* film, const pt_scene* scene, uint32_t samples) {
    if (!film || !scene) fail(PT_ERR_INVALID, "%s: null argument", who);
    if (!film->has_profile) fail(PT_ERR_INVALID, "%s: a film made from planes has no profile to render with", who);
    film_check_samples(who, film, samples);
    if (scene->device != film->device)
        fail(PT_ERR_INVALID, "%s: the scene is on device %d, the film on device %d", who, scene->device, film->device);
}

// film = film + pass buffers, then the counters
void film_merge(pt_film& film, uint32_t samples) {
    hipLaunchKernelGGL(k_film_merge, dim3(film_merge_blocks(film)), dim3(256), 0, 0, (float4*)film.accum,
                       (const float4*)film.pass_accum, film.stride_a / 4u, (float4*)film.moments,
                       (const float4*)film.pass_moments, film.stride_m / 4u);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipDeviceSynchronize());
    ++film.passes;
    film.last_pass_samples = samples;
    film.last_pass_tiles = 0;
    film.samples += samples;
}

void film_add_pass(pt_film& film, const pt_scene* scene, uint32_t samples) {
    film_check_pass("pt_film_add_pass", &film, scene, samples);
    HIP_CHECK(hipSetDevice(film.device));
    pt_profile p = film.profile;
    p.samples = samples;
    FrameTaps taps;
    taps.moments = (float2*)film.pass_moments;
    render_device(render_state(scene), p, &film.opts, nullptr, film.pass_accum, nullptr, false, &taps);
    HIP_CHECK(hipDeviceSynchronize());   // the frame is complete (and has not failed) before the film changes
    film_merge(film, samples);
}

void film_noise_launch(const pt_film& film, float lum_floor, bool with_err) {
    hipLaunchKernelGGL(k_film_noise, dim3(film.n_blocks), dim3(256), 0, 0, (const float2*)film.moments, (uint32_t)film.n_local,
                       (uint32_t)film.samples, lum_floor, with_err ? film.err : (float*)nullptr, film.block_sum, film.block_max);
    HIP_CHECK(hipGetLastError());
}

void film_noise(const pt_film& film, float lum_floor, double target, pt_film_noise_stats& out, float* err_host,
                float* block_sum_host, float* block_max_host) {
    film_check_noise_args("pt_film_noise", lum_floor, target);
    if (film.samples < 2u) fail(PT_ERR_INVALID, "pt_film_noise: a sample variance needs a total of >= 2 samples (got %llu)", (unsigned long long)film.samples);
    HIP_CHECK(hipSetDevice(film.device));
    film_noise_launch(film, lum_floor, err_host != nullptr);
    std::vector<float> sums(film.n_blocks);
    HIP_CHECK(hipMemcpy(sums.data(), film.block_sum, film.n_blocks * sizeof(float), hipMemcpyDeviceToHost));   // (waits for the kernel)
    if (block_sum_host) memcpy(block_sum_host, sums.data(), film.n_blocks * sizeof(float));
    if (block_max_host) HIP_CHECK(hipMemcpy(block_max_host, film.block_max, film.n_blocks * sizeof(float), hipMemcpyDeviceToHost));
    if (err_host) HIP_CHECK(hipMemcpy(err_host, film.err, film.n_local * sizeof(float), hipMemcpyDeviceToHost));
    double S = 0.0, worst = 0.0;
    uint32_t over = 0;
    for (uint32_t b = 0; b < film.n_blocks; ++b) {
        const uint64_t pixels = std::min<uint64_t>(256u, film.n_local - 256ull * b);
        const double mean_b = (double)sums[b] / (double)pixels;
        S = S + (double)sums[b];
        if (b == 0 || mean_b > worst) worst = mean_b;
        if (mean_b > target) ++over;
    }
    out.mean_error = S / (double)film.n_local;
    out.max_block_error = worst;
    out.fraction_over = (double)over / (double)film.n_blocks;
    out.samples = film.samples;
    out.n_blocks = film.n_blocks;
    out.converged = out.mean_error <= target ? 1u : 0u;
}

// ---- the adaptive film
FilmTiling film_tiling(const pt_film& film) {
    return FilmTiling{film.profile.width, film.profile.height, film.opts.tile_w, film.opts.tile_h,
                      (film.profile.width + film.opts.tile_w - 1u) / film.opts.tile_w};
}
uint32_t film_n_tiles(const pt_film& film) {
    const FilmTiling T = film_tiling(film);
    return T.tiles_x * ((T.height + T.tile_h - 1u) / T.tile_h);
}
uint64_t film_tile_pixels(const FilmTiling& T, uint32_t k) {
    const uint32_t x0 = (k % T.tiles_x) * T.tile_w, y0 = (k / T.tiles_x) * T.tile_h;
    return (uint64_t)std::min(T.tile_w, T.width - x0) * std::min(T.tile_h, T.height - y0);
}
void film_check_tiled(const char* who, const pt_film* film) {
    if (!film) fail(PT_ERR_INVALID, "%s: null argument", who);
    if (!film->has_profile) fail(PT_ERR_INVALID, "%s: a film made from planes has no tiling", who);
    if (film->opts.shard_count > 1 && !film->shard) fail(PT_ERR_INVALID, "%s: a sharded film takes whole passes only (shard_count %u)", who, film->opts.shard_count);
}
// The calls whose figures are defined over one device's planes
void film_refuse_shard(const char* who, const pt_film* film) {
    if (film && film->shard) fail(PT_ERR_INVALID, "%s: a shard film holds a part of the image (pt_film_assemble makes the whole film)", who);
}
void film_check_shard(const char* who, const pt_film* film) {
    if (!film) fail(PT_ERR_INVALID, "%s: null argument", who);
    if (!film->shard) fail(PT_ERR_INVALID, "%s: the film is not a shard film (pt_film_create_shard)", who);
}
// The options of a film's tile-list frames and tile lists: a shard film's lists are global, its own tiles render unsharded
pt_opts film_list_opts(const pt_film& film) {
    pt_opts o = film.opts;
    o.shard_rank = 0;
    o.shard_count = 1;
    return o;
}
FilmPacked film_packed(const pt_film& film) { return FilmPacked{film_tiling(film), (const uint32_t*)film.base_dev.p}; }
// The listed tiles this film holds, in list order: the list itself unless the film is packed
std::vector<uint32_t> film_own_tiles(const pt_film& film, const std::vector<uint32_t>& tiles) {
    if (!film.packed) return tiles;
    std::vector<uint32_t> own;
    for (uint32_t k : tiles)
        if (film.owns(k)) own.push_back(k);
    return own;
}
std::vector<uint32_t> film_all_tiles(const pt_film& film) {
    std::vector<uint32_t> all(film_n_tiles(film));
    for (uint32_t k = 0; k < all.size(); ++k) all[k] = k;
    return all;
}
// The tile map of the own tiles of a list (no tile: an empty map, nothing to launch)
TileMap film_own_map(const char* who, const pt_film& film, const std::vector<uint32_t>& own) {
    if (own.empty()) {
        TileMap m{};
        m.offsets.push_back(0u);
        return m;
    }
    return make_tile_list_map(who, film.profile, film_list_opts(film), own.data(), (uint32_t)own.size());
}
void film_upload_table(pt_film& film, const TileMap& tm) {
    std::vector<uint32_t> table(tm.offsets);
    table.insert(table.end(), tm.tiles.begin(), tm.tiles.end());
    HIP_CHECK(hipMemcpy(film.table.p, table.data(), table.size() * 4u, hipMemcpyHostToDevice));
}
// The four tile kernels on the film's layout.  n_list: the tiles of the uploaded table (> 0).
void film_launch_merge_tiles(const pt_film& film, uint32_t n_list, const float* pa, const float* pm, uint32_t samples) {
    if (film.packed)
        hipLaunchKernelGGL(k_film_merge_tiles_packed, dim3(n_list), dim3(256), 0, 0, pa, (const float2*)pm, (const uint32_t*)film.table.p,
                           n_list, film_packed(film), film.accum, (float2*)film.moments, film.count, samples);
    else
        hipLaunchKernelGGL(k_film_merge_tiles, dim3(n_list), dim3(256), 0, 0, pa, (const float2*)pm, (const uint32_t*)film.table.p, n_list,
                           film_tiling(film), film.accum, (float2*)film.moments, film.count, samples);
}
void film_launch_gather_tiles(const pt_film& film, uint32_t n_list, float* pa, float* pm) {
    if (film.packed)
        hipLaunchKernelGGL(k_film_gather_tiles_packed, dim3(n_list), dim3(256), 0, 0, (const float*)film.accum, (const float2*)film.moments,
                           (const uint32_t*)film.table.p, n_list, film_packed(film), pa, (float2*)pm);
    else
        hipLaunchKernelGGL(k_film_gather_tiles, dim3(n_list), dim3(256), 0, 0, (const float*)film.accum, (const float2*)film.moments,
                           (const uint32_t*)film.table.p, n_list, film_tiling(film), pa, (float2*)pm);
}
void film_launch_scatter_tiles(const pt_film& film, uint32_t n_list, const float* pa, const float* pm, uint32_t samples) {
    if (film.packed)
        hipLaunchKernelGGL(k_film_scatter_tiles_packed, dim3(n_list), dim3(256), 0, 0, pa, (const float2*)pm, (const uint32_t*)film.table.p,
                           n_list, film_packed(film), film.accum, (float2*)film.moments, film.count, samples);
    else
        hipLaunchKernelGGL(k_film_scatter_tiles, dim3(n_list), dim3(256), 0, 0, pa, (const float2*)pm, (const uint32_t*)film.table.p,
                           n_list, film_tiling(film), film.accum, (float2*)film.moments, film.count, samples);
}
// One workgroup per tile of the IMAGE, on either layout
void film_launch_tile_noise(const pt_film& film, float lum_floor, float* err, float* tile_sum, float* tile_max) {
    const uint32_t n_tiles = film_n_tiles(film);
    if (film.packed)
        hipLaunchKernelGGL(k_film_tile_noise_packed, dim3(n_tiles), dim3(256), 0, 0, (const float2*)film.moments,
                           (const uint32_t*)film.count, (uint32_t)film.samples, film_packed(film), lum_floor, err, tile_sum, tile_max);
    else
        hipLaunchKernelGGL(k_film_tile_noise, dim3(n_tiles), dim3(256), 0, 0, (const float2*)film.moments, (const uint32_t*)film.count,
                           (uint32_t)film.samples, film_tiling(film), lum_floor, err, tile_sum, tile_max);
}
void film_refuse_non_uniform(const char* who, const pt_film* film) {
    if (film && !film->uniform()) fail(PT_ERR_UNSUPPORTED, "%s: the film has a sample count per pixel (pt_film_add_tile_pass); this call assumes one", who);
}
// What a tile pass refuses before any device work; returns the list's tile map.
TileMap film_check_tile_pass(const char* who, const pt_film* film, uint32_t samples, const uint32_t* tiles, uint32_t n_tiles) {
    film_check_tiled(who, film);
    film_check_samples(who, film, samples);
    return make_tile_list_map(who, film->profile, film_list_opts(*film), tiles, n_tiles);
}
// The first tile pass: the count plane, filled with the uniform total; the table's buffer
void film_make_non_uniform(pt_film& film) {
    if (!film.uniform()) return;
    const uint32_t n_tiles = film_n_tiles(film);
    const size_t table_before = film.table.bytes;   // (the table's buffer outlives a pt_film_reset)
    film.table.ensure((size_t)(2u * n_tiles + 1u) * 4u);
    film.bytes_adaptive += film.table.bytes - table_before;
    std::vector<uint32_t> fill((size_t)film.n_local, (uint32_t)film.samples);
    uint32_t* d = nullptr;
    HIP_CHECK(hipMalloc((void**)&d, (size_t)film.n_local * 4u));   // (256-byte aligned, as every hipMalloc)
    if (hipMemcpy(d, fill.data(), fill.size() * 4u, hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipFree(d);
        fail(PT_ERR_DEVICE, "pt_film: the copy of the count plane failed");
    }
    film.count = d;
    film.tile_count.assign(n_tiles, film.samples);
    film.bytes_adaptive += (uint64_t)film.n_local * 4u;
}
// film = film + pass buffers over the tiles of tm - the listed tiles the film holds, which the pass buffers are packed by - then
// the counters, which follow the whole list
void film_merge_tiles(pt_film& film, const TileMap& tm, const std::vector<uint32_t>& listed, uint32_t samples) {
    film_make_non_uniform(film);
    if (tm.n_local_tiles) {   // (a shard film that holds none of the list: the pass happened elsewhere)
        film_upload_table(film, tm);
        film_launch_merge_tiles(film, tm.n_local_tiles, film.pass_accum, film.pass_moments, samples);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipDeviceSynchronize());
    }
    ++film.passes;
    ++film.tile_passes;
    film.last_pass_tiles = (uint32_t)listed.size();
    film.last_pass_samples = samples;
    for (uint32_t k : listed) film.tile_count[k] += samples;
    film.samples = *std::max_element(film.tile_count.begin(), film.tile_count.end());
}
void film_add_tile_pass(pt_film& film, const pt_scene* scene, uint32_t samples, const uint32_t* tiles, uint32_t n_tiles) {
    const char* who = "pt_film_add_tile_pass";
    if (!scene) fail(PT_ERR_INVALID, "%s: null argument", who);
    const TileMap listed = film_check_tile_pass(who, &film, samples, tiles, n_tiles);
    if (scene->device != film.device)
        fail(PT_ERR_INVALID, "%s: the scene is on device %d, the film on device %d", who, scene->device, film.device);
    HIP_CHECK(hipSetDevice(film.device));
    // a shard film renders the listed tiles it holds, as an unsharded tile-list frame: the pass buffers come in list order, which
    // is the film's own order for those tiles
    const std::vector<uint32_t> own = film_own_tiles(film, listed.tiles);
    const TileMap tm = film.packed ? film_own_map(who, film, own) : listed;
    if (!own.empty()) {
        pt_profile p = film.profile;
        p.samples = samples;
        FrameTaps taps;
        taps.moments = (float2*)film.pass_moments;
        const TileList list{own.data(), (uint32_t)own.size()};
        const pt_opts o = film_list_opts(film);
        render_device(render_state(scene), p, &o, nullptr, film.pass_accum, nullptr, false, &taps, &list);
        HIP_CHECK(hipDeviceSynchronize());   // the frame is complete (and has not failed) before the film changes
    }
    film_merge_tiles(film, tm, listed.tiles, samples);
}
// A whole frame on any film: a non-uniform one takes it as the tile pass that lists every tile
void film_add_whole_pass(pt_film& film, const pt_scene* scene, uint32_t samples) {
    if (film.uniform()) return film_add_pass(film, scene, samples);
    film_check_pass("pt_film_add_pass", &film, scene, samples);
    const std::vector<uint32_t> all = film_all_tiles(film);
    film_add_tile_pass(film, scene, samples, all.data(), (uint32_t)all.size());
}

// The host step of pt_film_tile_noise: the statistics, in f64, of one tile sum per tile of the film.
void film_tile_stats(const pt_film& film, const std::vector<float>& sums, double target, pt_film_tile_stats& out) {
    const uint64_t n_pixels = (uint64_t)film.profile.width * film.profile.height;   // (n_local of an unsharded film; a shard film: the whole film's)
    const FilmTiling T = film_tiling(film);
    const uint32_t n_tiles = (uint32_t)sums.size();
    double S = 0.0, worst = 0.0;
    uint32_t over = 0;
    uint64_t pixel_samples = 0;
    for (uint32_t t = 0; t < n_tiles; ++t) {
        const uint64_t pixels = film_tile_pixels(T, t);
        const double mean_t = (double)sums[t] / (double)pixels;
        S = S + (double)sums[t];
        if (t == 0 || mean_t > worst) worst = mean_t;
        if (mean_t > target) ++over;
        pixel_samples += pixels * (film.uniform() ? film.samples : film.tile_count[t]);
    }
    memset(&out, 0, sizeof out);
    out.mean_error = S / (double)n_pixels;
    out.max_tile_error = worst;
    out.samples = film.samples;
    out.pixel_samples = pixel_samples;
    out.n_tiles = n_tiles;
    out.over_tiles = over;
    out.converged = over == 0u ? 1u : 0u;
}

void film_tile_noise(const pt_film& film_c, float lum_floor, double target, pt_film_tile_stats& out, float* err_host,
                     float* tile_sum_host, float* tile_max_host) {
    const char* who = "pt_film_tile_noise";
    film_check_tiled(who, &film_c);
    film_refuse_shard(who, &film_c);
    film_check_noise_args(who, lum_floor, target);
    pt_film& film = const_cast<pt_film&>(film_c);   // (the tile arrays are made on first use: scratch, not the film's contents)
    const uint32_t n_tiles = film_n_tiles(film);
    const uint64_t least = film.uniform() ? film.samples : *std::min_element(film.tile_count.begin(), film.tile_count.end());
    if (least < 2u) fail(PT_ERR_INVALID, "%s: a sample variance needs >= 2 samples in every pixel (the fewest: %llu)", who, (unsigned long long)least);
    HIP_CHECK(hipSetDevice(film.device));
    if (!film.tile_sum) {
        HIP_CHECK(hipMalloc((void**)&film.tile_sum, (size_t)n_tiles * 8u));
        film.bytes_adaptive += (uint64_t)n_tiles * 8u;
    }
    float* tile_max = film.tile_sum + n_tiles;
    const FilmTiling T = film_tiling(film);
    hipLaunchKernelGGL(k_film_tile_noise, dim3(n_tiles), dim3(256), 0, 0, (const float2*)film.moments, (const uint32_t*)film.count,
                       (uint32_t)film.samples, T, lum_floor, err_host ? film.err : (float*)nullptr, film.tile_sum, tile_max);
    HIP_CHECK(hipGetLastError());
    std::vector<float> sums(n_tiles);
    HIP_CHECK(hipMemcpy(sums.data(), film.tile_sum, n_tiles * sizeof(float), hipMemcpyDeviceToHost));   // (waits for the kernel)
    if (tile_sum_host) memcpy(tile_sum_host, sums.data(), n_tiles * sizeof(float));
    if (tile_max_host) HIP_CHECK(hipMemcpy(tile_max_host, tile_max, n_tiles * sizeof(float), hipMemcpyDeviceToHost));
    if (err_host) HIP_CHECK(hipMemcpy(err_host, film.err, film.n_local * sizeof(float), hipMemcpyDeviceToHost));
    film_tile_stats(film, sums, target, out);
}

void film_fill_info(const pt_film& film, pt_film_info& info) {
    memset(&info, 0, sizeof info);
    info.width = film.has_profile ? film.profile.width : 0u;
    info.height = film.has_profile ? film.profile.height : 0u;
    info.passes = film.passes;
    info.last_pass_samples = film.last_pass_samples;
    info.n_local = film.n_local;
    info.samples = film.samples;
    info.device_bytes = film.bytes + film.bytes_adaptive + film.bytes_filter;
}

void film_check_resolve(const char* who, const pt_film* film, int tonemap_type, const void* rgb8, const void* color) {
    if (!film || (!rgb8 && !color)) fail(PT_ERR_INVALID, "%s: null argument", who);
    if (tonemap_type < PT_TONEMAP_REINHARD || tonemap_type > PT_TONEMAP_ACES) fail(PT_ERR_INVALID, "%s: unknown tonemap %d", who, tonemap_type);
    if (film->samples == 0) fail(PT_ERR_INVALID, "%s: the film holds no samples", who);
    if (!film->uniform() && *std::min_element(film->tile_count.begin(), film->tile_count.end()) == 0)
        fail(PT_ERR_INVALID, "%s: some tiles of the film hold no samples", who);
}

// The planes the resolve and the film filter read: a film's, or a temporal history's.  count == nullptr: every
// pixel has `samples` samples.  width and height are the filter's (a film made from planes has neither).
struct FilmPlanes {
    const float* accum;
    const float* moments;
    const uint32_t* count;
    uint32_t samples, width, height;
    uint64_t n;
};
FilmPlanes film_planes(const pt_film& film) {
    return {film.accum, film.moments, film.count, (uint32_t)film.samples, film.has_profile ? film.profile.width : 0u,
            film.has_profile ? film.profile.height : 0u, film.n_local};
}

void film_resolve_launch(const FilmPlanes& film, int tonemap_type, uint8_t* d_rgb8, float* d_color, hipStream_t stream) {
    const uint64_t n_floats = 3u * film.n;
    if (film.count != nullptr) {   // every pixel by its own count
        if (d_color) {
            const uint32_t blocks = (uint32_t)std::min<uint64_t>((n_floats + 255u) / 256u, FILM_MAX_BLOCKS);
            hipLaunchKernelGGL(k_film_color_counts, dim3(blocks), dim3(256), 0, stream, film.accum, film.count, d_color, n_floats);
        }
        if (d_rgb8)
            hipLaunchKernelGGL(k_film_post_counts, dim3(((uint32_t)film.n + 255u) / 256u), dim3(256), 0, stream, film.accum, film.count,
                               d_rgb8, (uint32_t)film.n, tonemap_type);
        HIP_CHECK(hipGetLastError());
        return;
    }
    if (d_color) {
        const uint32_t blocks = (uint32_t)std::min<uint64_t>((n_floats + 255u) / 256u, FILM_MAX_BLOCKS);
        hipLaunchKernelGGL(k_film_color, dim3(blocks), dim3(256), 0, stream, film.accum, d_color, n_floats, (float)film.samples);
    }
    if (d_rgb8)
        hipLaunchKernelGGL(k_postprocess, dim3(((uint32_t)film.n + 255u) / 256u), dim3(256), 0, stream, film.accum, d_rgb8,
                           (uint32_t)film.n, film.samples, tonemap_type);
    HIP_CHECK(hipGetLastError());
}
void film_resolve_launch(const pt_film& film, int tonemap_type, uint8_t* d_rgb8, float* d_color, hipStream_t stream) {
    film_resolve_launch(film_planes(film), tonemap_type, d_rgb8, d_color, stream);
}

// What the adaptive loops refuse before any device work (the null checks are the callers').
void film_check_adaptive(const char* who, const pt_film* film, const pt_scene* scene, const pt_film_adaptive_params* params) {
    film_check_tiled(who, film);
    if (film->windowed) fail(PT_ERR_INVALID, "%s: a windowed film takes windows only (pt_film_render_until_windowed)", who);
    film_check_noise_args(who, params->lum_floor, params->target);
    if (params->first_pass_samples < 2u) fail(PT_ERR_INVALID, "%s: first_pass_samples must be >= 2 (a sample variance needs two)", who);
    if (params->dilate > 1u) fail(PT_ERR_INVALID, "%s: dilate must be 0 or 1", who);
    if (!film->passes && (uint64_t)params->first_pass_samples > params->max_samples)
        fail(PT_ERR_INVALID, "%s: first_pass_samples %u exceeds max_samples %llu", who, params->first_pass_samples, (unsigned long long)params->max_samples);
    if (scene->device != film->device)
        fail(PT_ERR_INVALID, "%s: the scene is on device %d, the film on device %d", who, scene->device, film->device);
}

// Steps 5 and 6 of the adaptive loops: the candidates - the tiles whose mean error is above the target - and, dilate: their 8
// neighbours, ascending.
void film_select_active(const FilmTiling& T, const std::vector<float>& sums, double target, uint32_t dilate, std::vector<uint32_t>& active) {
    const uint32_t n_tiles = (uint32_t)sums.size(), tiles_y = n_tiles / T.tiles_x;
    std::vector<uint8_t> on(n_tiles, 0);
    for (uint32_t t = 0; t < n_tiles; ++t) {
        if (!((double)sums[t] / (double)film_tile_pixels(T, t) > target)) continue;
        const int tx = (int)(t % T.tiles_x), ty = (int)(t / T.tiles_x), r = (int)dilate;
        for (int y = std::max(0, ty - r); y <= std::min((int)tiles_y - 1, ty + r); ++y)
            for (int x = std::max(0, tx - r); x <= std::min((int)T.tiles_x - 1, tx + r); ++x) on[(uint32_t)y * T.tiles_x + (uint32_t)x] = 1;
    }
    active.clear();
    for (uint32_t t = 0; t < n_tiles; ++t)
        if (on[t]) active.push_back(t);
}

// The loop of pt_film_render_until_adaptive (include/ptgpu.h, steps 1 - 8).  noise(st, sums): step 4 - the tile statistics of
// what the film holds and, where sums is not null, the n_tiles tile sums the selection reads.
template <class Noise>
void film_adaptive_loop(pt_film* film, const pt_scene* scene, const pt_film_adaptive_params* params, pt_film_pass_fn on_pass,
                        void* user, pt_film_tile_stats* out, Noise noise) {
    const uint64_t cap = std::min<uint64_t>(params->max_samples, (uint64_t)PT_FILM_MAX_SAMPLES);
    const FilmTiling T = film_tiling(*film);
    const uint32_t n_tiles = film_n_tiles(*film);
    std::vector<float> sums(n_tiles);
    std::vector<uint32_t> active;   // the tiles of the next pass; empty: every tile
    pt_film_tile_stats st{};
    bool measured = false;
    auto measure = [&](uint32_t rendered) {
        noise(st, sums.data());
        st.active_tiles = rendered;
        measured = true;
        film_select_active(T, sums, params->target, params->dilate, active);
    };
    if (film->passes && film->samples >= 2u && film->samples >= params->uniform_samples) measure(0);   // (a film that has passes: its own active set)
    for (;;) {
        if (measured && st.converged) break;
        const uint64_t next = film->passes ? 2u * (uint64_t)film->last_pass_samples : (uint64_t)params->first_pass_samples;
        if (film->samples + next > cap) break;
        const bool all = !measured || !film->passes || film->samples < params->uniform_samples || active.size() == n_tiles;
        if (all) film_add_whole_pass(*film, scene, (uint32_t)next);
        else film_add_tile_pass(*film, scene, (uint32_t)next, active.data(), (uint32_t)active.size());
        measure(all ? n_tiles : (uint32_t)active.size());
        if (on_pass) {
            pt_film_info info;
            film_fill_info(*film, info);
            pt_film_noise_stats ns{};
            ns.mean_error = st.mean_error;
            ns.max_block_error = st.max_tile_error;
            ns.fraction_over = (double)st.over_tiles / (double)n_tiles;
            ns.samples = st.samples;
            ns.n_blocks = n_tiles;
            ns.converged = st.converged;
            on_pass(&info, &ns, user);
        }
    }
    if (!measured) noise(st, nullptr);   // (no pass fits: what the film holds)
    *out = st;
}

// ---- windowed films (pt_film_window.h)
uint64_t film_count_of(const pt_film& film, uint32_t tile) { return film.uniform() ? film.samples : film.tile_count[tile]; }

// What the window calls refuse before any device work.
void film_check_window(const char* who, const pt_film* film, const pt_scene* scene, uint32_t samples) {
    if (!film || !scene) fail(PT_ERR_INVALID, "%s: null argument", who);
    if (!film->windowed) fail(PT_ERR_INVALID, "%s: the film is not windowed (pt_film_create_windowed)", who);
    if (samples < 1u) fail(PT_ERR_INVALID, "%s: a window needs samples >= 1", who);
    if (scene->device != film->device)
        fail(PT_ERR_INVALID, "%s: the scene is on device %d, the film on device %d", who, scene->device, film->device);
}

// The frame's moments tap and the window [s0, s0 + samples) of the film's enumeration, rendered into (d_accum, d_moments) -
// packed in list order where list is not null - which hold the sums of [0, s0).  Waits for the frame.
void film_render_window(pt_film& film, const pt_scene* scene, uint32_t s0, uint32_t samples, const TileList* list, float* d_accum,
                        float* d_moments) {
    pt_profile p = film.profile;
    p.samples = film.enum_n;
    FrameTaps taps;
    taps.moments = (float2*)d_moments;
    const SampleWindow win{s0, s0 + samples};
    const pt_opts o = list ? film_list_opts(film) : film.opts;
    render_device(render_state(scene), p, &o, nullptr, d_accum, nullptr, false, &taps, list, &win);
    HIP_CHECK(hipDeviceSynchronize());   // the frame is complete (and has not failed) before the film changes
}

// The tile window: every listed tile t continues at its own count.  The tiles are grouped by count, counts ascending; group g
// is gathered to its own run of the pass buffers and rendered there as one tile-list window frame.  Only when every frame has
// completed are the runs scattered back - a failure before that leaves the film as it was.
void film_add_tile_window(pt_film& film, const pt_scene* scene, uint32_t samples, const uint32_t* tiles, uint32_t n_tiles) {
    const char* who = "pt_film_add_tile_window";
    film_check_window(who, &film, scene, samples);
    film_check_tiled(who, &film);
    const pt_opts list_opts = film_list_opts(film);
    const TileMap whole = make_tile_list_map(who, film.profile, list_opts, tiles, n_tiles);
    std::map<uint64_t, std::vector<uint32_t>> groups;   // count -> its tiles (a shard film: the ones it holds), ascending both ways
    for (uint32_t k : whole.tiles) {
        const uint64_t c = film_count_of(film, k);
        if (c + samples > film.enum_n)
            fail(PT_ERR_INVALID, "%s: tile %u holds %llu samples, %u more would pass the enumeration's %u", who, k, (unsigned long long)c, samples, film.enum_n);
        if (film.owns(k)) groups[c].push_back(k);
    }
    HIP_CHECK(hipSetDevice(film.device));
    const size_t table_before = film.table.bytes;
    film.table.ensure((size_t)(2u * film_n_tiles(film) + 1u) * 4u);
    film.bytes_adaptive += film.table.bytes - table_before;
    struct Run {
        TileMap tm;
        uint64_t off;   // the run's first packed pixel in the pass buffers
    };
    std::vector<Run> runs;
    uint64_t off = 0;
    auto upload = [&](const TileMap& tm) { film_upload_table(film, tm); };
    for (auto& g : groups) {
        Run r{make_tile_list_map(who, film.profile, list_opts, g.second.data(), (uint32_t)g.second.size()), off};
        float* pa = film.pass_accum + 3u * r.off;
        float* pm = film.pass_moments + 2u * r.off;
        upload(r.tm);
        film_launch_gather_tiles(film, r.tm.n_local_tiles, pa, pm);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipDeviceSynchronize());   // (the table is rewritten by the next run)
        const TileList list{g.second.data(), (uint32_t)g.second.size()};
        film_render_window(film, scene, (uint32_t)g.first, samples, &list, pa, pm);
        off += r.tm.n_local;
        runs.push_back(std::move(r));
    }
    film_make_non_uniform(film);
    for (const Run& r : runs) {
        upload(r.tm);
        film_launch_scatter_tiles(film, r.tm.n_local_tiles, film.pass_accum + 3u * r.off, film.pass_moments + 2u * r.off, samples);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipDeviceSynchronize());
        for (uint32_t k : r.tm.tiles) film.tile_count[k] += samples;
    }
    for (uint32_t k : whole.tiles)   // (a shard film: the windows that other ranks render)
        if (!film.owns(k)) film.tile_count[k] += samples;
    ++film.passes;
    ++film.tile_passes;
    ++film.tile_windows;
    film.last_pass_tiles = n_tiles;
    film.last_pass_samples = samples;
    film.samples = *std::max_element(film.tile_count.begin(), film.tile_count.end());
}

// The whole-frame window [n, n + samples) of every pixel.  A uniform film renders it into the pass buffers, seeded with a
// copy of the film, and adopts them on success; a non-uniform one takes the tile window that lists every tile.
void film_add_window(pt_film& film, const pt_scene* scene, uint32_t samples) {
    const char* who = "pt_film_add_window";
    film_check_window(who, &film, scene, samples);
    if (!film.uniform()) {
        const std::vector<uint32_t> all = film_all_tiles(film);
        return film_add_tile_window(film, scene, samples, all.data(), (uint32_t)all.size());
    }
    if (film.samples + samples > film.enum_n)
        fail(PT_ERR_INVALID, "%s: the film holds %llu samples, %u more would pass the enumeration's %u", who, (unsigned long long)film.samples, samples, film.enum_n);
    HIP_CHECK(hipSetDevice(film.device));
    if (film.samples) {
        HIP_CHECK(hipMemcpy(film.pass_accum, film.accum, film.stride_a * sizeof(float), hipMemcpyDeviceToDevice));
        HIP_CHECK(hipMemcpy(film.pass_moments, film.moments, film.stride_m * sizeof(float), hipMemcpyDeviceToDevice));
    }
    film_render_window(film, scene, (uint32_t)film.samples, samples, nullptr, film.pass_accum, film.pass_moments);
    HIP_CHECK(hipMemcpy(film.accum, film.pass_accum, film.n_local * 12u, hipMemcpyDeviceToDevice));
    HIP_CHECK(hipMemcpy(film.moments, film.pass_moments, film.n_local * 8u, hipMemcpyDeviceToDevice));
    HIP_CHECK(hipDeviceSynchronize());
    ++film.passes;
    ++film.windows;
    film.last_pass_samples = samples;
    film.last_pass_tiles = 0;
    film.samples += samples;
}

void film_check_window_params(const char* who, const pt_film* film, const pt_scene* scene, const pt_film_window_params* params) {
    if (!film->windowed) fail(PT_ERR_INVALID, "%s: the film is not windowed (pt_film_create_windowed)", who);
    film_check_tiled(who, film);
    film_check_noise_args(who, params->lum_floor, params->target);
    if (params->window_samples < 1u) fail(PT_ERR_INVALID, "%s: window_samples must be >= 1", who);
    if (!film->passes && params->window_samples < 2u)
        fail(PT_ERR_INVALID, "%s: the first window needs >= 2 samples (a sample variance needs two)", who);
    if (params->dilate > 1u) fail(PT_ERR_INVALID, "%s: dilate must be 0 or 1", who);
    if (params->adaptive > 1u) fail(PT_ERR_INVALID, "%s: adaptive must be 0 or 1", who);
    if (scene->device != film->device)
        fail(PT_ERR_INVALID, "%s: the scene is on device %d, the film on device %d", who, scene->device, film->device);
}

// The loop of pt_film_render_until_windowed (include/ptgpu.h).
// noise(st, sums): as in film_adaptive_loop.
template <class Noise>
void film_window_loop(pt_film* film, const pt_scene* scene, const pt_film_window_params* params, pt_film_pass_fn on_pass, void* user,
                      pt_film_tile_stats* out, Noise noise) {
    const FilmTiling T = film_tiling(*film);
    const uint32_t n_tiles = film_n_tiles(*film), N = film->enum_n;
    std::vector<float> sums(n_tiles);
    std::vector<uint32_t> active, todo;
    pt_film_tile_stats st{};
    bool measured = false;
    auto measure = [&](uint32_t rendered) {
        noise(st, sums.data());
        st.active_tiles = rendered;
        measured = true;
        film_select_active(T, sums, params->target, params->dilate, active);
    };
    auto least = [&] { return film->uniform() ? film->samples : *std::min_element(film->tile_count.begin(), film->tile_count.end()); };
    if (film->passes && least() >= 2u && (!params->adaptive || film->samples >= params->uniform_samples)) measure(0);
    for (;;) {
        if (measured && st.converged) break;
        const bool all = !measured || !film->passes || !params->adaptive || film->samples < params->uniform_samples;
        // the tiles of the next window: the active set without the tiles that are full; the window is clipped so that none passes N
        todo.clear();
        uint64_t most = 0;
        for (uint32_t i = 0; i < (all ? n_tiles : (uint32_t)active.size()); ++i) {
            const uint32_t t = all ? i : active[i];
            const uint64_t c = film_count_of(*film, t);
            if (c >= N) continue;
            todo.push_back(t);
            most = std::max(most, c);
        }
        if (todo.empty()) break;   // budget
        const uint32_t w = (uint32_t)std::min<uint64_t>(params->window_samples, N - most);
        if (film->uniform() && todo.size() == n_tiles) film_add_window(*film, scene, w);
        else film_add_tile_window(*film, scene, w, todo.data(), (uint32_t)todo.size());
        measure((uint32_t)todo.size());
        if (on_pass) {
            pt_film_info info;
            film_fill_info(*film, info);
            pt_film_noise_stats ns{};
            ns.mean_error = st.mean_error;
            ns.max_block_error = st.max_tile_error;
            ns.fraction_over = (double)st.over_tiles / (double)n_tiles;
            ns.samples = st.samples;
            ns.n_blocks = n_tiles;
            ns.converged = st.converged;
            on_pass(&info, &ns, user);
        }
    }
    if (!measured) noise(st, nullptr);   // (a full film that was never measured)
    *out = st;
}

// ---- sharded films (pt_film_shard.h)
// This rank's tile sums and maxima: one entry per tile of the image, 0.f for the tiles of other ranks.  err_host: packed local.
void film_shard_tile_noise(const pt_film& film_c, float lum_floor, float* tile_sum_host, float* tile_max_host, float* err_host) {
    const char* who = "pt_film_shard_tile_noise";
    film_check_shard(who, &film_c);
    film_check_noise_args(who, lum_floor, 0.0);
    pt_film& film = const_cast<pt_film&>(film_c);   // (the tile arrays are made on first use: scratch, not the film's contents)
    const uint32_t n_tiles = film_n_tiles(film);
    const uint64_t least = film.uniform() ? film.samples : *std::min_element(film.tile_count.begin(), film.tile_count.end());
    if (least < 2u) fail(PT_ERR_INVALID, "%s: a sample variance needs >= 2 samples in every pixel (the fewest: %llu)", who, (unsigned long long)least);
    HIP_CHECK(hipSetDevice(film.device));
    if (!film.tile_sum) {
        HIP_CHECK(hipMalloc((void**)&film.tile_sum, (size_t)n_tiles * 8u));
        film.bytes_adaptive += (uint64_t)n_tiles * 8u;
    }
    film_launch_tile_noise(film, lum_floor, err_host ? film.err : (float*)nullptr, film.tile_sum, film.tile_sum + n_tiles);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipDeviceSynchronize());
    if (tile_sum_host) HIP_CHECK(hipMemcpy(tile_sum_host, film.tile_sum, n_tiles * sizeof(float), hipMemcpyDeviceToHost));
    if (tile_max_host) HIP_CHECK(hipMemcpy(tile_max_host, film.tile_sum + n_tiles, n_tiles * sizeof(float), hipMemcpyDeviceToHost));
    if (err_host) HIP_CHECK(hipMemcpy(err_host, film.err, film.n_local * sizeof(float), hipMemcpyDeviceToHost));
}

// Step 4 of the sharded loops: the local tile noise, the exchange, the host statistics of the complete array.
struct ShardNoise {
    const char* who;
    pt_film* film;
    float lum_floor;
    double target;
    pt_film_exchange_fn exchange;
    void* exchange_user;
    void operator()(pt_film_tile_stats& st, float* sums) const {
        const uint32_t n_tiles = film_n_tiles(*film);
        std::vector<float> s(n_tiles), m(n_tiles);
        film_shard_tile_noise(*film, lum_floor, s.data(), m.data(), nullptr);
        if (exchange) {
            const int rc = exchange(s.data(), m.data(), n_tiles, exchange_user);
            if (rc != 0) fail(PT_ERR_DEVICE, "%s: the exchange of the tile noise failed (the callback returned %d)", who, rc);
        }
        film_tile_stats(*film, s, target, st);
        if (sums) memcpy(sums, s.data(), n_tiles * sizeof(float));
    }
};
void film_check_sharded_loop(const char* who, const pt_film* film, pt_film_exchange_fn exchange) {
    film_check_shard(who, film);
    if (!exchange && film->opts.shard_count > 1)
        fail(PT_ERR_INVALID, "%s: %u ranks hold the film, the loop needs an exchange", who, film->opts.shard_count);
}

// whole = the shards' planes in image order, and their counters.  Every refusal comes before any device work.
void film_assemble(pt_film& whole, const pt_film* const* shards, uint32_t n) {
    const char* who = "pt_film_assemble";
    if (!whole.has_profile || whole.shard || whole.opts.shard_count > 1)
        fail(PT_ERR_INVALID, "%s: the whole film must be an unsharded film with a profile (pt_film_create, pt_film_create_windowed)", who);
    if (whole.passes || whole.samples || !whole.uniform()) fail(PT_ERR_INVALID, "%s: the whole film must be empty (pt_film_reset)", who);
    if (!shards || !n) fail(PT_ERR_INVALID, "%s: null argument", who);
    const pt_film* s0 = shards[0];
    std::vector<uint8_t> seen(n, 0);
    for (uint32_t i = 0; i < n; ++i) {
        const pt_film* s = shards[i];
        film_check_shard(who, s);
        if (s->opts.shard_count != n) fail(PT_ERR_INVALID, "%s: %u shards of a film that %u ranks hold", who, n, s->opts.shard_count);
        if (seen[s->opts.shard_rank]) fail(PT_ERR_INVALID, "%s: rank %u appears twice", who, s->opts.shard_rank);
        seen[s->opts.shard_rank] = 1;   // (n distinct ranks below n: none is missing)
        const pt_profile &a = s->profile, &b = whole.profile;
        if (a.width != b.width || a.height != b.height || a.bounces != b.bounces || a.brdf != b.brdf || a.tonemap != b.tonemap)
            fail(PT_ERR_INVALID, "%s: shard %u has another profile than the whole film", who, i);
        if (s->opts.tile_w != whole.opts.tile_w || s->opts.tile_h != whole.opts.tile_h)
            fail(PT_ERR_INVALID, "%s: shard %u has tiles of %u x %u, the whole film of %u x %u", who, i, s->opts.tile_w, s->opts.tile_h,
                 whole.opts.tile_w, whole.opts.tile_h);
        if (s->windowed != whole.windowed || s->enum_n != whole.enum_n)
            fail(PT_ERR_INVALID, "%s: shard %u and the whole film differ in kind (windowed or not, the enumeration)", who, i);
        if (s->passes != s0->passes || s->last_pass_samples != s0->last_pass_samples || s->samples != s0->samples ||
            s->tile_passes != s0->tile_passes || s->last_pass_tiles != s0->last_pass_tiles || s->windows != s0->windows ||
            s->tile_windows != s0->tile_windows || s->uniform() != s0->uniform() || s->tile_count != s0->tile_count)
            fail(PT_ERR_INVALID, "%s: shard %u has other counters than shard 0 (they are not parts of one film)", who, i);
    }
    HIP_CHECK(hipSetDevice(whole.device));
    const bool counts = !s0->uniform();
    if (counts) film_make_non_uniform(whole);
    const size_t table_before = whole.table.bytes;
    whole.table.ensure((size_t)(2u * film_n_tiles(whole) + 1u) * 4u);
    whole.bytes_adaptive += whole.table.bytes - table_before;
    for (uint32_t i = 0; i < n; ++i) {
        const pt_film& s = *shards[i];
        const float *src_a = s.accum, *src_m = s.moments;
        const uint32_t* src_c = s.count;
        if (s.device != whole.device) {   // staged through the host into the whole film's pass buffers (counts: its err plane)
            std::vector<float> ha(3u * s.n_local), hm(2u * s.n_local);
            std::vector<uint32_t> hc(counts ? s.n_local : 0u);
            HIP_CHECK(hipSetDevice(s.device));
            HIP_CHECK(hipMemcpy(ha.data(), s.accum, ha.size() * 4u, hipMemcpyDeviceToHost));
            HIP_CHECK(hipMemcpy(hm.data(), s.moments, hm.size() * 4u, hipMemcpyDeviceToHost));
            if (counts) HIP_CHECK(hipMemcpy(hc.data(), s.count, hc.size() * 4u, hipMemcpyDeviceToHost));
            HIP_CHECK(hipSetDevice(whole.device));
            HIP_CHECK(hipMemcpy(whole.pass_accum, ha.data(), ha.size() * 4u, hipMemcpyHostToDevice));
            HIP_CHECK(hipMemcpy(whole.pass_moments, hm.data(), hm.size() * 4u, hipMemcpyHostToDevice));
            if (counts) HIP_CHECK(hipMemcpy(whole.err, hc.data(), hc.size() * 4u, hipMemcpyHostToDevice));
            src_a = whole.pass_accum, src_m = whole.pass_moments, src_c = counts ? (const uint32_t*)whole.err : nullptr;
        }
        if (!s.packed) {   // one rank: image order already
            HIP_CHECK(hipMemcpy(whole.accum, src_a, s.n_local * 12u, hipMemcpyDeviceToDevice));
            HIP_CHECK(hipMemcpy(whole.moments, src_m, s.n_local * 8u, hipMemcpyDeviceToDevice));
            if (counts) HIP_CHECK(hipMemcpy(whole.count, src_c, s.n_local * 4u, hipMemcpyDeviceToDevice));
        } else {
            const TileMap tm = make_tile_map(s.profile, s.opts, s.opts.shard_rank);
            film_upload_table(whole, tm);
            hipLaunchKernelGGL(k_film_import_shard, dim3(tm.n_local_tiles), dim3(256), 0, 0, src_a, (const float2*)src_m, src_c,
                               (const uint32_t*)whole.table.p, tm.n_local_tiles, film_tiling(whole), whole.accum, (float2*)whole.moments,
                               counts ? whole.count : (uint32_t*)nullptr);
            HIP_CHECK(hipGetLastError());
        }
        HIP_CHECK(hipDeviceSynchronize());   // (the table and the staging planes are rewritten by the next shard)
    }
    whole.passes = s0->passes;
    whole.last_pass_samples = s0->last_pass_samples;
    whole.samples = s0->samples;
    whole.tile_passes = s0->tile_passes;
    whole.last_pass_tiles = s0->last_pass_tiles;
    whole.windows = s0->windows;
    whole.tile_windows = s0->tile_windows;
    if (counts) whole.tile_count = s0->tile_count;
}

// ---- the film filter (pt_film_denoise.h)
struct FdnScratch {   // pt_film_denoise_scratch_bytes: the filter's planes, the ferr plane, the two tile arrays
    DnScratch dn;
    uint64_t ferr, tile_sum, tile_max, total;
};
FdnScratch fdn_scratch_layout(uint64_t n, uint32_t n_tiles) {
    auto up = [](uint64_t v) { return (v + 255u) & ~(uint64_t)255u; };
    FdnScratch L;
    L.dn = dn_scratch_layout(n);
    L.ferr = L.dn.total;
    L.tile_sum = L.ferr + up(4u * n);
    L.tile_max = L.tile_sum + up(4u * (uint64_t)n_tiles);
    L.total = L.tile_max + up(4u * (uint64_t)n_tiles);
    return L;
}
FdnScratch fdn_scratch_layout(const pt_film& film) { return fdn_scratch_layout(film.n_local, film_n_tiles(film)); }

// What the pt_film_denoise family refuses before any device work (null pointers other than the film are the callers').
void fdn_check(const char* who, const pt_film* film, int variance, const pt_denoise_params* p, float lum_floor, bool want_ferr) {
    film_check_tiled(who, film);
    film_refuse_shard(who, film);
    if (variance != 0 && variance != 1) fail(PT_ERR_INVALID, "%s: variance must be 0 (plain) or 1 (variance-guided)", who);
    if (!variance && want_ferr) fail(PT_ERR_INVALID, "%s: the plain filter carries no variance, so it has no ferr", who);
    if (variance) dnv_check(who, p, film->profile.width, film->profile.height, 2u);
    else {
        dn_check_params(who, p);
        dn_check_size(who, film->profile.width, film->profile.height);
    }
    film_check_noise_args(who, lum_floor, 0.0);
    const uint64_t least = film->uniform() ? film->samples : *std::min_element(film->tile_count.begin(), film->tile_count.end());
    if (least == 0) fail(PT_ERR_INVALID, "%s: some pixels of the film hold no samples", who);
    if (variance && least < 2u) fail(PT_ERR_INVALID, "%s: a sample variance needs >= 2 samples in every pixel (the fewest: %llu)", who, (unsigned long long)least);
}
void fdn_check_scene(const char* who, const pt_film* film, const pt_scene* scene) {
    if (scene->device != film->device)
        fail(PT_ERR_INVALID, "%s: the scene is on device %d, the film on device %d", who, scene->device, film->device);
}

// prep, the passes and the finish on the film's planes; d_color, d_rgb8 and d_ferr (variance only) may be null.
// ev (measurement only): 4 events - before prep, after prep, after the passes, after the finish.
void fdn_launch(const FilmPlanes& film, int variance, const pt_denoise_params& p, float lum_floor, const float4* d_guides,
                float* d_color, uint8_t* d_rgb8, float* d_ferr, uint8_t* d_scratch, hipStream_t stream, hipEvent_t* ev = nullptr) {
    const uint32_t width = film.width, height = film.height, n = width * height, blocks = (n + 255u) / 256u;
    const uint32_t no_demod = p.flags & PT_DENOISE_NO_DEMODULATE;
    const float2* mom = (const float2*)film.moments;
    size_t e = 0;
    if (ev) HIP_CHECK(hipEventRecord(ev[e++], stream));
    if (p.iterations == 0) {   // nothing is filtered: the film's resolve, and the raw error
        if (ev) HIP_CHECK(hipEventRecord(ev[e++], stream));
        if (ev) HIP_CHECK(hipEventRecord(ev[e++], stream));
        if (d_color || d_rgb8) film_resolve_launch(film, p.tonemap, d_rgb8, d_color, stream);
        if (d_ferr)
            hipLaunchKernelGGL(k_fdn_finish, dim3(blocks), dim3(256), 0, stream, (const float4*)nullptr, (const float*)nullptr,
                               film.accum, mom, film.count, film.samples, n, no_demod,
                               p.tonemap, lum_floor, (float*)nullptr, (uint8_t*)nullptr, d_ferr);
        HIP_CHECK(hipGetLastError());
        if (ev) HIP_CHECK(hipEventRecord(ev[e++], stream));
        return;
    }
    const DnScratch L = dn_scratch_layout(n);
    float4* X = (float4*)(d_scratch + L.xa);
    float4* Y = (float4*)(d_scratch + L.xb);
    float4* U = (float4*)(d_scratch + L.u);
    float2* G = (float2*)(d_scratch + L.g);
    float* D = (float*)(d_scratch + L.d);
    if (variance)
        hipLaunchKernelGGL(k_fdn_prep<1>, dim3(blocks), dim3(256), 0, stream, film.accum, mom, film.count,
                           film.samples, d_guides, width, height, no_demod, X, U, G, D);
    else
        hipLaunchKernelGGL(k_fdn_prep<0>, dim3(blocks), dim3(256), 0, stream, film.accum, mom, film.count,
                           film.samples, d_guides, width, height, no_demod, X, U, G, D);
    HIP_CHECK(hipGetLastError());
    if (ev) HIP_CHECK(hipEventRecord(ev[e++], stream));
    size_t unused = 0;
    if (variance) dnv_passes(width, height, p, X, Y, U, G, stream, nullptr, unused);
    else dn_passes(width, height, p, X, Y, U, G, stream, nullptr, unused);
    if (ev) HIP_CHECK(hipEventRecord(ev[e++], stream));
    if (variance)
        hipLaunchKernelGGL(k_fdn_finish, dim3(blocks), dim3(256), 0, stream, (const float4*)X, (const float*)D, film.accum,
                           mom, film.count, film.samples, n, no_demod, p.tonemap, lum_floor, d_color,
                           d_rgb8, d_ferr);
    else   // (past the passes k_dn_finish reads neither accum nor samples)
        hipLaunchKernelGGL(k_dn_finish, dim3(blocks), dim3(256), 0, stream, (const float4*)X, (const float*)D, film.accum,
                           film.samples, n, no_demod, p.tonemap, d_color, d_rgb8);
    HIP_CHECK(hipGetLastError());
    if (ev) HIP_CHECK(hipEventRecord(ev[e++], stream));
}

void fdn_launch(const pt_film& film, int variance, const pt_denoise_params& p, float lum_floor, const float4* d_guides,
                float* d_color, uint8_t* d_rgb8, float* d_ferr, uint8_t* d_scratch, hipStream_t stream, hipEvent_t* ev = nullptr) {
    fdn_launch(film_planes(film), variance, p, lum_floor, d_guides, d_color, d_rgb8, d_ferr, d_scratch, stream, ev);
}

void fdn_tile_reduce_launch(const pt_film& film, const float* d_err, float* d_tile_sum, float* d_tile_max, hipStream_t stream) {
    hipLaunchKernelGGL(k_film_tile_reduce, dim3(film_n_tiles(film)), dim3(256), 0, stream, d_err, film_tiling(film), d_tile_sum, d_tile_max);
    HIP_CHECK(hipGetLastError());
}

// The host forms' scratch, made on first use: pt_film_denoise_scratch_bytes and a plane of guides behind it.
uint8_t* film_filter_scratch(const pt_film& film_c) {
    pt_film& film = const_cast<pt_film&>(film_c);   // (scratch, not the film's contents)
    if (!film.filter) {
        const uint64_t bytes = fdn_scratch_layout(film).total + 32u * film.n_local;
        HIP_CHECK(hipMalloc((void**)&film.filter, bytes));
        film.bytes_filter = bytes;
    }
    return film.filter;
}
float4* film_filter_guides(const pt_film& film) { return (float4*)(film_filter_scratch(film) + fdn_scratch_layout(film).total); }

// Steps 2 - 5 of pt_film_filtered_noise over guides that are on the device already.
void film_filtered_noise(const pt_film& film, const float4* d_guides, const pt_denoise_params& p, float lum_floor, double target,
                         pt_film_tile_stats& out, float* ferr_host, float* tile_sum_host, float* tile_max_host) {
    uint8_t* scratch = film_filter_scratch(film);
    const FdnScratch L = fdn_scratch_layout(film);
    const uint32_t n_tiles = film_n_tiles(film);
    float *ferr = (float*)(scratch + L.ferr), *tile_sum = (float*)(scratch + L.tile_sum), *tile_max = (float*)(scratch + L.tile_max);
    fdn_launch(film, 1, p, lum_floor, d_guides, nullptr, nullptr, ferr, scratch, nullptr);
    fdn_tile_reduce_launch(film, ferr, tile_sum, tile_max, nullptr);
    std::vector<float> sums(n_tiles);
    HIP_CHECK(hipMemcpy(sums.data(), tile_sum, n_tiles * sizeof(float), hipMemcpyDeviceToHost));   // (waits for the kernels)
    if (tile_sum_host) memcpy(tile_sum_host, sums.data(), n_tiles * sizeof(float));
    if (tile_max_host) HIP_CHECK(hipMemcpy(tile_max_host, tile_max, n_tiles * sizeof(float), hipMemcpyDeviceToHost));
    if (ferr_host) HIP_CHECK(hipMemcpy(ferr_host, ferr, film.n_local * sizeof(float), hipMemcpyDeviceToHost));
    film_tile_stats(film, sums, target, out);
}

}  // namespace

// ==================================================================== C ABI
extern "C" {

const char* pt_last_error(void) { return g_err.c_str(); }
const char* pt_version(void) { return "path-tracer_amd 0.1 (gfx950)"; }

int pt_scene_create(const pt_scene_desc* desc, int device, pt_scene** out) {
    return guarded([&] {
        if (!desc || !out) fail(PT_ERR_INVALID, "pt_scene_create: null argument");
        pt_prep prep;
        auto s = std::make_unique<pt_scene>();
        EarlyGrids early{*s, device};
        prep_create(*desc, prep, &early);
        scene_upload(prep, device, *s, early.built ? &early.grids : nullptr);
        *out = s.release();
    });
}

int pt_prep_create(const pt_scene_desc* desc, pt_prep** out) {
    return guarded([&] {
        if (!desc || !out) fail(PT_ERR_INVALID, "pt_prep_create: null argument");
        auto p = std::make_unique<pt_prep>();
        prep_create(*desc, *p);
        *out = p.release();
    });
}

void pt_prep_destroy(pt_prep* prep) { delete prep; }

int pt_scene_create_from_prep(const pt_prep* prep, int device, pt_scene** out) {
    return guarded([&] {
        if (!prep || !out) fail(PT_ERR_INVALID, "pt_scene_create_from_prep: null argument");
        auto s = std::make_unique<pt_scene>();
        scene_upload(*prep, device, *s);
        *out = s.release();
    });
}

void pt_scene_destroy(pt_scene* scene) { delete scene; }

int pt_scene_set_camera(pt_scene* scene, const pt_camera* camera) {
    return guarded([&] {
        if (!scene || !camera) fail(PT_ERR_INVALID, "pt_scene_set_camera: null argument");
        scene_set_camera(*scene, *camera);
    });
}

int pt_scene_set_lights(pt_scene* scene, const pt_light* lights, uint32_t n_lights) {
    return guarded([&] {
        if (!scene || (!lights && n_lights > 0)) fail(PT_ERR_INVALID, "pt_scene_set_lights: null argument");
        scene_set_lights(*scene, lights, n_lights);
    });
}

int pt_scene_set_materials(pt_scene* scene, const pt_material* materials, uint32_t n_materials) {
    return guarded([&] {
        if (!scene || !materials) fail(PT_ERR_INVALID, "pt_scene_set_materials: null argument");
        scene_set_materials(*scene, materials, n_materials);
    });
}

uint64_t pt_local_pixel_count(const pt_profile* profile, const pt_opts* opts) {
    uint64_t n = 0;
    guarded([&] {
        if (!profile) fail(PT_ERR_INVALID, "pt_local_pixel_count: null profile");
        pt_opts o;
        normalise_opts(*profile, opts, o);
        n = make_tile_map(*profile, o, o.shard_rank).n_local;
    });
    return n;
}

int pt_local_pixel_map(const pt_profile* profile, const pt_opts* opts, uint32_t* out) {
    return guarded([&] {
        if (!profile || !out) fail(PT_ERR_INVALID, "pt_local_pixel_map: null argument");
        pt_opts o;
        normalise_opts(*profile, opts, o);
        const pt_profile& p = *profile;
        if (o.shard_count <= 1) {
            for (uint64_t i = 0; i < (uint64_t)p.width * p.height; ++i) out[i] = (uint32_t)i;
            return;
        }
        TileMap tm = make_tile_map(p, o, o.shard_rank);
        for (uint32_t lt = 0; lt < tm.n_local_tiles; ++lt) {
            uint32_t k = tm.tiles[lt];
            uint32_t tx = k % tm.tiles_x, ty = k / tm.tiles_x;
            uint32_t cw = std::min(o.tile_w, p.width - tx * o.tile_w), ch = std::min(o.tile_h, p.height - ty * o.tile_h);
            for (uint32_t y = 0; y < ch; ++y)
                for (uint32_t x = 0; x < cw; ++x)
                    out[tm.offsets[lt] + y * cw + x] = (tx * o.tile_w + x) + (ty * o.tile_h + y) * p.width;
        }
    });
}

int pt_render_device(const pt_scene* scene, const pt_profile* profile, const pt_opts* opts, void* d_rgb8,
                     void* d_accum, void* hip_stream) {
    return guarded([&] {
        if (!scene || !profile) fail(PT_ERR_INVALID, "pt_render_device: null argument");
        render_device(render_state(scene), *profile, opts, d_rgb8, d_accum, (hipStream_t)hip_stream);
    });
}

int pt_render(const pt_scene* scene, const pt_profile* profile, const pt_opts* opts, uint8_t* rgb8, float* accum) {
    return guarded([&] {
        if (!scene || !profile) fail(PT_ERR_INVALID, "pt_render: null argument");
        HIP_CHECK(hipSetDevice(scene->device));
        pt_opts o;
        normalise_opts(*profile, opts, o);
        uint64_t n = make_tile_map(*profile, o, o.shard_rank).n_local;
        Staged<uint8_t> d_rgb(nullptr, n * 3);
        Staged<float> d_acc(nullptr, n * 3);
        render_device(render_state(scene), *profile, opts, d_rgb.d, d_acc.d, nullptr, true);
        HIP_CHECK(hipDeviceSynchronize());
        if (rgb8) d_rgb.fetch(rgb8, n * 3);
        if (accum) d_acc.fetch(accum, n * 3);
    });
}

uint64_t pt_tiles_pixel_count(const pt_profile* profile, const pt_opts* opts, const uint32_t* tiles, uint32_t n_tiles) {
    uint64_t n = 0;
    guarded([&] {
        if (!profile) fail(PT_ERR_INVALID, "pt_tiles_pixel_count: null profile");
        pt_opts o;
        normalise_opts(*profile, opts, o);
        n = make_tile_list_map("pt_tiles_pixel_count", *profile, o, tiles, n_tiles).n_local;
    });
    return n;
}

int pt_tiles_pixel_map(const pt_profile* profile, const pt_opts* opts, const uint32_t* tiles, uint32_t n_tiles, uint32_t* out) {
    return guarded([&] {
        if (!profile || !out) fail(PT_ERR_INVALID, "pt_tiles_pixel_map: null argument");
        pt_opts o;
        normalise_opts(*profile, opts, o);
        const pt_profile& p = *profile;
        const TileMap tm = make_tile_list_map("pt_tiles_pixel_map", p, o, tiles, n_tiles);
        for (uint32_t lt = 0; lt < tm.n_local_tiles; ++lt) {
            const uint32_t k = tm.tiles[lt];
            const uint32_t tx = k % tm.tiles_x, ty = k / tm.tiles_x;
            const uint32_t cw = std::min(o.tile_w, p.width - tx * o.tile_w), ch = std::min(o.tile_h, p.height - ty * o.tile_h);
            for (uint32_t y = 0; y < ch; ++y)
                for (uint32_t x = 0; x < cw; ++x)
                    out[tm.offsets[lt] + y * cw + x] = (tx * o.tile_w + x) + (ty * o.tile_h + y) * p.width;
        }
    });
}

int pt_render_tiles_device(const pt_scene* scene, const pt_profile* profile, const pt_opts* opts, const uint32_t* tiles,
                           uint32_t n_tiles, void* d_rgb8, void* d_accum, void* d_moments, void* hip_stream) {
    return guarded([&] {
        if (!scene || !profile || (!d_rgb8 && !d_accum && !d_moments)) fail(PT_ERR_INVALID, "pt_render_tiles_device: null argument");
        const TileList list{tiles, n_tiles};
        FrameTaps taps;
        taps.moments = (float2*)d_moments;
        render_device(render_state(scene), *profile, opts, d_rgb8, d_accum, (hipStream_t)hip_stream, false,
                      d_moments ? &taps : nullptr, &list);
    });
}

int pt_render_tiles(const pt_scene* scene, const pt_profile* profile, const pt_opts* opts, const uint32_t* tiles, uint32_t n_tiles,
                    uint8_t* rgb8, float* accum, float* moments) {
    return guarded([&] {
        if (!scene || !profile || (!rgb8 && !accum && !moments)) fail(PT_ERR_INVALID, "pt_render_tiles: null argument");
        pt_opts o;
        normalise_opts(*profile, opts, o);
        const uint64_t n = make_tile_list_map("pt_render_tiles", *profile, o, tiles, n_tiles).n_local;
        if (moments) moments_check_opts("pt_render_tiles", opts);
        HIP_CHECK(hipSetDevice(scene->device));
        Staged<uint8_t> d_rgb(nullptr, n * 3);
        Staged<float> d_acc(nullptr, n * 3);
        Staged<float2> d_mom(nullptr, moments ? n : 0);
        const TileList list{tiles, n_tiles};
        FrameTaps taps;
        taps.moments = d_mom.d;
        render_device(render_state(scene), *profile, opts, d_rgb.d, d_acc.d, nullptr, false, moments ? &taps : nullptr, &list);
        HIP_CHECK(hipDeviceSynchronize());
        if (rgb8) d_rgb.fetch(rgb8, n * 3);
        if (accum) d_acc.fetch(accum, n * 3);
        if (moments) d_mom.fetch((float2*)moments, n);
    });
}

int pt_render_window_device(const pt_scene* scene, const pt_profile* profile, const pt_opts* opts, uint32_t s0, uint32_t s1,
                            const uint32_t* tiles, uint32_t n_tiles, void* d_rgb8, void* d_accum, void* d_moments, void* hip_stream) {
    return guarded([&] {
        if (!scene || !profile || !d_accum) fail(PT_ERR_INVALID, "pt_render_window_device: null argument");
        if (d_moments) moments_check_opts("pt_render_window_device", opts);
        const TileList list{tiles, n_tiles};
        const SampleWindow win{s0, s1};
        FrameTaps taps;
        taps.moments = (float2*)d_moments;
        render_device(render_state(scene), *profile, opts, d_rgb8, d_accum, (hipStream_t)hip_stream, false,
                      d_moments ? &taps : nullptr, tiles ? &list : nullptr, &win);
    });
}

int pt_render_window(const pt_scene* scene, const pt_profile* profile, const pt_opts* opts, uint32_t s0, uint32_t s1,
                     const uint32_t* tiles, uint32_t n_tiles, uint8_t* rgb8, float* accum, float* moments) {
    return guarded([&] {
        const char* who = "pt_render_window";
        if (!scene || !profile || !accum) fail(PT_ERR_INVALID, "%s: null argument", who);
        if (s0 >= s1 || s1 > profile->samples)
            fail(PT_ERR_INVALID, "%s: the window [%u, %u) of a frame of %u samples", who, s0, s1, profile->samples);
        pt_opts o;
        normalise_opts(*profile, opts, o);
        const uint64_t n = tiles ? make_tile_list_map(who, *profile, o, tiles, n_tiles).n_local
                                 : make_tile_map(*profile, o, o.shard_rank).n_local;
        if (moments) moments_check_opts(who, opts);
        HIP_CHECK(hipSetDevice(scene->device));
        // (the carry: the sums of [0, s0) go in with the buffers; a window that starts at 0 overwrites them)
        Staged<uint8_t> d_rgb(nullptr, n * 3);
        Staged<float> d_acc(s0 ? accum : nullptr, n * 3);
        Staged<float2> d_mom(s0 ? (const float2*)moments : nullptr, moments ? n : 0);
        const TileList list{tiles, n_tiles};
        const SampleWindow win{s0, s1};
        FrameTaps taps;
        taps.moments = d_mom.d;
        render_device(render_state(scene), *profile, opts, d_rgb.d, d_acc.d, nullptr, false, moments ? &taps : nullptr,
                      tiles ? &list : nullptr, &win);
        HIP_CHECK(hipDeviceSynchronize());
        if (rgb8) d_rgb.fetch(rgb8, n * 3);
        d_acc.fetch(accum, n * 3);
        if (moments) d_mom.fetch((float2*)moments, n);
    });
}

int pt_debug_render(const pt_scene* scene, uint32_t width, uint32_t height, uint8_t* planes, int* any_hit) {
    return guarded([&] {
        if (!scene || !planes || !any_hit) fail(PT_ERR_INVALID, "pt_debug_render: null argument");
        if (!width || !height || (uint64_t)width * height >= (1ull << 31)) fail(PT_ERR_INVALID, "pt_debug_render: bad resolution");
        HIP_CHECK(hipSetDevice(scene->device));
        size_t bytes = (size_t)width * height * 3 * PT_DEBUG_PLANES;
        Staged<uint8_t> d_planes(nullptr, bytes);
        Staged<int> d_flag(nullptr, 1);
        HIP_CHECK(hipMemset(d_planes.d, 0, bytes));
        HIP_CHECK(hipMemset(d_flag.d, 0, sizeof(int)));
        hipLaunchKernelGGL(k_debug, dim3((width * height + 255u) / 256u), dim3(256), 0, 0, scene->dev, width, height,
                           d_planes.d, d_flag.d);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipDeviceSynchronize());
        d_planes.fetch(planes, bytes);
        d_flag.fetch(any_hit, 1);
    });
}

int pt_render_guides_device(const pt_scene* scene, uint32_t width, uint32_t height, void* d_guides, void* hip_stream) {
    return guarded([&] {
        if (!scene || !d_guides) fail(PT_ERR_INVALID, "pt_render_guides_device: null argument");
        dn_check_size("pt_render_guides_device", width, height);
        HIP_CHECK(hipSetDevice(scene->device));
        guides_launch(*scene, width, height, (float4*)d_guides, (hipStream_t)hip_stream);
    });
}

int pt_render_guides(const pt_scene* scene, uint32_t width, uint32_t height, float* guides) {
    return guarded([&] {
        if (!scene || !guides) fail(PT_ERR_INVALID, "pt_render_guides: null argument");
        dn_check_size("pt_render_guides", width, height);
        HIP_CHECK(hipSetDevice(scene->device));
        const size_t n = (size_t)width * height;
        Staged<float4> d_guides(nullptr, n * 2);
        guides_launch(*scene, width, height, d_guides.d, nullptr);
        HIP_CHECK(hipDeviceSynchronize());
        d_guides.fetch((float4*)guides, n * 2);
    });
}

void pt_denoise_params_default(pt_denoise_params* p) {
    if (!p) return;
    // the winner of tools/measure_denoise_gain.py (tests/golden/denoise_gain.json)
    p->iterations = PT_DENOISE_DEFAULT_ITERATIONS;
    p->flags = 0;
    p->normal_power_log2 = PT_DENOISE_DEFAULT_NORMAL_POWER_LOG2;
    p->tonemap = PT_TONEMAP_FILMIC;
    p->sigma_color = PT_DENOISE_DEFAULT_SIGMA_COLOR;
    p->sigma_depth = PT_DENOISE_DEFAULT_SIGMA_DEPTH;
}

uint64_t pt_denoise_scratch_bytes(uint32_t width, uint32_t height) {
    const uint64_t n = (uint64_t)width * height;
    return n ? dn_scratch_layout(n).total : 0;
}

int pt_denoise_device(int device, uint32_t width, uint32_t height, uint32_t samples, const pt_denoise_params* params,
                      const void* d_accum, const void* d_guides, void* d_out_color, void* d_out_rgb8, void* d_scratch,
                      void* hip_stream) {
    return guarded([&] {
        dn_check_params("pt_denoise_device", params);
        if (!d_accum || !d_guides || (!d_scratch && params->iterations)) fail(PT_ERR_INVALID, "pt_denoise_device: null argument");
        dn_check_size("pt_denoise_device", width, height);
        if (!samples) fail(PT_ERR_INVALID, "pt_denoise_device: samples is 0");
        if (device >= 0) HIP_CHECK(hipSetDevice(device));
        denoise_launch(width, height, samples, *params, (const float*)d_accum, (const float4*)d_guides, (float*)d_out_color,
                       (uint8_t*)d_out_rgb8, (uint8_t*)d_scratch, (hipStream_t)hip_stream);
    });
}

int pt_denoise(int device, uint32_t width, uint32_t height, uint32_t samples, const pt_denoise_params* params,
               const float* accum, const float* guides, float* out_color, uint8_t* out_rgb8) {
    return guarded([&] {
        dn_check_params("pt_denoise", params);
        if (!accum || !guides) fail(PT_ERR_INVALID, "pt_denoise: null argument");
        dn_check_size("pt_denoise", width, height);
        if (!samples) fail(PT_ERR_INVALID, "pt_denoise: samples is 0");
        if (device >= 0) HIP_CHECK(hipSetDevice(device));
        const size_t n = (size_t)width * height;
        Staged<float> d_acc(accum, n * 3), d_color(nullptr, n * 3);
        Staged<float4> d_guides((const float4*)guides, n * 2);
        Staged<uint8_t> d_rgb(nullptr, n * 3), d_scratch(nullptr, pt_denoise_scratch_bytes(width, height));
        denoise_launch(width, height, samples, *params, d_acc.d, d_guides.d, d_color.d, d_rgb.d, d_scratch.d, nullptr);
        HIP_CHECK(hipDeviceSynchronize());
        if (out_color) d_color.fetch(out_color, n * 3);
        if (out_rgb8) d_rgb.fetch(out_rgb8, n * 3);
    });
}

int pt_denoise_stage_times(int device, uint32_t width, uint32_t height, uint32_t samples, const pt_denoise_params* params,
                           const void* d_accum, const void* d_guides, void* d_out_color, void* d_out_rgb8, void* d_scratch,
                           float* ms) {
    return guarded([&] {
        dn_check_params("pt_denoise_stage_times", params);
        if (!d_accum || !d_guides || !ms || (!d_scratch && params->iterations)) fail(PT_ERR_INVALID, "pt_denoise_stage_times: null argument");
        dn_check_size("pt_denoise_stage_times", width, height);
        if (!samples) fail(PT_ERR_INVALID, "pt_denoise_stage_times: samples is 0");
        if (device >= 0) HIP_CHECK(hipSetDevice(device));
        const size_t n_ev = params->iterations ? params->iterations + 3u : 2u;
        std::vector<hipEvent_t> ev(n_ev, nullptr);
        struct Free {
            std::vector<hipEvent_t>& e;
            ~Free() {
                for (hipEvent_t x : e)
                    if (x) (void)hipEventDestroy(x);
            }
        } guard{ev};
        for (hipEvent_t& x : ev) HIP_CHECK(hipEventCreate(&x));
        denoise_launch(width, height, samples, *params, (const float*)d_accum, (const float4*)d_guides, (float*)d_out_color,
                       (uint8_t*)d_out_rgb8, (uint8_t*)d_scratch, nullptr, ev.data());
        HIP_CHECK(hipDeviceSynchronize());
        for (int k = 0; k < PT_DENOISE_STAGES; ++k) ms[k] = 0.f;
        if (params->iterations == 0) {
            HIP_CHECK(hipEventElapsedTime(&ms[PT_DENOISE_STAGES - 1], ev[0], ev[1]));
            return;
        }
        HIP_CHECK(hipEventElapsedTime(&ms[0], ev[0], ev[1]));
        for (uint32_t i = 0; i < params->iterations; ++i) HIP_CHECK(hipEventElapsedTime(&ms[1 + i], ev[1 + i], ev[2 + i]));
        HIP_CHECK(hipEventElapsedTime(&ms[PT_DENOISE_STAGES - 1], ev[1 + params->iterations], ev[2 + params->iterations]));
    });
}

int pt_render_denoised(const pt_scene* scene, const pt_profile* profile, const pt_opts* opts, const pt_denoise_params* params,
                       uint8_t* rgb8, float* color) {
    return guarded([&] {
        if (!scene || !profile) fail(PT_ERR_INVALID, "pt_render_denoised: null argument");
        dn_check_params("pt_render_denoised", params);
        pt_opts o;
        normalise_opts(*profile, opts, o);
        if (o.shard_count > 1) fail(PT_ERR_UNSUPPORTED, "pt_render_denoised: the filter needs the whole image (shard_count %u)", o.shard_count);
        if (!profile->samples) fail(PT_ERR_INVALID, "pt_render_denoised: samples is 0");
        HIP_CHECK(hipSetDevice(scene->device));
        const uint32_t w = profile->width, h = profile->height;
        const size_t n = (size_t)w * h;
        Staged<uint8_t> d_rgb(nullptr, n * 3), d_scratch(nullptr, pt_denoise_scratch_bytes(w, h));
        Staged<float> d_acc(nullptr, n * 3), d_color(nullptr, n * 3);
        Staged<float4> d_guides(nullptr, n * 2);
        // the raw frame (its rgb8 feeds the preview callback only), then guides and filter behind it on the same stream
        render_device(render_state(scene), *profile, opts, d_rgb.d, d_acc.d, nullptr, true);
        guides_launch(*scene, w, h, d_guides.d, nullptr);
        denoise_launch(w, h, profile->samples, *params, d_acc.d, d_guides.d, color ? d_color.d : nullptr, rgb8 ? d_rgb.d : nullptr,
                       d_scratch.d, nullptr);
        HIP_CHECK(hipDeviceSynchronize());
        if (rgb8) d_rgb.fetch(rgb8, n * 3);
        if (color) d_color.fetch(color, n * 3);
    });
}

int pt_lightmix_capture(const pt_scene* scene, const pt_profile* profile, const pt_opts* opts, pt_lightmix** out) {
    return guarded([&] {
        if (!scene || !profile || !out) fail(PT_ERR_INVALID, "pt_lightmix_capture: null argument");
        *out = lightmix_capture(render_state(scene), *profile, opts).release();
    });
}

int pt_lightmix_create_from_planes(int device, uint32_t n_lights, uint32_t samples, uint64_t n_local, const float* unit,
                                   const float* planes, pt_lightmix** out) {
    return guarded([&] {
        if (!planes || !out || (!unit && n_lights)) fail(PT_ERR_INVALID, "pt_lightmix_create_from_planes: null argument");
        if (n_lights > (uint32_t)PT_LIGHTMIX_MAX_LIGHTS)
            fail(PT_ERR_UNSUPPORTED, "pt_lightmix_create_from_planes: %u lights, at most %d", n_lights, (int)PT_LIGHTMIX_MAX_LIGHTS);
        if (!samples) fail(PT_ERR_INVALID, "pt_lightmix_create_from_planes: samples is 0");
        if (!n_local || n_local >= (1ull << 31)) fail(PT_ERR_INVALID, "pt_lightmix_create_from_planes: n_local must be in 1 .. 2^31 - 1");
        for (uint32_t l = 0; l < n_lights; ++l)
            if (!std::isfinite(unit[l]) || unit[l] == 0.f) fail(PT_ERR_INVALID, "pt_lightmix_create_from_planes: unit %u must be finite and not 0", l);
        if (device >= 0) HIP_CHECK(hipSetDevice(device));
        else HIP_CHECK(hipGetDevice(&device));
        auto m = lightmix_alloc(device, n_lights, samples, n_local);
        for (uint32_t l = 0; l < n_lights; ++l) m->unit[l] = unit[l];
        for (uint32_t i = 0; i <= n_lights; ++i)
            HIP_CHECK(hipMemcpy(m->plane(i), planes + (uint64_t)i * n_local * 3u, n_local * 12u, hipMemcpyHostToDevice));
        *out = m.release();
    });
}

void pt_lightmix_destroy(pt_lightmix* mix) { delete mix; }

int pt_lightmix_get_info(const pt_lightmix* mix, pt_lightmix_info* info) {
    return guarded([&] {
        if (!mix || !info) fail(PT_ERR_INVALID, "pt_lightmix_get_info: null argument");
        memset(info, 0, sizeof *info);
        info->n_lights = mix->n_lights;
        info->samples = mix->samples;
        info->n_local = mix->n_local;
        info->device_bytes = mix->bytes;
        memcpy(info->unit, mix->unit, sizeof mix->unit);
    });
}

int pt_lightmix_basis(const pt_lightmix* mix, uint32_t plane, float* host) {
    return guarded([&] {
        if (!mix || !host) fail(PT_ERR_INVALID, "pt_lightmix_basis: null argument");
        if (plane > mix->n_lights) fail(PT_ERR_INVALID, "pt_lightmix_basis: plane %u of %u", plane, mix->n_lights + 1u);
        HIP_CHECK(hipSetDevice(mix->device));
        HIP_CHECK(hipMemcpy(host, mix->plane(plane), mix->n_local * 12u, hipMemcpyDeviceToHost));
    });
}

int pt_lightmix_apply_device(const pt_lightmix* mix, const float* colors, int tonemap, void* d_rgb8, void* d_accum, void* hip_stream) {
    return guarded([&] {
        const LmFactors F = lightmix_factors("pt_lightmix_apply_device", mix, colors, tonemap, d_rgb8, d_accum);
        if (((uintptr_t)d_rgb8 & 3u) || ((uintptr_t)d_accum & 15u))
            fail(PT_ERR_INVALID, "pt_lightmix_apply_device: d_rgb8 must be 4-byte and d_accum 16-byte aligned");
        HIP_CHECK(hipSetDevice(mix->device));
        lightmix_launch(*mix, F, tonemap, (uint8_t*)d_rgb8, (float*)d_accum, (hipStream_t)hip_stream);
    });
}

int pt_lightmix_apply(const pt_lightmix* mix, const float* colors, int tonemap, uint8_t* rgb8, float* accum) {
    return guarded([&] {
        const LmFactors F = lightmix_factors("pt_lightmix_apply", mix, colors, tonemap, rgb8, accum);
        HIP_CHECK(hipSetDevice(mix->device));
        const size_t n = (size_t)mix->n_local * 3u;
        Staged<uint8_t> d_rgb(nullptr, n);
        Staged<float> d_acc(nullptr, n);
        lightmix_launch(*mix, F, tonemap, rgb8 ? d_rgb.d : nullptr, accum ? d_acc.d : nullptr, nullptr);
        HIP_CHECK(hipDeviceSynchronize());
        if (rgb8) d_rgb.fetch(rgb8, n);
        if (accum) d_acc.fetch(accum, n);
    });
}

int pt_film_create(int device, const pt_profile* profile, const pt_opts* opts, pt_film** out) {
    return guarded([&] {
        if (!profile || !out) fail(PT_ERR_INVALID, "pt_film_create: null argument");
        moments_check_opts("pt_film_create", opts);
        pt_opts o;
        normalise_opts(*profile, opts, o);
        o.progress = nullptr;
        o.progress_user = nullptr;
        o.preview = nullptr;
        o.preview_user = nullptr;
        if (profile->brdf != PT_BRDF_COOK_TORRANCE) fail(PT_ERR_INVALID, "pt_film_create: unknown brdf %d", profile->brdf);
        if (profile->tonemap < PT_TONEMAP_REINHARD || profile->tonemap > PT_TONEMAP_ACES) fail(PT_ERR_INVALID, "pt_film_create: unknown tonemap %d", profile->tonemap);
        const uint64_t n_local = make_tile_map(*profile, o, o.shard_rank).n_local;
        if (n_local == 0) fail(PT_ERR_INVALID, "pt_film_create: this rank has no pixels");
        if (device >= 0) HIP_CHECK(hipSetDevice(device));
        else HIP_CHECK(hipGetDevice(&device));
        auto f = film_alloc(device, n_local);
        f->has_profile = true;
        f->profile = *profile;
        f->profile.samples = 0;
        f->opts = o;
        *out = f.release();
    });
}

int pt_film_create_from_planes(int device, uint64_t n_local, uint64_t samples, uint32_t last_pass_samples, const float* accum,
                               const float* moments, pt_film** out) {
    return guarded([&] {
        if (!accum || !moments || !out) fail(PT_ERR_INVALID, "pt_film_create_from_planes: null argument");
        if (!n_local || n_local >= (1ull << 31)) fail(PT_ERR_INVALID, "pt_film_create_from_planes: n_local must be in 1 .. 2^31 - 1");
        if (!samples || samples > (uint64_t)PT_FILM_MAX_SAMPLES)
            fail(PT_ERR_INVALID, "pt_film_create_from_planes: samples must be in 1 .. %u", (unsigned)PT_FILM_MAX_SAMPLES);
        if (!last_pass_samples || last_pass_samples > samples)
            fail(PT_ERR_INVALID, "pt_film_create_from_planes: last_pass_samples must be in 1 .. samples");
        if (device >= 0) HIP_CHECK(hipSetDevice(device));
        else HIP_CHECK(hipGetDevice(&device));
        auto f = film_alloc(device, n_local);
        HIP_CHECK(hipMemcpy(f->accum, accum, n_local * 12u, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(f->moments, moments, n_local * 8u, hipMemcpyHostToDevice));
        f->passes = 1;
        f->last_pass_samples = last_pass_samples;
        f->samples = samples;
        *out = f.release();
    });
}

void pt_film_destroy(pt_film* film) { delete film; }

int pt_film_reset(pt_film* film) {
    return guarded([&] {
        if (!film) fail(PT_ERR_INVALID, "pt_film_reset: null argument");
        HIP_CHECK(hipSetDevice(film->device));
        HIP_CHECK(hipMemset(film->accum, 0, film->stride_a * sizeof(float)));
        HIP_CHECK(hipMemset(film->moments, 0, film->stride_m * sizeof(float)));
        HIP_CHECK(hipDeviceSynchronize());
        if (film->count) {   // uniform again: the count plane goes (the tile arrays and the table's buffer are scratch and stay)
            (void)hipFree(film->count);
            film->count = nullptr;
            film->bytes_adaptive -= film->n_local * 4u;
            film->tile_count.clear();
        }
        film->tile_passes = film->last_pass_tiles = 0;
        film->windows = film->tile_windows = 0;
        film->passes = 0;
        film->last_pass_samples = 0;
        film->samples = 0;
    });
}

int pt_film_get_info(const pt_film* film, pt_film_info* info) {
    return guarded([&] {
        if (!film || !info) fail(PT_ERR_INVALID, "pt_film_get_info: null argument");
        film_fill_info(*film, *info);
    });
}

int pt_film_read(const pt_film* film, float* accum, float* moments) {
    return guarded([&] {
        if (!film) fail(PT_ERR_INVALID, "pt_film_read: null argument");
        HIP_CHECK(hipSetDevice(film->device));
        if (accum) HIP_CHECK(hipMemcpy(accum, film->accum, film->n_local * 12u, hipMemcpyDeviceToHost));
        if (moments) HIP_CHECK(hipMemcpy(moments, film->moments, film->n_local * 8u, hipMemcpyDeviceToHost));
    });
}

int pt_film_planes_device(const pt_film* film, void** d_accum, void** d_moments) {
    return guarded([&] {
        if (!film) fail(PT_ERR_INVALID, "pt_film_planes_device: null argument");
        film_refuse_non_uniform("pt_film_planes_device", film);
        if (d_accum) *d_accum = film->accum;
        if (d_moments) *d_moments = film->moments;
    });
}

int pt_film_add_pass(pt_film* film, const pt_scene* scene, uint32_t samples) {
    return guarded([&] {
        film_check_pass("pt_film_add_pass", film, scene, samples);
        film_add_whole_pass(*film, scene, samples);
    });
}

int pt_film_add_planes(pt_film* film, uint32_t samples, const float* accum, const float* moments) {
    return guarded([&] {
        if (!film || !accum || !moments) fail(PT_ERR_INVALID, "pt_film_add_planes: null argument");
        film_refuse_non_uniform("pt_film_add_planes", film);
        film_check_samples("pt_film_add_planes", film, samples);
        HIP_CHECK(hipSetDevice(film->device));
        HIP_CHECK(hipMemcpy(film->pass_accum, accum, film->n_local * 12u, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(film->pass_moments, moments, film->n_local * 8u, hipMemcpyHostToDevice));
        film_merge(*film, samples);
    });
}

int pt_film_noise(const pt_film* film, float lum_floor, double target, pt_film_noise_stats* out, float* err_host,
                  float* block_sum_host, float* block_max_host) {
    return guarded([&] {
        if (!film || !out) fail(PT_ERR_INVALID, "pt_film_noise: null argument");
        film_refuse_non_uniform("pt_film_noise", film);
        pt_film_noise_stats st{};
        film_noise(*film, lum_floor, target, st, err_host, block_sum_host, block_max_host);
        *out = st;
    });
}

int pt_film_resolve_device(const pt_film* film, int tonemap, void* d_rgb8, void* d_color, void* hip_stream) {
    return guarded([&] {
        film_check_resolve("pt_film_resolve_device", film, tonemap, d_rgb8, d_color);
        HIP_CHECK(hipSetDevice(film->device));
        film_resolve_launch(*film, tonemap, (uint8_t*)d_rgb8, (float*)d_color, (hipStream_t)hip_stream);
    });
}

int pt_film_resolve(const pt_film* film, int tonemap, uint8_t* rgb8, float* color) {
    return guarded([&] {
        film_check_resolve("pt_film_resolve", film, tonemap, rgb8, color);
        HIP_CHECK(hipSetDevice(film->device));
        const size_t n = (size_t)film->n_local * 3u;
        Staged<uint8_t> d_rgb(nullptr, n);
        Staged<float> d_color(nullptr, n);
        film_resolve_launch(*film, tonemap, rgb8 ? d_rgb.d : nullptr, color ? d_color.d : nullptr, nullptr);
        HIP_CHECK(hipDeviceSynchronize());
        if (rgb8) d_rgb.fetch(rgb8, n);
        if (color) d_color.fetch(color, n);
    });
}

int pt_film_render_until(pt_film* film, const pt_scene* scene, uint32_t first_pass_samples, uint64_t max_samples, float lum_floor,
                         double target, pt_film_pass_fn on_pass, void* user, pt_film_noise_stats* out) {
    return guarded([&] {
        if (!film || !scene || !out) fail(PT_ERR_INVALID, "pt_film_render_until: null argument");
        if (!film->has_profile) fail(PT_ERR_INVALID, "pt_film_render_until: a film made from planes has no profile to render with");
        if (film->windowed) fail(PT_ERR_INVALID, "pt_film_render_until: a windowed film takes windows only (pt_film_render_until_windowed)");
        film_refuse_shard("pt_film_render_until", film);
        film_refuse_non_uniform("pt_film_render_until", film);
        film_check_noise_args("pt_film_render_until", lum_floor, target);
        if (first_pass_samples < 2u) fail(PT_ERR_INVALID, "pt_film_render_until: first_pass_samples must be >= 2 (a sample variance needs two)");
        if (!film->passes && (uint64_t)first_pass_samples > max_samples)
            fail(PT_ERR_INVALID, "pt_film_render_until: first_pass_samples %u exceeds max_samples %llu", first_pass_samples, (unsigned long long)max_samples);
        if (scene->device != film->device)
            fail(PT_ERR_INVALID, "pt_film_render_until: the scene is on device %d, the film on device %d", scene->device, film->device);
        const uint64_t cap = std::min<uint64_t>(max_samples, (uint64_t)PT_FILM_MAX_SAMPLES);
        pt_film_noise_stats st{};
        bool measured = false;
        for (;;) {
            const uint64_t next = film->passes ? 2u * (uint64_t)film->last_pass_samples : (uint64_t)first_pass_samples;
            if (film->samples + next > cap) break;
            film_add_pass(*film, scene, (uint32_t)next);
            film_noise(*film, lum_floor, target, st, nullptr, nullptr, nullptr);
            measured = true;
            if (on_pass) {
                pt_film_info info;
                film_fill_info(*film, info);
                on_pass(&info, &st, user);
            }
            if (st.converged) break;
        }
        if (!measured) film_noise(*film, lum_floor, target, st, nullptr, nullptr, nullptr);   // (no pass fits: what the film holds)
        *out = st;
    });
}

int pt_film_kernel_times(const pt_film* film, float lum_floor, int with_err, uint32_t reps, float* ms_merge, float* ms_noise) {
    return guarded([&] {
        if (!film || !ms_merge || !ms_noise || !reps) fail(PT_ERR_INVALID, "pt_film_kernel_times: null argument");
        if (film->samples < 2u) fail(PT_ERR_INVALID, "pt_film_kernel_times: the film's total must be >= 2");
        film_refuse_non_uniform("pt_film_kernel_times", film);
        film_check_noise_args("pt_film_kernel_times", lum_floor, 0.0);
        HIP_CHECK(hipSetDevice(film->device));
        hipEvent_t e0 = nullptr, e1 = nullptr;
        struct Free {
            hipEvent_t &a, &b;
            ~Free() {
                if (a) (void)hipEventDestroy(a);
                if (b) (void)hipEventDestroy(b);
            }
        } guard{e0, e1};
        HIP_CHECK(hipEventCreate(&e0));
        HIP_CHECK(hipEventCreate(&e1));
        for (uint32_t r = 0; r < 2u * reps; ++r) {
            const bool merge = r < reps;
            HIP_CHECK(hipEventRecord(e0, 0));
            if (merge)   // the roles swapped: pass = pass + film (the pass buffers are scratch between passes)
                hipLaunchKernelGGL(k_film_merge, dim3(film_merge_blocks(*film)), dim3(256), 0, 0, (float4*)film->pass_accum,
                                   (const float4*)film->accum, film->stride_a / 4u, (float4*)film->pass_moments,
                                   (const float4*)film->moments, film->stride_m / 4u);
            else
                film_noise_launch(*film, lum_floor, with_err != 0);
            HIP_CHECK(hipEventRecord(e1, 0));
            HIP_CHECK(hipEventSynchronize(e1));
            HIP_CHECK(hipEventElapsedTime(merge ? &ms_merge[r] : &ms_noise[r - reps], e0, e1));
        }
        HIP_CHECK(hipGetLastError());
    });
}

// ---- the adaptive film
int pt_film_add_tile_pass(pt_film* film, const pt_scene* scene, uint32_t samples, const uint32_t* tiles, uint32_t n_tiles) {
    return guarded([&] {
        if (!film || !scene) fail(PT_ERR_INVALID, "pt_film_add_tile_pass: null argument");
        film_add_tile_pass(*film, scene, samples, tiles, n_tiles);
    });
}

int pt_film_add_tile_planes(pt_film* film, uint32_t samples, const uint32_t* tiles, uint32_t n_tiles, const float* accum,
                            const float* moments) {
    return guarded([&] {
        if (!film || !accum || !moments) fail(PT_ERR_INVALID, "pt_film_add_tile_planes: null argument");
        const TileMap listed = film_check_tile_pass("pt_film_add_tile_planes", film, samples, tiles, n_tiles);
        const TileMap tm = film->packed ? film_own_map("pt_film_add_tile_planes", *film, film_own_tiles(*film, listed.tiles)) : listed;
        HIP_CHECK(hipSetDevice(film->device));
        if (tm.n_local) {
            HIP_CHECK(hipMemcpy(film->pass_accum, accum, tm.n_local * 12u, hipMemcpyHostToDevice));
            HIP_CHECK(hipMemcpy(film->pass_moments, moments, tm.n_local * 8u, hipMemcpyHostToDevice));
        }
        film_merge_tiles(*film, tm, listed.tiles, samples);
    });
}

int pt_film_read_counts(const pt_film* film, uint32_t* counts) {
    return guarded([&] {
        if (!film || !counts) fail(PT_ERR_INVALID, "pt_film_read_counts: null argument");
        if (film->uniform()) {
            std::fill(counts, counts + film->n_local, (uint32_t)film->samples);
            return;
        }
        HIP_CHECK(hipSetDevice(film->device));
        HIP_CHECK(hipMemcpy(counts, film->count, film->n_local * 4u, hipMemcpyDeviceToHost));
    });
}

int pt_film_tile_noise(const pt_film* film, float lum_floor, double target, pt_film_tile_stats* out, float* err_host,
                       float* tile_sum_host, float* tile_max_host) {
    return guarded([&] {
        if (!film || !out) fail(PT_ERR_INVALID, "pt_film_tile_noise: null argument");
        pt_film_tile_stats st{};
        film_tile_noise(*film, lum_floor, target, st, err_host, tile_sum_host, tile_max_host);
        *out = st;
    });
}

int pt_film_get_adaptive_info(const pt_film* film, pt_film_adaptive_info* out) {
    return guarded([&] {
        if (!film || !out) fail(PT_ERR_INVALID, "pt_film_get_adaptive_info: null argument");
        film_check_tiled("pt_film_get_adaptive_info", film);
        const FilmTiling T = film_tiling(*film);
        memset(out, 0, sizeof *out);
        out->uniform = film->uniform() ? 1u : 0u;
        out->tile_w = T.tile_w;
        out->tile_h = T.tile_h;
        out->tiles_x = T.tiles_x;
        out->tiles_y = (T.height + T.tile_h - 1u) / T.tile_h;
        out->n_tiles = out->tiles_x * out->tiles_y;
        out->tile_passes = film->tile_passes;
        out->last_pass_tiles = film->last_pass_tiles ? film->last_pass_tiles : film->passes ? out->n_tiles : 0u;
        out->max_samples = film->samples;
        out->min_samples = film->uniform() ? film->samples : *std::min_element(film->tile_count.begin(), film->tile_count.end());
        for (uint32_t t = 0; t < out->n_tiles; ++t)
            out->pixel_samples += film_tile_pixels(T, t) * (film->uniform() ? film->samples : film->tile_count[t]);
        out->device_bytes = film->bytes + film->bytes_adaptive + film->bytes_filter;
    });
}

void pt_film_adaptive_params_default(pt_film_adaptive_params* p) {
    if (!p) return;
    memset(p, 0, sizeof *p);
    p->lum_floor = PT_FILM_DEFAULT_LUM_FLOOR;
    p->target = 0.02;
    p->first_pass_samples = 8;
    p->uniform_samples = 24;
    p->dilate = 1;
    p->max_samples = 512;
}

int pt_film_render_until_adaptive(pt_film* film, const pt_scene* scene, const pt_film_adaptive_params* params,
                                  pt_film_pass_fn on_pass, void* user, pt_film_tile_stats* out) {
    return guarded([&] {
        const char* who = "pt_film_render_until_adaptive";
        if (!film || !scene || !params || !out) fail(PT_ERR_INVALID, "%s: null argument", who);
        film_refuse_shard(who, film);
        film_check_adaptive(who, film, scene, params);
        film_adaptive_loop(film, scene, params, on_pass, user, out,
                           [&](pt_film_tile_stats& st, float* sums) {
                               film_tile_noise(*film, params->lum_floor, params->target, st, nullptr, sums, nullptr);
                           });
    });
}

// ---- windowed films
int pt_film_create_windowed(int device, const pt_profile* profile, const pt_opts* opts, pt_film** out) {
    if (profile && out && (profile->samples < 2u || profile->samples > PT_FILM_MAX_SAMPLES))
        return guarded([&] {
            fail(PT_ERR_INVALID, "pt_film_create_windowed: the enumeration (profile.samples) must be in 2 .. %u (got %u)",
                 (unsigned)PT_FILM_MAX_SAMPLES, profile->samples);
        });
    const int rc = pt_film_create(device, profile, opts, out);
    if (rc == PT_OK) {
        (*out)->windowed = true;
        (*out)->enum_n = profile->samples;
    }
    return rc;
}

int pt_film_add_window(pt_film* film, const pt_scene* scene, uint32_t samples) {
    return guarded([&] {
        film_check_window("pt_film_add_window", film, scene, samples);
        film_add_window(*film, scene, samples);
    });
}

int pt_film_add_tile_window(pt_film* film, const pt_scene* scene, uint32_t samples, const uint32_t* tiles, uint32_t n_tiles) {
    return guarded([&] {
        film_check_window("pt_film_add_tile_window", film, scene, samples);
        film_add_tile_window(*film, scene, samples, tiles, n_tiles);
    });
}

int pt_film_get_window_info(const pt_film* film, pt_film_window_info* out) {
    return guarded([&] {
        if (!film || !out) fail(PT_ERR_INVALID, "pt_film_get_window_info: null argument");
        memset(out, 0, sizeof *out);
        out->windowed = film->windowed ? 1u : 0u;
        out->enumeration = film->enum_n;
        out->windows = film->windows;
        out->tile_windows = film->tile_windows;
    });
}

void pt_film_window_params_default(pt_film_window_params* p) {
    if (!p) return;
    memset(p, 0, sizeof *p);
    p->lum_floor = PT_FILM_DEFAULT_LUM_FLOOR;
    p->target = 0.02;
    p->window_samples = PT_FILM_DEFAULT_WINDOW_SAMPLES;
    p->adaptive = 1;
    p->uniform_samples = 24;
    p->dilate = 1;
}

int pt_film_render_until_windowed(pt_film* film, const pt_scene* scene, const pt_film_window_params* params, pt_film_pass_fn on_pass,
                                  void* user, pt_film_tile_stats* out) {
    return guarded([&] {
        const char* who = "pt_film_render_until_windowed";
        if (!film || !scene || !params || !out) fail(PT_ERR_INVALID, "%s: null argument", who);
        film_refuse_shard(who, film);
        film_check_window_params(who, film, scene, params);
        film_window_loop(film, scene, params, on_pass, user, out, [&](pt_film_tile_stats& st, float* sums) {
            film_tile_noise(*film, params->lum_floor, params->target, st, nullptr, sums, nullptr);
        });
    });
}

int pt_film_window_kernel_times(pt_film* film, uint32_t reps, float* ms_gather, float* ms_scatter) {
    return guarded([&] {
        const char* who = "pt_film_window_kernel_times";
        if (!film || !ms_gather || !ms_scatter || !reps) fail(PT_ERR_INVALID, "%s: null argument", who);
        film_check_tiled(who, film);
        if (film->uniform()) fail(PT_ERR_INVALID, "%s: the film has taken no tile window", who);
        HIP_CHECK(hipSetDevice(film->device));
        // every tile the film holds (a shard film: its own, through the packed variants)
        const TileMap tm = film_own_map(who, *film, film_own_tiles(*film, film_all_tiles(*film)));
        const uint32_t n_tiles = tm.n_local_tiles;
        film_upload_table(*film, tm);
        hipEvent_t e0 = nullptr, e1 = nullptr;
        struct Free {
            hipEvent_t &a, &b;
            ~Free() {
                if (a) (void)hipEventDestroy(a);
                if (b) (void)hipEventDestroy(b);
            }
        } guard{e0, e1};
        HIP_CHECK(hipEventCreate(&e0));
        HIP_CHECK(hipEventCreate(&e1));
        // gather every tile, then scatter what was gathered with zero samples: every load and store of a real tile window, and
        // the film's planes and counts as they were
        for (uint32_t r = 0; r < reps; ++r) {
            HIP_CHECK(hipEventRecord(e0, 0));
            film_launch_gather_tiles(*film, n_tiles, film->pass_accum, film->pass_moments);
            HIP_CHECK(hipEventRecord(e1, 0));
            HIP_CHECK(hipEventSynchronize(e1));
            HIP_CHECK(hipEventElapsedTime(&ms_gather[r], e0, e1));
            HIP_CHECK(hipEventRecord(e0, 0));
            film_launch_scatter_tiles(*film, n_tiles, film->pass_accum, film->pass_moments, 0u);
            HIP_CHECK(hipEventRecord(e1, 0));
            HIP_CHECK(hipEventSynchronize(e1));
            HIP_CHECK(hipEventElapsedTime(&ms_scatter[r], e0, e1));
        }
        HIP_CHECK(hipGetLastError());
    });
}

int pt_film_adaptive_kernel_times(pt_film* film, float lum_floor, int tonemap, uint32_t reps, float* ms_merge, float* ms_noise,
                                  float* ms_resolve) {
    return guarded([&] {
        const char* who = "pt_film_adaptive_kernel_times";
        if (!film || !ms_merge || !ms_noise || !ms_resolve || !reps) fail(PT_ERR_INVALID, "%s: null argument", who);
        film_check_tiled(who, film);
        film_check_noise_args(who, lum_floor, 0.0);
        film_check_resolve(who, film, tonemap, ms_resolve, nullptr);
        if (film->uniform()) fail(PT_ERR_INVALID, "%s: the film has taken no tile pass", who);
        if (*std::min_element(film->tile_count.begin(), film->tile_count.end()) < 2u) fail(PT_ERR_INVALID, "%s: every pixel needs >= 2 samples", who);
        HIP_CHECK(hipSetDevice(film->device));
        const uint32_t n_tiles = film_n_tiles(*film);
        if (!film->tile_sum) {
            HIP_CHECK(hipMalloc((void**)&film->tile_sum, (size_t)n_tiles * 8u));
            film->bytes_adaptive += (uint64_t)n_tiles * 8u;
        }
        // the merge of a pass of zeros and zero samples over every tile: every load, addition and store of a real pass, and the
        // film's planes as they were (x + 0 = x for every x a sum of radiances can be)
        // (every tile the film holds: a shard film's own, through the packed variants)
        const TileMap tm = film_own_map(who, *film, film_own_tiles(*film, film_all_tiles(*film)));
        film_upload_table(*film, tm);
        HIP_CHECK(hipMemset(film->pass_accum, 0, film->stride_a * sizeof(float)));
        HIP_CHECK(hipMemset(film->pass_moments, 0, film->stride_m * sizeof(float)));
        Staged<uint8_t> d_rgb(nullptr, (size_t)film->n_local * 3u);
        hipEvent_t e0 = nullptr, e1 = nullptr;
        struct Free {
            hipEvent_t &a, &b;
            ~Free() {
                if (a) (void)hipEventDestroy(a);
                if (b) (void)hipEventDestroy(b);
            }
        } guard{e0, e1};
        HIP_CHECK(hipEventCreate(&e0));
        HIP_CHECK(hipEventCreate(&e1));
        for (uint32_t r = 0; r < 3u * reps; ++r) {
            const uint32_t which = r / reps;
            HIP_CHECK(hipEventRecord(e0, 0));
            if (which == 0)
                film_launch_merge_tiles(*film, tm.n_local_tiles, film->pass_accum, film->pass_moments, 0u);
            else if (which == 1)
                film_launch_tile_noise(*film, lum_floor, film->err, film->tile_sum, film->tile_sum + n_tiles);
            else
                hipLaunchKernelGGL(k_film_post_counts, dim3(((uint32_t)film->n_local + 255u) / 256u), dim3(256), 0, 0,
                                   (const float*)film->accum, (const uint32_t*)film->count, d_rgb.d, (uint32_t)film->n_local, tonemap);
            HIP_CHECK(hipEventRecord(e1, 0));
            HIP_CHECK(hipEventSynchronize(e1));
            HIP_CHECK(hipEventElapsedTime(which == 0 ? &ms_merge[r] : which == 1 ? &ms_noise[r - reps] : &ms_resolve[r - 2u * reps], e0, e1));
        }
        HIP_CHECK(hipGetLastError());
    });
}

// ---- sharded films
int pt_film_create_shard(int device, const pt_profile* profile, const pt_opts* opts, uint32_t windowed, pt_film** out) {
    if (windowed > 1u) return guarded([&] { fail(PT_ERR_INVALID, "pt_film_create_shard: windowed must be 0 or 1"); });
    const int rc = windowed ? pt_film_create_windowed(device, profile, opts, out) : pt_film_create(device, profile, opts, out);
    if (rc != PT_OK) return rc;
    const int rc_shard = guarded([&] {
        pt_film& f = **out;
        f.shard = true;
        f.packed = f.opts.shard_count > 1;
        if (!f.packed) return;
        const TileMap tm = make_tile_map(f.profile, f.opts, f.opts.shard_rank);
        f.base_of.assign(film_n_tiles(f), (uint32_t)FILM_NOT_OWNED);
        for (uint32_t lt = 0; lt < tm.n_local_tiles; ++lt) f.base_of[tm.tiles[lt]] = tm.offsets[lt];
        HIP_CHECK(hipSetDevice(f.device));
        f.base_dev.ensure(f.base_of.size() * 4u);
        f.bytes_adaptive += f.base_dev.bytes;
        HIP_CHECK(hipMemcpy(f.base_dev.p, f.base_of.data(), f.base_of.size() * 4u, hipMemcpyHostToDevice));
    });
    if (rc_shard != PT_OK) {
        delete *out;
        *out = nullptr;
    }
    return rc_shard;
}

int pt_film_get_shard_info(const pt_film* film, pt_film_shard_info* out) {
    return guarded([&] {
        if (!film || !out) fail(PT_ERR_INVALID, "pt_film_get_shard_info: null argument");
        memset(out, 0, sizeof *out);
        out->shard = film->shard ? 1u : 0u;
        out->rank = film->opts.shard_rank;
        out->count = film->has_profile ? film->opts.shard_count : 0u;
        if (!film->has_profile) return;
        out->n_tiles = film_n_tiles(*film);
        out->own_tiles = make_tile_map(film->profile, film->opts, film->opts.shard_rank).n_local_tiles;
        out->n_pixels = (uint64_t)film->profile.width * film->profile.height;
    });
}

int pt_film_shard_tile_noise(const pt_film* film, float lum_floor, float* tile_sum, float* tile_max, float* err_host) {
    return guarded([&] {
        if (!film || !tile_sum || !tile_max) fail(PT_ERR_INVALID, "pt_film_shard_tile_noise: null argument");
        film_shard_tile_noise(*film, lum_floor, tile_sum, tile_max, err_host);
    });
}

int pt_film_tile_stats_from_sums(const pt_film* film, const float* tile_sum, double target, pt_film_tile_stats* out) {
    return guarded([&] {
        const char* who = "pt_film_tile_stats_from_sums";
        if (!film || !tile_sum || !out) fail(PT_ERR_INVALID, "%s: null argument", who);
        if (!film->has_profile) fail(PT_ERR_INVALID, "%s: a film made from planes has no tiling", who);
        film_check_noise_args(who, 1.f, target);
        pt_film_tile_stats st{};
        film_tile_stats(*film, std::vector<float>(tile_sum, tile_sum + film_n_tiles(*film)), target, st);
        *out = st;
    });
}

int pt_film_select_tiles(const pt_film* film, const float* tile_sum, double target, uint32_t dilate, uint32_t* tiles, uint32_t* n_out) {
    return guarded([&] {
        const char* who = "pt_film_select_tiles";
        if (!film || !tile_sum || !tiles || !n_out) fail(PT_ERR_INVALID, "%s: null argument", who);
        if (!film->has_profile) fail(PT_ERR_INVALID, "%s: a film made from planes has no tiling", who);
        film_check_noise_args(who, 1.f, target);
        if (dilate > 1u) fail(PT_ERR_INVALID, "%s: dilate must be 0 or 1", who);
        std::vector<uint32_t> active;
        film_select_active(film_tiling(*film), std::vector<float>(tile_sum, tile_sum + film_n_tiles(*film)), target, dilate, active);
        std::copy(active.begin(), active.end(), tiles);
        *n_out = (uint32_t)active.size();
    });
}

int pt_film_render_until_adaptive_sharded(pt_film* film, const pt_scene* scene, const pt_film_adaptive_params* params,
                                          pt_film_exchange_fn exchange, void* exchange_user, pt_film_pass_fn on_pass, void* user,
                                          pt_film_tile_stats* out) {
    return guarded([&] {
        const char* who = "pt_film_render_until_adaptive_sharded";
        if (!film || !scene || !params || !out) fail(PT_ERR_INVALID, "%s: null argument", who);
        film_check_sharded_loop(who, film, exchange);
        film_check_adaptive(who, film, scene, params);
        film_adaptive_loop(film, scene, params, on_pass, user, out,
                           ShardNoise{who, film, params->lum_floor, params->target, exchange, exchange_user});
    });
}

int pt_film_render_until_windowed_sharded(pt_film* film, const pt_scene* scene, const pt_film_window_params* params,
                                          pt_film_exchange_fn exchange, void* exchange_user, pt_film_pass_fn on_pass, void* user,
                                          pt_film_tile_stats* out) {
    return guarded([&] {
        const char* who = "pt_film_render_until_windowed_sharded";
        if (!film || !scene || !params || !out) fail(PT_ERR_INVALID, "%s: null argument", who);
        film_check_sharded_loop(who, film, exchange);
        film_check_window_params(who, film, scene, params);
        film_window_loop(film, scene, params, on_pass, user, out,
                         ShardNoise{who, film, params->lum_floor, params->target, exchange, exchange_user});
    });
}

int pt_film_assemble(pt_film* whole, const pt_film* const* shards, uint32_t n) {
    return guarded([&] {
        if (!whole) fail(PT_ERR_INVALID, "pt_film_assemble: null argument");
        film_assemble(*whole, shards, n);
    });
}

// ---- the film filter
uint64_t pt_film_denoise_scratch_bytes(const pt_film* film) {
    if (!film || !film->has_profile || film->opts.shard_count > 1 || film->shard) return 0;
    return fdn_scratch_layout(*film).total;
}

int pt_film_denoise_device(const pt_film* film, int variance, const pt_denoise_params* params, float lum_floor, const void* d_guides,
                           void* d_out_color, void* d_out_rgb8, void* d_out_ferr, void* d_scratch, void* hip_stream) {
    return guarded([&] {
        const char* who = "pt_film_denoise_device";
        if (!film || !params || !d_guides || (!d_out_color && !d_out_rgb8 && !d_out_ferr)) fail(PT_ERR_INVALID, "%s: null argument", who);
        fdn_check(who, film, variance, params, lum_floor, d_out_ferr != nullptr);
        if (!d_scratch && params->iterations) fail(PT_ERR_INVALID, "%s: null argument", who);
        HIP_CHECK(hipSetDevice(film->device));
        fdn_launch(*film, variance, *params, lum_floor, (const float4*)d_guides, (float*)d_out_color, (uint8_t*)d_out_rgb8,
                   (float*)d_out_ferr, (uint8_t*)d_scratch, (hipStream_t)hip_stream);
    });
}

int pt_film_denoise(const pt_film* film, const pt_scene* scene, int variance, const pt_denoise_params* params, float lum_floor,
                    uint8_t* rgb8, float* color, float* ferr) {
    return guarded([&] {
        const char* who = "pt_film_denoise";
        if (!film || !scene || !params || (!rgb8 && !color && !ferr)) fail(PT_ERR_INVALID, "%s: null argument", who);
        fdn_check(who, film, variance, params, lum_floor, ferr != nullptr);
        fdn_check_scene(who, film, scene);
        HIP_CHECK(hipSetDevice(film->device));
        const size_t n = (size_t)film->n_local;
        uint8_t* scratch = film_filter_scratch(*film);
        float4* d_guides = film_filter_guides(*film);
        // only the planes that were asked for are staged (ferr: the scratch has a plane for it)
        std::unique_ptr<Staged<uint8_t>> d_rgb;
        std::unique_ptr<Staged<float>> d_color;
        if (rgb8) d_rgb = std::make_unique<Staged<uint8_t>>(nullptr, n * 3);
        if (color) d_color = std::make_unique<Staged<float>>(nullptr, n * 3);
        float* d_ferr = ferr ? (float*)(scratch + fdn_scratch_layout(*film).ferr) : nullptr;
        guides_launch(*scene, film->profile.width, film->profile.height, d_guides, nullptr);
        fdn_launch(*film, variance, *params, lum_floor, d_guides, color ? d_color->d : nullptr, rgb8 ? d_rgb->d : nullptr, d_ferr,
                   scratch, nullptr);
        HIP_CHECK(hipDeviceSynchronize());
        if (rgb8) d_rgb->fetch(rgb8, n * 3);
        if (color) d_color->fetch(color, n * 3);
        if (ferr) HIP_CHECK(hipMemcpy(ferr, d_ferr, n * sizeof(float), hipMemcpyDeviceToHost));
    });
}

int pt_film_tile_reduce_device(const pt_film* film, const void* d_err, void* d_tile_sum, void* d_tile_max, void* hip_stream) {
    return guarded([&] {
        const char* who = "pt_film_tile_reduce_device";
        if (!film || !d_err || !d_tile_sum || !d_tile_max) fail(PT_ERR_INVALID, "%s: null argument", who);
        film_check_tiled(who, film);
        film_refuse_shard(who, film);
        HIP_CHECK(hipSetDevice(film->device));
        fdn_tile_reduce_launch(*film, (const float*)d_err, (float*)d_tile_sum, (float*)d_tile_max, (hipStream_t)hip_stream);
    });
}

int pt_film_filtered_noise(const pt_film* film, const pt_scene* scene, const pt_denoise_params* params, float lum_floor, double target,
                           pt_film_tile_stats* out, float* ferr_host, float* tile_sum_host, float* tile_max_host) {
    return guarded([&] {
        const char* who = "pt_film_filtered_noise";
        if (!film || !scene || !params || !out) fail(PT_ERR_INVALID, "%s: null argument", who);
        fdn_check(who, film, 1, params, lum_floor, true);
        film_check_noise_args(who, lum_floor, target);
        fdn_check_scene(who, film, scene);
        HIP_CHECK(hipSetDevice(film->device));
        float4* d_guides = film_filter_guides(*film);
        guides_launch(*scene, film->profile.width, film->profile.height, d_guides, nullptr);
        pt_film_tile_stats st{};
        film_filtered_noise(*film, d_guides, *params, lum_floor, target, st, ferr_host, tile_sum_host, tile_max_host);
        *out = st;
    });
}

void pt_film_filtered_params_default(pt_film_filtered_params* p) {
    if (!p) return;
    pt_film_adaptive_params_default(&p->adaptive);
    pt_denoise_var_params_default(&p->filter);
}

int pt_film_render_until_filtered(pt_film* film, const pt_scene* scene, const pt_film_filtered_params* params,
                                  pt_film_pass_fn on_pass, void* user, pt_film_tile_stats* out) {
    return guarded([&] {
        const char* who = "pt_film_render_until_filtered";
        if (!film || !scene || !params || !out) fail(PT_ERR_INVALID, "%s: null argument", who);
        const pt_film_adaptive_params& a = params->adaptive;
        film_refuse_shard(who, film);
        film_check_adaptive(who, film, scene, &a);
        dnv_check(who, &params->filter, film->profile.width, film->profile.height, 2u);
        // A film that is measured as it stands - it has its uniform samples, or no pass fits the budget - must pass the filter's
        // count rule now, before the scratch is made and the guides are rendered; any other film takes a whole pass of >= 2 first.
        const uint64_t next = film->passes ? 2u * (uint64_t)film->last_pass_samples : (uint64_t)a.first_pass_samples;
        const bool measure_first = film->passes && film->samples >= 2u && film->samples >= a.uniform_samples;
        const bool pass_fits = film->samples + next <= std::min<uint64_t>(a.max_samples, (uint64_t)PT_FILM_MAX_SAMPLES);
        if (measure_first || !pass_fits) fdn_check(who, film, 1, &params->filter, a.lum_floor, true);
        HIP_CHECK(hipSetDevice(film->device));
        float4* d_guides = film_filter_guides(*film);   // rendered once: the film does not watch the scene
        guides_launch(*scene, film->profile.width, film->profile.height, d_guides, nullptr);
        film_adaptive_loop(film, scene, &a, on_pass, user, out, [&](pt_film_tile_stats& st, float* sums) {
            fdn_check(who, film, 1, &params->filter, a.lum_floor, true);
            film_filtered_noise(*film, d_guides, params->filter, a.lum_floor, a.target, st, nullptr, sums, nullptr);
        });
    });
}

int pt_film_denoise_kernel_times(const pt_film* film, const pt_scene* scene, const pt_denoise_params* params, float lum_floor,
                                 uint32_t reps, float* ms_prep, float* ms_passes, float* ms_finish, float* ms_reduce) {
    return guarded([&] {
        const char* who = "pt_film_denoise_kernel_times";
        if (!film || !scene || !params || !reps || !ms_prep || !ms_passes || !ms_finish || !ms_reduce) fail(PT_ERR_INVALID, "%s: null argument", who);
        fdn_check(who, film, 1, params, lum_floor, true);
        fdn_check_scene(who, film, scene);
        HIP_CHECK(hipSetDevice(film->device));
        uint8_t* scratch = film_filter_scratch(*film);
        float4* d_guides = film_filter_guides(*film);
        const FdnScratch L = fdn_scratch_layout(*film);
        guides_launch(*scene, film->profile.width, film->profile.height, d_guides, nullptr);
        std::vector<hipEvent_t> ev(5, nullptr);
        struct Free {
            std::vector<hipEvent_t>& e;
            ~Free() {
                for (hipEvent_t x : e)
                    if (x) (void)hipEventDestroy(x);
            }
        } guard{ev};
        for (hipEvent_t& x : ev) HIP_CHECK(hipEventCreate(&x));
        for (uint32_t r = 0; r < reps; ++r) {
            fdn_launch(*film, 1, *params, lum_floor, d_guides, nullptr, nullptr, (float*)(scratch + L.ferr), scratch, nullptr, ev.data());
            fdn_tile_reduce_launch(*film, (const float*)(scratch + L.ferr), (float*)(scratch + L.tile_sum), (float*)(scratch + L.tile_max), nullptr);
            HIP_CHECK(hipEventRecord(ev[4], nullptr));
            HIP_CHECK(hipEventSynchronize(ev[4]));
            HIP_CHECK(hipEventElapsedTime(&ms_prep[r], ev[0], ev[1]));
            HIP_CHECK(hipEventElapsedTime(&ms_passes[r], ev[1], ev[2]));
            HIP_CHECK(hipEventElapsedTime(&ms_finish[r], ev[2], ev[3]));
            HIP_CHECK(hipEventElapsedTime(&ms_reduce[r], ev[3], ev[4]));
        }
    });
}

int pt_render_moments_device(const pt_scene* scene, const pt_profile* profile, const pt_opts* opts, void* d_rgb8,
                             void* d_accum, void* d_moments, void* hip_stream) {
    return guarded([&] {
        if (!scene || !profile || !d_moments) fail(PT_ERR_INVALID, "pt_render_moments_device: null argument");
        moments_check_opts("pt_render_moments_device", opts);
        FrameTaps taps;
        taps.moments = (float2*)d_moments;
        render_device(render_state(scene), *profile, opts, d_rgb8, d_accum, (hipStream_t)hip_stream, false, &taps);
    });
}

int pt_render_moments(const pt_scene* scene, const pt_profile* profile, const pt_opts* opts, uint8_t* rgb8, float* accum,
                      float* moments) {
    return guarded([&] {
        if (!scene || !profile || !moments) fail(PT_ERR_INVALID, "pt_render_moments: null argument");
        moments_check_opts("pt_render_moments", opts);
        HIP_CHECK(hipSetDevice(scene->device));
        pt_opts o;
        normalise_opts(*profile, opts, o);
        uint64_t n = make_tile_map(*profile, o, o.shard_rank).n_local;
        Staged<uint8_t> d_rgb(nullptr, n * 3);
        Staged<float> d_acc(nullptr, n * 3);
        Staged<float2> d_mom(nullptr, n);
        FrameTaps taps;
        taps.moments = d_mom.d;
        render_device(render_state(scene), *profile, opts, d_rgb.d, d_acc.d, nullptr, true, &taps);
        HIP_CHECK(hipDeviceSynchronize());
        if (rgb8) d_rgb.fetch(rgb8, n * 3);
        if (accum) d_acc.fetch(accum, n * 3);
        d_mom.fetch((float2*)moments, n);
    });
}

int pt_render_samples(const pt_scene* scene, const pt_profile* profile, const pt_opts* opts, float* samples) {
    return guarded([&] {
        if (!scene || !profile || !samples) fail(PT_ERR_INVALID, "pt_render_samples: null argument");
        moments_check_opts("pt_render_samples", opts);
        pt_opts o;
        normalise_opts(*profile, opts, o);
        const uint64_t n = make_tile_map(*profile, o, o.shard_rank).n_local;
        if (n && (uint64_t)profile->samples > (256ull << 20) / (n * 12u))
            fail(PT_ERR_INVALID, "pt_render_samples: %u planes of %llu pixels exceed 256 MiB", profile->samples, (unsigned long long)n);
        HIP_CHECK(hipSetDevice(scene->device));
        Staged<float> d_samples(nullptr, (size_t)profile->samples * n * 3);
        FrameTaps taps;
        taps.samples = d_samples.d;
        render_device(render_state(scene), *profile, opts, nullptr, nullptr, nullptr, false, &taps);
        HIP_CHECK(hipDeviceSynchronize());
        d_samples.fetch(samples, (size_t)profile->samples * n * 3);
    });
}

void pt_denoise_var_params_default(pt_denoise_params* p) {
    if (!p) return;
    // the winner of tools/measure_denoise_var_gain.py (tests/golden/denoise_var_gain.json)
    p->iterations = PT_DENOISE_VAR_DEFAULT_ITERATIONS;
    p->flags = PT_DENOISE_VAR_DEFAULT_FLAGS;
    p->normal_power_log2 = PT_DENOISE_VAR_DEFAULT_NORMAL_POWER_LOG2;
    p->tonemap = PT_TONEMAP_FILMIC;
    p->sigma_color = PT_DENOISE_VAR_DEFAULT_SIGMA_COLOR;
    p->sigma_depth = PT_DENOISE_VAR_DEFAULT_SIGMA_DEPTH;
}

uint64_t pt_denoise_var_scratch_bytes(uint32_t width, uint32_t height) { return pt_denoise_scratch_bytes(width, height); }

int pt_denoise_var_device(int device, uint32_t width, uint32_t height, uint32_t samples, const pt_denoise_params* params,
                          const void* d_accum, const void* d_moments, const void* d_guides, void* d_out_color,
                          void* d_out_rgb8, void* d_scratch, void* hip_stream) {
    return guarded([&] {
        dnv_check("pt_denoise_var_device", params, width, height, samples);
        if (!d_accum || !d_moments || !d_guides || (!d_scratch && params->iterations)) fail(PT_ERR_INVALID, "pt_denoise_var_device: null argument");
        if (device >= 0) HIP_CHECK(hipSetDevice(device));
        denoise_var_launch(width, height, samples, *params, (const float*)d_accum, (const float2*)d_moments, (const float4*)d_guides,
                           (float*)d_out_color, (uint8_t*)d_out_rgb8, (uint8_t*)d_scratch, (hipStream_t)hip_stream);
    });
}

int pt_denoise_var(int device, uint32_t width, uint32_t height, uint32_t samples, const pt_denoise_params* params,
                   const float* accum, const float* moments, const float* guides, float* out_color, uint8_t* out_rgb8) {
    return guarded([&] {
        dnv_check("pt_denoise_var", params, width, height, samples);
        if (!accum || !moments || !guides) fail(PT_ERR_INVALID, "pt_denoise_var: null argument");
        if (device >= 0) HIP_CHECK(hipSetDevice(device));
        const size_t n = (size_t)width * height;
        Staged<float> d_acc(accum, n * 3), d_color(nullptr, n * 3);
        Staged<float2> d_mom((const float2*)moments, n);
        Staged<float4> d_guides((const float4*)guides, n * 2);
        Staged<uint8_t> d_rgb(nullptr, n * 3), d_scratch(nullptr, pt_denoise_var_scratch_bytes(width, height));
        denoise_var_launch(width, height, samples, *params, d_acc.d, d_mom.d, d_guides.d, d_color.d, d_rgb.d, d_scratch.d, nullptr);
        HIP_CHECK(hipDeviceSynchronize());
        if (out_color) d_color.fetch(out_color, n * 3);
        if (out_rgb8) d_rgb.fetch(out_rgb8, n * 3);
    });
}

int pt_denoise_var_stage_times(int device, uint32_t width, uint32_t height, uint32_t samples, const pt_denoise_params* params,
                               const void* d_accum, const void* d_moments, const void* d_guides, void* d_out_color,
                               void* d_out_rgb8, void* d_scratch, float* ms) {
    return guarded([&] {
        dnv_check("pt_denoise_var_stage_times", params, width, height, samples);
        if (!d_accum || !d_moments || !d_guides || !ms || (!d_scratch && params->iterations)) fail(PT_ERR_INVALID, "pt_denoise_var_stage_times: null argument");
        if (device >= 0) HIP_CHECK(hipSetDevice(device));
        const size_t n_ev = params->iterations ? params->iterations + 3u : 2u;
        std::vector<hipEvent_t> ev(n_ev, nullptr);
        struct Free {
            std::vector<hipEvent_t>& e;
            ~Free() {
                for (hipEvent_t x : e)
                    if (x) (void)hipEventDestroy(x);
            }
        } guard{ev};
        for (hipEvent_t& x : ev) HIP_CHECK(hipEventCreate(&x));
        denoise_var_launch(width, height, samples, *params, (const float*)d_accum, (const float2*)d_moments, (const float4*)d_guides,
                           (float*)d_out_color, (uint8_t*)d_out_rgb8, (uint8_t*)d_scratch, nullptr, ev.data());
        HIP_CHECK(hipDeviceSynchronize());
        for (int k = 0; k < PT_DENOISE_STAGES; ++k) ms[k] = 0.f;
        if (params->iterations == 0) {
            HIP_CHECK(hipEventElapsedTime(&ms[PT_DENOISE_STAGES - 1], ev[0], ev[1]));
            return;
        }
        HIP_CHECK(hipEventElapsedTime(&ms[0], ev[0], ev[1]));
        for (uint32_t i = 0; i < params->iterations; ++i) HIP_CHECK(hipEventElapsedTime(&ms[1 + i], ev[1 + i], ev[2 + i]));
        HIP_CHECK(hipEventElapsedTime(&ms[PT_DENOISE_STAGES - 1], ev[1 + params->iterations], ev[2 + params->iterations]));
    });
}

int pt_render_denoised_var(const pt_scene* scene, const pt_profile* profile, const pt_opts* opts, const pt_denoise_params* params,
                           uint8_t* rgb8, float* color) {
    return guarded([&] {
        if (!scene || !profile) fail(PT_ERR_INVALID, "pt_render_denoised_var: null argument");
        dnv_check("pt_render_denoised_var", params, profile->width, profile->height, profile->samples);
        moments_check_opts("pt_render_denoised_var", opts);
        pt_opts o;
        normalise_opts(*profile, opts, o);
        if (o.shard_count > 1) fail(PT_ERR_UNSUPPORTED, "pt_render_denoised_var: the filter needs the whole image (shard_count %u)", o.shard_count);
        HIP_CHECK(hipSetDevice(scene->device));
        const uint32_t w = profile->width, h = profile->height;
        const size_t n = (size_t)w * h;
        Staged<uint8_t> d_rgb(nullptr, n * 3), d_scratch(nullptr, pt_denoise_var_scratch_bytes(w, h));
        Staged<float> d_acc(nullptr, n * 3), d_color(nullptr, n * 3);
        Staged<float2> d_mom(nullptr, n);
        Staged<float4> d_guides(nullptr, n * 2);
        FrameTaps taps;
        taps.moments = d_mom.d;
        // the raw frame with its moments (its rgb8 feeds the preview callback only), then guides and filter on the same stream
        render_device(render_state(scene), *profile, opts, d_rgb.d, d_acc.d, nullptr, true, &taps);
        guides_launch(*scene, w, h, d_guides.d, nullptr);
        denoise_var_launch(w, h, profile->samples, *params, d_acc.d, d_mom.d, d_guides.d, color ? d_color.d : nullptr,
                           rgb8 ? d_rgb.d : nullptr, d_scratch.d, nullptr);
        HIP_CHECK(hipDeviceSynchronize());
        if (rgb8) d_rgb.fetch(rgb8, n * 3);
        if (color) d_color.fetch(color, n * 3);
    });
}

int pt_assemble_tiles(const pt_profile* profile, uint32_t shard_count, uint32_t tile_w, uint32_t tile_h,
                      uint64_t slice_pixels, uint32_t elem_bytes, const void* d_gathered, void* d_image,
                      void* hip_stream) {
    return guarded([&] {
        if (!profile || !d_gathered || !d_image) fail(PT_ERR_INVALID, "pt_assemble_tiles: null argument");
        pt_opts o{};
        o.shard_count = shard_count;
        o.tile_w = tile_w;
        o.tile_h = tile_h;
        pt_opts on;
        normalise_opts(*profile, &o, on);
        if (on.shard_count <= 1) {
            HIP_CHECK(hipMemcpyAsync(d_image, d_gathered, (size_t)profile->width * profile->height * elem_bytes,
                                     hipMemcpyDeviceToDevice, (hipStream_t)hip_stream));
            return;
        }
        // rank/tile offset table: built once per (resolution, shard count, tile size, device) and kept on the
        // device, so the per-frame call is a single kernel launch with no allocation and no host sync
        struct Cached {
            uint32_t* d = nullptr;
            uint32_t max_local = 0, tiles_x = 0;
        };
        static std::map<std::tuple<uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, int>, Cached> cache;
        static std::mutex cache_mutex;
        int dev = 0;
        HIP_CHECK(hipGetDevice(&dev));
        Cached c;
        {
            std::lock_guard<std::mutex> lock(cache_mutex);
            auto key = std::make_tuple(profile->width, profile->height, on.shard_count, on.tile_w, on.tile_h, dev);
            auto it = cache.find(key);
            if (it == cache.end()) {
                std::vector<uint32_t> table;
                for (uint32_t r = 0; r < on.shard_count; ++r) {
                    TileMap tm = make_tile_map(*profile, on, r);
                    c.tiles_x = tm.tiles_x;
                    c.max_local = std::max(c.max_local, tm.n_local_tiles);
                    table.resize(2 * (size_t)tm.tiles_x * tm.tiles_y, 0u);
                    for (uint32_t lt = 0; lt < tm.n_local_tiles; ++lt) {
                        table[2 * (size_t)tm.tiles[lt]] = r;
                        table[2 * (size_t)tm.tiles[lt] + 1] = tm.offsets[lt];
                    }
                }
                HIP_CHECK(hipMalloc((void**)&c.d, table.size() * 4));
                HIP_CHECK(hipMemcpy(c.d, table.data(), table.size() * 4, hipMemcpyHostToDevice));
                it = cache.emplace(key, c).first;
            }
            c = it->second;
        }
        for (uint32_t r = 0; r < on.shard_count; ++r)
            if (make_tile_map(*profile, on, r).n_local > slice_pixels) fail(PT_ERR_INVALID, "slice_pixels too small for rank %u", r);
        uint32_t npix = profile->width * profile->height;
        hipLaunchKernelGGL(k_assemble, dim3((npix + 255u) / 256u), dim3(256), 0, (hipStream_t)hip_stream,
                           (const uint8_t*)d_gathered, (uint8_t*)d_image, c.d, profile->width,
                           profile->height, on.tile_w, on.tile_h, c.tiles_x, slice_pixels, elem_bytes);
        HIP_CHECK(hipGetLastError());
    });
}

}  // extern "C"

// ------------------------------------------------------------------ sample-coherent AOVs (pt_aov.h)
namespace {

// What pt_render_aov* derive from their arguments; everything they refuse is refused here, before any device work.
struct AovFrame {
    AovParams A{};
    TileMap tm;
    pt_opts o{};
    bool grid = false, alpha = false;
};

AovFrame aov_frame(const char* who, const pt_scene* scene, const pt_profile* profile, const pt_opts* opts, uint32_t aov_flags,
                   const void* out) {
    if (!scene || !profile || !out) fail(PT_ERR_INVALID, "%s: null argument", who);
    if (aov_flags & ~(uint32_t)(PT_AOV_FIRST_ENTRY | PT_AOV_CENTRE)) fail(PT_ERR_INVALID, "%s: unknown aov_flags 0x%x", who, aov_flags);
    if ((uintptr_t)out & 15u) fail(PT_ERR_INVALID, "%s: the output must be 16-byte aligned", who);
    AovFrame f;
    normalise_opts(*profile, opts, f.o);
    if (profile->samples == 0) fail(PT_ERR_INVALID, "%s: profile.samples must be > 0", who);
    f.tm = make_tile_map(*profile, f.o, f.o.shard_rank);
    if (f.tm.n_local == 0) fail(PT_ERR_INVALID, "%s: this rank has no pixels", who);
    AovParams& A = f.A;
    A.width = profile->width;
    A.height = profile->height;
    A.samples = profile->samples;
    A.n_local = (uint32_t)f.tm.n_local;
    A.flags = aov_flags;
    while (A.log2_seg < 6u && (1u << A.log2_seg) < A.samples) ++A.log2_seg;
    A.n_local_tiles = f.o.shard_count > 1 ? f.tm.n_local_tiles : 0u;
    A.tile_w = f.o.tile_w;
    A.tile_h = f.o.tile_h;
    A.tiles_x = f.tm.tiles_x;
    f.grid = !(f.o.flags & PT_FLAG_NO_GRIDS) && scene->dev.cam_grid.res != 0;
    f.alpha = scene->dev.has_translucent != 0;
    return f;
}

// The frame's tile table (sharded frames only: the scene's cached one, as pt_render_device takes it).
const uint32_t* aov_tiles(const pt_scene* scene, const pt_profile& p, const AovFrame& f) {
    if (f.o.shard_count <= 1) return nullptr;
    return tile_table(render_state(scene), p, f.o, f.tm, render_env().morton);
}

void aov_launch(const pt_scene& s, const AovFrame& f, const uint32_t* d_tiles, float4* d_aov, hipStream_t stream) {
    const uint64_t lanes = (uint64_t)f.A.n_local << f.A.log2_seg;
    dispatch([&](auto alpha, auto grid) {
        hipLaunchKernelGGL((k_aov<alpha, grid>), dim3((uint32_t)((lanes + 255u) / 256u)), dim3(256), 0, stream, s.dev, f.A, d_tiles, d_aov);
    }, f.alpha, f.grid);
    HIP_CHECK(hipGetLastError());
}

void aov_guides_check(const char* who, uint64_t n_pixels, uint32_t samples, const void* aov, const void* guides) {
    if (!aov || !guides) fail(PT_ERR_INVALID, "%s: null argument", who);
    if (!n_pixels || n_pixels >= (1ull << 31)) fail(PT_ERR_INVALID, "%s: n_pixels must be in 1 .. 2^31 - 1", who);
    if (!samples) fail(PT_ERR_INVALID, "%s: samples is 0", who);
}

void aov_guides_launch(uint64_t n, uint32_t samples, const float4* d_aov, float4* d_guides, hipStream_t stream) {
    hipLaunchKernelGGL(k_aov_guides, dim3((uint32_t)((n + 255u) / 256u)), dim3(256), 0, stream, d_aov, n, samples, d_guides);
    HIP_CHECK(hipGetLastError());
}

}  // namespace

extern "C" {

int pt_render_aov_device(const pt_scene* scene, const pt_profile* profile, const pt_opts* opts, uint32_t aov_flags, void* d_aov,
                         void* hip_stream) {
    return guarded([&] {
        const AovFrame f = aov_frame("pt_render_aov_device", scene, profile, opts, aov_flags, d_aov);
        HIP_CHECK(hipSetDevice(scene->device));
        aov_launch(*scene, f, aov_tiles(scene, *profile, f), (float4*)d_aov, (hipStream_t)hip_stream);
    });
}

int pt_render_aov(const pt_scene* scene, const pt_profile* profile, const pt_opts* opts, uint32_t aov_flags, float* aov) {
    return guarded([&] {
        const AovFrame f = aov_frame("pt_render_aov", scene, profile, opts, aov_flags, (const void*)16);
        if (!aov) fail(PT_ERR_INVALID, "pt_render_aov: null argument");
        HIP_CHECK(hipSetDevice(scene->device));
        const size_t n = f.tm.n_local;
        Staged<float4> d_aov(nullptr, n * 4);
        aov_launch(*scene, f, aov_tiles(scene, *profile, f), d_aov.d, nullptr);
        HIP_CHECK(hipDeviceSynchronize());
        d_aov.fetch((float4*)aov, n * 4);
    });
}

int pt_render_aov_samples(const pt_scene* scene, const pt_profile* profile, const pt_opts* opts, uint32_t aov_flags, float* records) {
    return guarded([&] {
        const AovFrame f = aov_frame("pt_render_aov_samples", scene, profile, opts, aov_flags, (const void*)16);
        if (!records) fail(PT_ERR_INVALID, "pt_render_aov_samples: null argument");
        const uint64_t n = f.tm.n_local;
        if ((uint64_t)profile->samples > (256ull << 20) / (n * 64u))
            fail(PT_ERR_INVALID, "pt_render_aov_samples: %u planes of %llu pixels exceed 256 MiB", profile->samples, (unsigned long long)n);
        HIP_CHECK(hipSetDevice(scene->device));
        const uint64_t items = (uint64_t)profile->samples * n;
        Staged<float4> d_rec(nullptr, items * 4);
        const uint32_t* d_tiles = aov_tiles(scene, *profile, f);
        dispatch([&](auto alpha, auto grid) {
            hipLaunchKernelGGL((k_aov_samples<alpha, grid>), dim3((uint32_t)((items + 255u) / 256u)), dim3(256), 0, nullptr, scene->dev, f.A,
                               d_tiles, d_rec.d);
        }, f.alpha, f.grid);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipDeviceSynchronize());
        d_rec.fetch((float4*)records, items * 4);
    });
}

int pt_aov_guides_device(int device, uint64_t n_pixels, uint32_t samples, const void* d_aov, void* d_guides, void* hip_stream) {
    return guarded([&] {
        aov_guides_check("pt_aov_guides_device", n_pixels, samples, d_aov, d_guides);
        if (((uintptr_t)d_aov | (uintptr_t)d_guides) & 15u) fail(PT_ERR_INVALID, "pt_aov_guides_device: the planes must be 16-byte aligned");
        if (device >= 0) HIP_CHECK(hipSetDevice(device));
        aov_guides_launch(n_pixels, samples, (const float4*)d_aov, (float4*)d_guides, (hipStream_t)hip_stream);
    });
}

int pt_aov_guides(int device, uint64_t n_pixels, uint32_t samples, const float* aov, float* guides) {
    return guarded([&] {
        aov_guides_check("pt_aov_guides", n_pixels, samples, aov, guides);
        if (device >= 0) HIP_CHECK(hipSetDevice(device));
        Staged<float4> d_aov((const float4*)aov, n_pixels * 4), d_guides(nullptr, n_pixels * 2);
        aov_guides_launch(n_pixels, samples, d_aov.d, d_guides.d, nullptr);
        HIP_CHECK(hipDeviceSynchronize());
        d_guides.fetch((float4*)guides, n_pixels * 2);
    });
}

int pt_render_denoised_aov(const pt_scene* scene, const pt_profile* profile, const pt_opts* opts, const pt_denoise_params* params,
                           int variance, uint32_t aov_flags, uint8_t* rgb8, float* color) {
    return guarded([&] {
        const char* who = "pt_render_denoised_aov";
        if (!scene || !profile) fail(PT_ERR_INVALID, "%s: null argument", who);
        if (variance) {
            dnv_check(who, params, profile->width, profile->height, profile->samples);
            moments_check_opts(who, opts);
        } else {
            dn_check_params(who, params);
        }
        const AovFrame f = aov_frame(who, scene, profile, opts, aov_flags, (const void*)16);
        if (f.o.shard_count > 1) fail(PT_ERR_UNSUPPORTED, "%s: the filter needs the whole image (shard_count %u)", who, f.o.shard_count);
        HIP_CHECK(hipSetDevice(scene->device));
        const uint32_t w = profile->width, h = profile->height;
        const size_t n = (size_t)w * h;
        Staged<uint8_t> d_rgb(nullptr, n * 3), d_scratch(nullptr, pt_denoise_scratch_bytes(w, h));
        Staged<float> d_acc(nullptr, n * 3), d_color(nullptr, n * 3);
        Staged<float2> d_mom(nullptr, variance ? n : 0);
        Staged<float4> d_aov(nullptr, n * 4), d_guides(nullptr, n * 2);
        FrameTaps taps;
        taps.moments = d_mom.d;
        // the raw frame (with its moments), then the AOV pass, the conversion and the filter behind it on the same stream
        render_device(render_state(scene), *profile, opts, d_rgb.d, d_acc.d, nullptr, true, variance ? &taps : nullptr);
        aov_launch(*scene, f, nullptr, d_aov.d, nullptr);
        aov_guides_launch(n, profile->samples, d_aov.d, d_guides.d, nullptr);
        if (variance)
            denoise_var_launch(w, h, profile->samples, *params, d_acc.d, d_mom.d, d_guides.d, color ? d_color.d : nullptr,
                               rgb8 ? d_rgb.d : nullptr, d_scratch.d, nullptr);
        else
            denoise_launch(w, h, profile->samples, *params, d_acc.d, d_guides.d, color ? d_color.d : nullptr, rgb8 ? d_rgb.d : nullptr,
                           d_scratch.d, nullptr);
        HIP_CHECK(hipDeviceSynchronize());
        if (rgb8) d_rgb.fetch(rgb8, n * 3);
        if (color) d_color.fetch(color, n * 3);
    });
}

}  // extern "C"

// ------------------------------------------------------------------ temporal history (pt_history.h)
// One allocation: two sets of planes (accum, moments, count, surf), the guides of the newest view, and the buffers
// pt_history_add_frame renders into (accum, moments, AOV records) - each on a 256-byte boundary.
struct pt_history {
    int device = 0;
    uint32_t width = 0, height = 0;
    uint64_t n = 0, bytes = 0;
    pt_history_params params{};
    uint8_t* base = nullptr;
    struct Set {
        float* accum = nullptr;
        float2* moments = nullptr;
        uint32_t* count = nullptr;
        float4* surf = nullptr;
    } set[2];
    int cur = 0;   // set[cur]: the current view; set[cur ^ 1]: the previous one (the next launch's output)
    float4* guides = nullptr;
    float *frame_accum = nullptr, *frame_aov = nullptr;
    float2* frame_moments = nullptr;
    int32_t* frame_map = nullptr;   // the map of the last pt_history_add_frame
    HistView view[2]{};   // [0] previous, [1] current
    uint32_t frames = 0, last_samples = 0;
    uint8_t* filter = nullptr;   // the film filter's scratch, made on first use, kept by pt_history_reset
    uint64_t bytes_filter = 0;
    ~pt_history() {
        if (filter) (void)hipFree(filter);
        if (base) (void)hipFree(base);
    }
};

namespace {

void hist_check_params(const char* who, const pt_history_params* p) {
    if (!p) fail(PT_ERR_INVALID, "%s: null parameters", who);
    if (!(p->normal_cos >= -1.f && p->normal_cos <= 1.f)) fail(PT_ERR_INVALID, "%s: normal_cos must be in -1 .. 1", who);
    if (!(p->plane_tol >= 0.f) || !std::isfinite(p->plane_tol)) fail(PT_ERR_INVALID, "%s: plane_tol must be finite and not negative", who);
    if (p->max_samples < 1u || p->max_samples >= (uint32_t)PT_FILM_MAX_SAMPLES)
        fail(PT_ERR_INVALID, "%s: max_samples %u outside 1 .. %u", who, p->max_samples, (unsigned)PT_FILM_MAX_SAMPLES - 1u);
    if (p->rotate < 1u || p->rotate > 4096u) fail(PT_ERR_INVALID, "%s: rotate %u outside 1 .. 4096", who, p->rotate);
}

// The view constants of include/ptgpu.h from the columns of a transform and tan(fov / 2).
HistView hist_view(const char* who, const float* c0, const float* c1, const float* c2, const float* c3, float ty, uint32_t width,
                   uint32_t height) {
    const double a[3][3] = {{c0[0], c1[0], c2[0]}, {c0[1], c1[1], c2[1]}, {c0[2], c1[2], c2[2]}};   // a[row][column]
    double C[3][3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            const int r0 = (i + 1) % 3, r1 = (i + 2) % 3, k0 = (j + 1) % 3, k1 = (j + 2) % 3;   // (cyclic: the sign is in the order)
            C[i][j] = a[r0][k0] * a[r1][k1] - a[r0][k1] * a[r1][k0];
        }
    const double det = a[0][0] * C[0][0] + a[0][1] * C[0][1] + a[0][2] * C[0][2];
    if (det == 0.0 || !std::isfinite(det)) fail(PT_ERR_INVALID, "%s: the camera transform is singular", who);
    HistView v;
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) v.M[3 * r + c] = (float)(C[c][r] / det);
    memcpy(v.c3, c3, 12);
    v.ty = ty;
    v.tx = ty * ((float)width / (float)height);
    return v;
}
HistView hist_view(const char* who, const pt_camera& cam, uint32_t width, uint32_t height) {
    const float* T = cam.transform;
    return hist_view(who, T, T + 4, T + 8, T + 12, tanf(cam.fov / 2.f), width, height);
}

void hist_check_advance(const char* who, const pt_history* h, uint32_t samples) {
    if (samples < 1u) fail(PT_ERR_INVALID, "%s: a frame needs samples >= 1", who);
    if ((uint64_t)h->params.max_samples + samples > (uint64_t)PT_FILM_MAX_SAMPLES)
        fail(PT_ERR_INVALID, "%s: max_samples %u + %u samples, at most %u", who, h->params.max_samples, samples, (unsigned)PT_FILM_MAX_SAMPLES);
}

HistArgs hist_args(const pt_history& h, const HistView& prev, uint32_t samples) {
    HistArgs A;
    A.prev = prev;
    A.width = h.width;
    A.height = h.height;
    A.samples = samples;
    A.max_samples = h.params.max_samples;
    A.normal_cos = h.params.normal_cos;
    A.plane_tol = h.params.plane_tol;
    return A;
}

void hist_launch(const pt_history& h, const HistArgs& A, const pt_history::Set& from, const pt_history::Set& to, const float* d_accum,
                 const float2* d_moments, const float4* d_aov, int32_t* d_map, hipStream_t stream) {
    hipLaunchKernelGGL(k_hist_advance, dim3((uint32_t)((h.n + 255u) / 256u)), dim3(256), 0, stream, A, d_aov, d_accum, d_moments,
                       (const float*)from.accum, (const float2*)from.moments, (const uint32_t*)from.count, (const float4*)from.surf,
                       to.accum, to.moments, to.count, to.surf, d_map);
    HIP_CHECK(hipGetLastError());
}

// The frame `view` of N samples joins the history: the launch, the guides of the new view, the swap.  Everything was checked.
void hist_advance(pt_history& h, const HistView& view, uint32_t samples, const float* d_accum, const float2* d_moments,
                  const float4* d_aov, int32_t* d_map, hipStream_t stream) {
    const HistView prev = h.frames ? h.view[1] : view;   // (an empty history: every count is 0, no tap passes)
    hist_launch(h, hist_args(h, prev, samples), h.set[h.cur], h.set[h.cur ^ 1], d_accum, d_moments, d_aov, d_map, stream);
    aov_guides_launch(h.n, samples, d_aov, h.guides, stream);
    h.cur ^= 1;
    h.view[0] = prev;
    h.view[1] = view;
    h.frames += 1u;
    h.last_samples = samples;
}

void hist_zero_counts(pt_history& h) {
    for (auto& s : h.set) HIP_CHECK(hipMemsetAsync(s.count, 0, h.n * sizeof(uint32_t), nullptr));
    HIP_CHECK(hipDeviceSynchronize());
}

FilmPlanes hist_planes(const pt_history& h) {
    const pt_history::Set& s = h.set[h.cur];
    return {s.accum, (const float*)s.moments, s.count, h.last_samples, h.width, h.height, h.n};
}

// The fewest samples a pixel holds.  Every advance leaves count >= N everywhere, so only a history whose last frame had one
// sample needs its plane read (that read waits for the device).
uint32_t hist_min_count(const pt_history& h, uint32_t* max_out = nullptr, bool exact = false) {
    if (!h.frames) {
        if (max_out) *max_out = 0u;
        return 0u;
    }
    if (!exact && h.last_samples >= 2u) return h.last_samples;
    std::vector<uint32_t> c(h.n);
    HIP_CHECK(hipMemcpy(c.data(), h.set[h.cur].count, h.n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    const auto mm = std::minmax_element(c.begin(), c.end());
    if (max_out) *max_out = *mm.second;
    return *mm.first;
}

void hist_check_resolve(const char* who, const pt_history* h, int tonemap_type, const void* rgb8, const void* color) {
    if (!h || (!rgb8 && !color)) fail(PT_ERR_INVALID, "%s: null argument", who);
    if (tonemap_type < PT_TONEMAP_REINHARD || tonemap_type > PT_TONEMAP_ACES) fail(PT_ERR_INVALID, "%s: unknown tonemap %d", who, tonemap_type);
    if (!h->frames) fail(PT_ERR_INVALID, "%s: the history holds no samples", who);
}

void hist_check_denoise(const char* who, const pt_history* h, int variance, const pt_denoise_params* p, float lum_floor, const void* rgb8,
                        const void* color) {
    if (!h || !p || (!rgb8 && !color)) fail(PT_ERR_INVALID, "%s: null argument", who);
    if (variance != 0 && variance != 1) fail(PT_ERR_INVALID, "%s: variance must be 0 (plain) or 1 (variance-guided)", who);
    if (variance) dnv_check(who, p, h->width, h->height, 2u);
    else dn_check_params(who, p);
    film_check_noise_args(who, lum_floor, 0.0);
    if (!h->frames) fail(PT_ERR_INVALID, "%s: the history holds no samples", who);
    if (variance) {
        HIP_CHECK(hipSetDevice(h->device));
        const uint32_t least = hist_min_count(*h);
        if (least < 2u) fail(PT_ERR_INVALID, "%s: a sample variance needs >= 2 samples in every pixel (the fewest: %u)", who, least);
    }
}

uint8_t* hist_filter_scratch(const pt_history& h_c) {
    pt_history& h = const_cast<pt_history&>(h_c);   // (scratch, not the history's contents)
    if (!h.filter) {
        const uint64_t bytes = dn_scratch_layout(h.n).total;
        HIP_CHECK(hipMalloc((void**)&h.filter, bytes));
        h.bytes_filter = bytes;
    }
    return h.filter;
}

}  // namespace

extern "C" {

void pt_history_params_default(pt_history_params* p) {
    if (!p) return;
    p->normal_cos = PT_HISTORY_DEFAULT_NORMAL_COS;
    p->plane_tol = PT_HISTORY_DEFAULT_PLANE_TOL;
    p->max_samples = PT_HISTORY_DEFAULT_MAX_SAMPLES;
    p->rotate = PT_HISTORY_DEFAULT_ROTATE;
}

int pt_history_create(int device, uint32_t width, uint32_t height, const pt_history_params* params, pt_history** out) {
    return guarded([&] {
        const char* who = "pt_history_create";
        if (!out) fail(PT_ERR_INVALID, "%s: null argument", who);
        *out = nullptr;
        hist_check_params(who, params);
        dn_check_size(who, width, height);
        if ((uint64_t)width * height > (1ull << 28)) fail(PT_ERR_INVALID, "%s: image too large", who);
        if (device >= 0) HIP_CHECK(hipSetDevice(device));
        auto h = std::make_unique<pt_history>();
        HIP_CHECK(hipGetDevice(&h->device));
        h->width = width;
        h->height = height;
        h->n = (uint64_t)width * height;
        h->params = *params;
        auto up = [](uint64_t v) { return (v + 255u) & ~(uint64_t)255u; };
        const uint64_t n = h->n, b_acc = up(12u * n), b_mom = up(8u * n), b_cnt = up(4u * n), b_surf = up(32u * n), b_aov = up(64u * n);
        h->bytes = 2u * (b_acc + b_mom + b_cnt + b_surf) + b_surf /* guides */ + b_acc + b_mom + b_aov + b_cnt /* map */;
        HIP_CHECK(hipMalloc((void**)&h->base, h->bytes));
        HIP_CHECK(hipMemset(h->base, 0, h->bytes));
        uint8_t* p = h->base;
        for (auto& s : h->set) {
            s.surf = (float4*)p, p += b_surf;
            s.accum = (float*)p, p += b_acc;
            s.moments = (float2*)p, p += b_mom;
            s.count = (uint32_t*)p, p += b_cnt;
        }
        h->guides = (float4*)p, p += b_surf;
        h->frame_aov = (float*)p, p += b_aov;
        h->frame_accum = (float*)p, p += b_acc;
        h->frame_moments = (float2*)p, p += b_mom;
        h->frame_map = (int32_t*)p;
        *out = h.release();
    });
}

void pt_history_destroy(pt_history* hist) { delete hist; }

int pt_history_reset(pt_history* hist) {
    return guarded([&] {
        if (!hist) fail(PT_ERR_INVALID, "pt_history_reset: null argument");
        HIP_CHECK(hipSetDevice(hist->device));
        hist_zero_counts(*hist);
        hist->frames = 0;
        hist->last_samples = 0;
        hist->view[0] = hist->view[1] = HistView{};
    });
}

int pt_history_get_info(const pt_history* hist, pt_history_info* out) {
    return guarded([&] {
        if (!hist || !out) fail(PT_ERR_INVALID, "pt_history_get_info: null argument");
        memset(out, 0, sizeof *out);
        out->width = hist->width;
        out->height = hist->height;
        out->frames = hist->frames;
        out->last_samples = hist->last_samples;
        if (hist->frames) {
            HIP_CHECK(hipSetDevice(hist->device));
            out->min_count = hist_min_count(*hist, &out->max_count, true);
        }
        out->device_bytes = hist->bytes + hist->bytes_filter;
        out->params = hist->params;
    });
}

int pt_history_get_view(const pt_history* hist, int which, pt_history_view* out) {
    return guarded([&] {
        if (!hist || !out) fail(PT_ERR_INVALID, "pt_history_get_view: null argument");
        if (which != 0 && which != 1) fail(PT_ERR_INVALID, "pt_history_get_view: which must be 0 (previous) or 1 (current)");
        if (!hist->frames) fail(PT_ERR_INVALID, "pt_history_get_view: the history has seen no frame");
        static_assert(sizeof(pt_history_view) == sizeof(HistView), "pt_history_view is HistView");
        memcpy(out, &hist->view[which], sizeof *out);
    });
}

int pt_history_advance_device(pt_history* hist, const pt_camera* camera, uint32_t samples, const void* d_accum, const void* d_moments,
                              const void* d_aov, void* d_map, void* hip_stream) {
    return guarded([&] {
        const char* who = "pt_history_advance_device";
        if (!hist || !camera || !d_accum || !d_moments || !d_aov) fail(PT_ERR_INVALID, "%s: null argument", who);
        hist_check_advance(who, hist, samples);
        if ((((uintptr_t)d_accum | (uintptr_t)d_moments | (uintptr_t)d_aov) & 15u) || ((uintptr_t)d_map & 3u))
            fail(PT_ERR_INVALID, "%s: the planes must be 16-byte aligned (the map: 4)", who);
        const HistView view = hist_view(who, *camera, hist->width, hist->height);
        HIP_CHECK(hipSetDevice(hist->device));
        hist_advance(*hist, view, samples, (const float*)d_accum, (const float2*)d_moments, (const float4*)d_aov, (int32_t*)d_map,
                     (hipStream_t)hip_stream);
    });
}

int pt_history_advance(pt_history* hist, const pt_camera* camera, uint32_t samples, const float* accum, const float* moments,
                       const float* aov, int32_t* map) {
    return guarded([&] {
        const char* who = "pt_history_advance";
        if (!hist || !camera || !accum || !moments || !aov) fail(PT_ERR_INVALID, "%s: null argument", who);
        hist_check_advance(who, hist, samples);
        const HistView view = hist_view(who, *camera, hist->width, hist->height);
        HIP_CHECK(hipSetDevice(hist->device));
        const size_t n = hist->n;
        // (the history's own frame buffers take the host planes)
        HIP_CHECK(hipMemcpy(hist->frame_accum, accum, n * 12u, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(hist->frame_moments, moments, n * 8u, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(hist->frame_aov, aov, n * 64u, hipMemcpyHostToDevice));
        Staged<int32_t> d_map(nullptr, map ? n : 0);
        hist_advance(*hist, view, samples, hist->frame_accum, hist->frame_moments, (const float4*)hist->frame_aov, map ? d_map.d : nullptr,
                     nullptr);
        HIP_CHECK(hipDeviceSynchronize());
        if (map) d_map.fetch(map, n);
    });
}

int pt_history_add_frame(pt_history* hist, const pt_scene* scene, const pt_profile* profile, const pt_opts* opts, uint32_t frame_index) {
    return guarded([&] {
        const char* who = "pt_history_add_frame";
        if (!hist || !scene || !profile) fail(PT_ERR_INVALID, "%s: null argument", who);
        if (profile->width != hist->width || profile->height != hist->height)
            fail(PT_ERR_INVALID, "%s: a %ux%u frame for a %ux%u history", who, profile->width, profile->height, hist->width, hist->height);
        if (scene->device != hist->device)
            fail(PT_ERR_INVALID, "%s: the scene is on device %d, the history on device %d", who, scene->device, hist->device);
        moments_check_opts(who, opts);
        pt_opts o;
        normalise_opts(*profile, opts, o);
        if (o.shard_count > 1) fail(PT_ERR_UNSUPPORTED, "%s: a history holds the whole image (shard_count %u)", who, o.shard_count);
        const uint32_t N = profile->samples, K = hist->params.rotate;
        hist_check_advance(who, hist, N);
        if ((uint64_t)K * N > (uint64_t)PT_FILM_MAX_SAMPLES) fail(PT_ERR_INVALID, "%s: rotate %u x %u samples, at most %u", who, K, N, (unsigned)PT_FILM_MAX_SAMPLES);
        const DevScene& D = scene->dev;
        const HistView view = hist_view(who, D.cam_c0, D.cam_c1, D.cam_c2, D.cam_c3, D.tan_half_fov, hist->width, hist->height);
        const AovFrame f = aov_frame(who, scene, profile, opts, 0u, hist->frame_aov);
        HIP_CHECK(hipSetDevice(hist->device));
        FrameTaps taps;
        taps.moments = hist->frame_moments;
        if (K == 1u) {
            render_device(render_state(scene), *profile, opts, nullptr, hist->frame_accum, nullptr, false, &taps);
        } else {
            const uint32_t j = frame_index % K;
            pt_profile wide = *profile;
            wide.samples = K * N;
            const SampleWindow win{j * N, j * N + N};
            HIP_CHECK(hipMemsetAsync(hist->frame_accum, 0, hist->n * 12u, nullptr));
            HIP_CHECK(hipMemsetAsync(hist->frame_moments, 0, hist->n * 8u, nullptr));
            render_device(render_state(scene), wide, opts, nullptr, hist->frame_accum, nullptr, false, &taps, nullptr, &win);
        }
        aov_launch(*scene, f, nullptr, (float4*)hist->frame_aov, nullptr);
        hist_advance(*hist, view, N, hist->frame_accum, hist->frame_moments, (const float4*)hist->frame_aov, hist->frame_map, nullptr);
        HIP_CHECK(hipDeviceSynchronize());
    });
}

int pt_history_read(const pt_history* hist, float* accum, float* moments, uint32_t* counts, float* surf, float* guides, int32_t* map) {
    return guarded([&] {
        if (!hist) fail(PT_ERR_INVALID, "pt_history_read: null argument");
        HIP_CHECK(hipSetDevice(hist->device));
        const pt_history::Set& s = hist->set[hist->cur];
        const size_t n = hist->n;
        if (accum) HIP_CHECK(hipMemcpy(accum, s.accum, n * 12u, hipMemcpyDeviceToHost));
        if (moments) HIP_CHECK(hipMemcpy(moments, s.moments, n * 8u, hipMemcpyDeviceToHost));
        if (counts) HIP_CHECK(hipMemcpy(counts, s.count, n * 4u, hipMemcpyDeviceToHost));
        if (surf) HIP_CHECK(hipMemcpy(surf, s.surf, n * 32u, hipMemcpyDeviceToHost));
        if (guides) HIP_CHECK(hipMemcpy(guides, hist->guides, n * 32u, hipMemcpyDeviceToHost));
        if (map) HIP_CHECK(hipMemcpy(map, hist->frame_map, n * 4u, hipMemcpyDeviceToHost));
    });
}

int pt_history_resolve_device(const pt_history* hist, int tonemap, void* d_rgb8, void* d_color, void* hip_stream) {
    return guarded([&] {
        hist_check_resolve("pt_history_resolve_device", hist, tonemap, d_rgb8, d_color);
        HIP_CHECK(hipSetDevice(hist->device));
        film_resolve_launch(hist_planes(*hist), tonemap, (uint8_t*)d_rgb8, (float*)d_color, (hipStream_t)hip_stream);
    });
}

int pt_history_resolve(const pt_history* hist, int tonemap, uint8_t* rgb8, float* color) {
    return guarded([&] {
        hist_check_resolve("pt_history_resolve", hist, tonemap, rgb8, color);
        HIP_CHECK(hipSetDevice(hist->device));
        const size_t n = (size_t)hist->n * 3u;
        Staged<uint8_t> d_rgb(nullptr, n);
        Staged<float> d_color(nullptr, n);
        film_resolve_launch(hist_planes(*hist), tonemap, rgb8 ? d_rgb.d : nullptr, color ? d_color.d : nullptr, nullptr);
        HIP_CHECK(hipDeviceSynchronize());
        if (rgb8) d_rgb.fetch(rgb8, n);
        if (color) d_color.fetch(color, n);
    });
}

int pt_history_denoise_device(const pt_history* hist, int variance, const pt_denoise_params* params, float lum_floor, void* d_rgb8,
                              void* d_color, void* hip_stream) {
    return guarded([&] {
        hist_check_denoise("pt_history_denoise_device", hist, variance, params, lum_floor, d_rgb8, d_color);
        HIP_CHECK(hipSetDevice(hist->device));
        fdn_launch(hist_planes(*hist), variance, *params, lum_floor, hist->guides, (float*)d_color, (uint8_t*)d_rgb8, nullptr,
                   hist_filter_scratch(*hist), (hipStream_t)hip_stream);
    });
}

int pt_history_denoise(const pt_history* hist, int variance, const pt_denoise_params* params, float lum_floor, uint8_t* rgb8,
                       float* color) {
    return guarded([&] {
        hist_check_denoise("pt_history_denoise", hist, variance, params, lum_floor, rgb8, color);
        HIP_CHECK(hipSetDevice(hist->device));
        const size_t n = (size_t)hist->n * 3u;
        Staged<uint8_t> d_rgb(nullptr, rgb8 ? n : 0);
        Staged<float> d_color(nullptr, color ? n : 0);
        fdn_launch(hist_planes(*hist), variance, *params, lum_floor, hist->guides, color ? d_color.d : nullptr, rgb8 ? d_rgb.d : nullptr,
                   nullptr, hist_filter_scratch(*hist), nullptr);
        HIP_CHECK(hipDeviceSynchronize());
        if (rgb8) d_rgb.fetch(rgb8, n);
        if (color) d_color.fetch(color, n);
    });
}

int pt_history_kernel_times(const pt_history* hist, uint32_t reps, float* ms_advance) {
    return guarded([&] {
        const char* who = "pt_history_kernel_times";
        if (!hist || !ms_advance || !reps) fail(PT_ERR_INVALID, "%s: null argument", who);
        if (!hist->frames) fail(PT_ERR_INVALID, "%s: the history holds no samples", who);
        HIP_CHECK(hipSetDevice(hist->device));
        hipEvent_t e0 = nullptr, e1 = nullptr;
        struct Free {
            hipEvent_t &a, &b;
            ~Free() {
                if (a) (void)hipEventDestroy(a);
                if (b) (void)hipEventDestroy(b);
            }
        } guard{e0, e1};
        HIP_CHECK(hipEventCreate(&e0));
        HIP_CHECK(hipEventCreate(&e1));
        // current set -> the other one (scratch between advances), with the frame buffers as they stand; no swap
        const HistArgs A = hist_args(*hist, hist->view[1], std::max(1u, hist->last_samples));
        for (uint32_t r = 0; r < reps; ++r) {
            HIP_CHECK(hipEventRecord(e0, 0));
            hist_launch(*hist, A, hist->set[hist->cur], hist->set[hist->cur ^ 1], hist->frame_accum, hist->frame_moments,
                        (const float4*)hist->frame_aov, nullptr, nullptr);
            HIP_CHECK(hipEventRecord(e1, 0));
            HIP_CHECK(hipEventSynchronize(e1));
            HIP_CHECK(hipEventElapsedTime(&ms_advance[r], e0, e1));
        }
    });
}

}  // extern "C"

// ------------------------------------------------------------------ RCCL gather
// librccl.so is loaded on first use: a single-GPU host never needs it.
namespace {
struct Rccl {
    typedef struct { char internal[128]; } UniqueId;
    int (*GetUniqueId)(UniqueId*) = nullptr;
    int (*CommInitRank)(void**, int, UniqueId, int) = nullptr;
    int (*CommInitAll)(void**, int, const int*) = nullptr;
    int (*CommDestroy)(void*) = nullptr;
    int (*AllGather)(const void*, void*, size_t, int, void*, hipStream_t) = nullptr;
    const char* (*GetErrorString)(int) = nullptr;
    void* handle = nullptr;
    std::string error;
};
Rccl& rccl() {
    static Rccl r;
    static std::once_flag once;
    std::call_once(once, [] {
        for (const char* name : {"librccl.so", "librccl.so.1", "/opt/rocm/lib/librccl.so"}) {
            r.handle = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
            if (r.handle) break;
        }
        if (!r.handle) {
            r.error = std::string("cannot load librccl.so: ") + dlerror();
            return;
        }
        auto sym = [&](const char* n) {
            void* p = dlsym(r.handle, n);
            if (!p && r.error.empty()) r.error = std::string("librccl.so lacks ") + n;
            return p;
        };
        r.GetUniqueId = (decltype(r.GetUniqueId))sym("ncclGetUniqueId");
        r.CommInitRank = (decltype(r.CommInitRank))sym("ncclCommInitRank");
        r.CommInitAll = (decltype(r.CommInitAll))sym("ncclCommInitAll");
        r.CommDestroy = (decltype(r.CommDestroy))sym("ncclCommDestroy");
        r.AllGather = (decltype(r.AllGather))sym("ncclAllGather");
        r.GetErrorString = (decltype(r.GetErrorString))sym("ncclGetErrorString");
    });
    if (!r.error.empty()) fail(PT_ERR_DEVICE, "%s", r.error.c_str());
    return r;
}
#define RCCL_CHECK(expr)                                                                                           \
    do {                                                                                                           \
        int _e = (expr);                                                                                           \
        if (_e != 0) fail(PT_ERR_DEVICE, "%s failed: %s (%s:%d)", #expr, rccl().GetErrorString(_e), __FILE__, __LINE__); \
    } while (0)

// pt_get_*_cache_stats: each value to the caller's variable; nothing is written unless every pointer is given.
int cache_stats(std::initializer_list<std::pair<uint64_t*, uint64_t>> out) {
    for (const auto& o : out)
        if (!o.first) return PT_ERR_INVALID;
    for (const auto& o : out) *o.first = o.second;
    return PT_OK;
}
// pt_get_hit1_cache_stats / pt_get_hit2_cache_stats: the cache's numbers and its counter of unknown casts from the device
int bounce_hits_stats(const pt_scene* scene, const pt_scene::FrameCache& fc, const DeviceBuffer& unknown_casts_dev, const char* who,
                      uint64_t* bytes, uint64_t* items, uint64_t* items_cached, uint64_t* resets, uint64_t* stores, uint64_t* loads,
                      uint64_t* unknown_casts) {
    return guarded([&] {
        uint64_t unknown = 0;
        if (unknown_casts_dev.p) {   // (synchronises, like pt_get_cull_stats)
            HIP_CHECK(hipSetDevice(scene->device));
            HIP_CHECK(hipDeviceSynchronize());
            HIP_CHECK(hipMemcpy(&unknown, unknown_casts_dev.p, 8, hipMemcpyDeviceToHost));
        }
        if (cache_stats({{bytes, fc.buf.bytes}, {items, fc.items}, {items_cached, fc.mark}, {resets, fc.counter[0]}, {stores, fc.counter[1]},
                         {loads, fc.counter[2]}, {unknown_casts, unknown}}) != PT_OK)
            fail(PT_ERR_INVALID, "%s: null argument", who);
    });
}
}  // namespace

struct pt_comm {
    void* comm = nullptr;
    int rank = 0, size = 1, device = 0;
};

extern "C" {

int pt_comm_unique_id(uint8_t id[PT_COMM_ID_BYTES]) {
    return guarded([&] {
        if (!id) fail(PT_ERR_INVALID, "pt_comm_unique_id: null argument");
        static_assert(sizeof(Rccl::UniqueId) == PT_COMM_ID_BYTES, "ncclUniqueId is 128 bytes");
        Rccl::UniqueId u;
        RCCL_CHECK(rccl().GetUniqueId(&u));
        memcpy(id, &u, sizeof u);
    });
}

int pt_comm_create(const uint8_t id[PT_COMM_ID_BYTES], int rank, int size, int device, pt_comm** out) {
    return guarded([&] {
        if (!id || !out || size < 1 || rank < 0 || rank >= size) fail(PT_ERR_INVALID, "pt_comm_create: bad argument");
        select_device(device);
        auto c = std::make_unique<pt_comm>();
        HIP_CHECK(hipGetDevice(&c->device));
        c->rank = rank;
        c->size = size;
        Rccl::UniqueId u;
        memcpy(&u, id, sizeof u);
        RCCL_CHECK(rccl().CommInitRank(&c->comm, size, u, rank));
        *out = c.release();
    });
}

int pt_comm_create_all(const int* devices, int n, pt_comm** out) {
    return guarded([&] {
        if (!devices || !out || n < 1) fail(PT_ERR_INVALID, "pt_comm_create_all: bad argument");
        std::vector<void*> comms(n, nullptr);
        RCCL_CHECK(rccl().CommInitAll(comms.data(), n, devices));
        for (int i = 0; i < n; ++i) {
            out[i] = new pt_comm;
            out[i]->comm = comms[i];
            out[i]->rank = i;
            out[i]->size = n;
            out[i]->device = devices[i];
        }
    });
}

void pt_comm_destroy(pt_comm* c) {
    if (!c) return;
    if (c->comm) {
        (void)hipSetDevice(c->device);
        (void)rccl().CommDestroy(c->comm);
    }
    delete c;
}

int pt_gather_tiles(pt_comm* comm, const pt_profile* profile, uint32_t tile_w, uint32_t tile_h, uint64_t slice_pixels,
                    uint32_t elem_bytes, const void* d_local, void* d_gathered, void* d_image, void* hip_stream) {
    return guarded([&] {
        if (!comm || !profile || !d_local || !d_gathered || !d_image) fail(PT_ERR_INVALID, "pt_gather_tiles: null argument");
        if (elem_bytes != 3 && elem_bytes != 12) fail(PT_ERR_INVALID, "pt_gather_tiles: elem_bytes must be 3 or 12");
        HIP_CHECK(hipSetDevice(comm->device));
        // one exchange step: every rank contributes its packed, zero-padded slice (ncclChar = 0)
        RCCL_CHECK(rccl().AllGather(d_local, d_gathered, (size_t)slice_pixels * elem_bytes, 0 /* ncclChar */, comm->comm,
                                    (hipStream_t)hip_stream));
        int rc = pt_assemble_tiles(profile, (uint32_t)comm->size, tile_w, tile_h, slice_pixels, elem_bytes, d_gathered, d_image,
                                   hip_stream);
        if (rc != PT_OK) throw GpuError{rc, g_err};
    });
}

int pt_render_gathered(const pt_scene* scene, pt_comm* comm, const pt_profile* profile, const pt_opts* opts,
                       uint64_t slice_pixels, uint8_t* rgb8_frame) {
    return guarded([&] {
        if (!scene || !comm || !profile || !opts) fail(PT_ERR_INVALID, "pt_render_gathered: null argument");
        if (opts->shard_count != (uint32_t)comm->size || opts->shard_rank != (uint32_t)comm->rank)
            fail(PT_ERR_INVALID, "pt_render_gathered: opts shard %u/%u does not match communicator rank %d/%d", opts->shard_rank,
                 opts->shard_count, comm->rank, comm->size);
        HIP_CHECK(hipSetDevice(scene->device));
        pt_opts o;
        normalise_opts(*profile, opts, o);
        const uint64_t n_local = make_tile_map(*profile, o, o.shard_rank).n_local;
        if (n_local > slice_pixels) fail(PT_ERR_INVALID, "pt_render_gathered: slice_pixels too small");
        const size_t npix = (size_t)profile->width * profile->height;
        Staged<uint8_t> d_local(nullptr, slice_pixels * 3), d_gathered(nullptr, slice_pixels * 3 * comm->size), d_image(nullptr, npix * 3);
        HIP_CHECK(hipMemset(d_local.d, 0, slice_pixels * 3));   // the padding of the slice
        render_device(render_state(scene), *profile, opts, d_local.d, nullptr, nullptr);
        int rc = pt_gather_tiles(comm, profile, o.tile_w, o.tile_h, slice_pixels, 3, d_local.d, d_gathered.d, d_image.d, nullptr);
        if (rc != PT_OK) throw GpuError{rc, g_err};
        HIP_CHECK(hipDeviceSynchronize());
        if (rgb8_frame) d_image.fetch(rgb8_frame, npix * 3);
    });
}

int pt_film_exchange_comm(float* tile_sum, float* tile_max, uint32_t n_tiles, void* user) {
    return guarded([&] {
        pt_comm* comm = (pt_comm*)user;
        if (!comm || !tile_sum || !tile_max || !n_tiles) fail(PT_ERR_INVALID, "pt_film_exchange_comm: null argument");
        HIP_CHECK(hipSetDevice(comm->device));
        // one exchange step: every rank contributes its two arrays; an entry's value is its owner's, every other rank's is
        // +0.f, and errors are not negative - so the largest of an entry's values is the owner's, bit for bit
        const size_t n = 2u * (size_t)n_tiles;
        std::vector<float> mine(tile_sum, tile_sum + n_tiles), all(n * (size_t)comm->size);
        mine.insert(mine.end(), tile_max, tile_max + n_tiles);
        Staged<float> d_mine(mine.data(), n), d_all(nullptr, all.size());
        RCCL_CHECK(rccl().AllGather(d_mine.d, d_all.d, n * sizeof(float), 0 /* ncclChar */, comm->comm, nullptr));
        HIP_CHECK(hipDeviceSynchronize());
        d_all.fetch(all.data(), all.size());
        for (size_t i = 0; i < n; ++i) {
            float v = all[i];
            for (int r = 1; r < comm->size; ++r)
                if (all[(size_t)r * n + i] > v) v = all[(size_t)r * n + i];
            (i < n_tiles ? tile_sum[i] : tile_max[i - n_tiles]) = v;
        }
    });
}

int pt_get_timing(const pt_scene* scene, pt_timing* out) {
    if (!scene || !out) return PT_ERR_INVALID;
    *out = scene->timing;
    return PT_OK;
}
int pt_get_counters(const pt_scene* scene, pt_counters* out) {
    if (!scene || !out) return PT_ERR_INVALID;
    *out = scene->counters;
    return PT_OK;
}
int pt_get_cull_stats(const pt_scene* scene, uint32_t* n_blocks, uint32_t* n_empty) {
    return guarded([&] {
        if (!scene || !n_blocks || !n_empty) fail(PT_ERR_INVALID, "pt_get_cull_stats: null argument");
        *n_blocks = scene->frame_state.mask_blocks;
        *n_empty = 0;
        if (scene->frame_state.mask_blocks) {
            HIP_CHECK(hipSetDevice(scene->device));
            HIP_CHECK(hipDeviceSynchronize());
            std::vector<uint32_t> mask(scene->frame_state.mask_blocks);
            HIP_CHECK(hipMemcpy(mask.data(), scene->pipe.block_mask.p, mask.size() * 4, hipMemcpyDeviceToHost));
            for (uint32_t m : mask) *n_empty += m != 0u;
        }
    });
}
int pt_get_rng_cache_stats(const pt_scene* scene, uint64_t* bytes, uint64_t* items, uint64_t* items_cached, uint64_t* fills) {
    if (!scene) return PT_ERR_INVALID;
    const pt_scene::FrameCache& fc = scene->rng_cache;
    return cache_stats({{bytes, fc.buf.bytes}, {items, fc.items}, {items_cached, fc.mark}, {fills, fc.counter[0]}});
}
int pt_get_hit_cache_stats(const pt_scene* scene, uint64_t* bytes, uint64_t* items, uint64_t* items_cached, uint64_t* stores, uint64_t* loads) {
    if (!scene) return PT_ERR_INVALID;
    const pt_scene::FrameCache& fc = scene->hit_cache;
    return cache_stats({{bytes, fc.buf.bytes}, {items, fc.items}, {items_cached, fc.mark}, {stores, fc.counter[0]}, {loads, fc.counter[1]}});
}
int pt_get_hit1_cache_stats(const pt_scene* scene, uint64_t* bytes, uint64_t* items, uint64_t* items_cached, uint64_t* resets,
                            uint64_t* stores, uint64_t* loads, uint64_t* unknown_casts) {
    if (!scene) return PT_ERR_INVALID;
    return bounce_hits_stats(scene, scene->hit1_cache, scene->hit1_unknown, "pt_get_hit1_cache_stats", bytes, items, items_cached, resets,
                             stores, loads, unknown_casts);
}
int pt_get_hit1_fused_stats(const pt_scene* scene, uint64_t* launches, uint64_t* written, uint64_t* elided, uint64_t* unknown) {
    if (!scene) return PT_ERR_INVALID;
    return guarded([&] {
        uint64_t n[4] = {0, 0, 0, 0};   // (pt_scene::hit1_unknown)
        if (scene->hit1_unknown.p) {    // (synchronises, like pt_get_hit1_cache_stats)
            HIP_CHECK(hipSetDevice(scene->device));
            HIP_CHECK(hipDeviceSynchronize());
            HIP_CHECK(hipMemcpy(n, scene->hit1_unknown.p, sizeof n, hipMemcpyDeviceToHost));
        }
        if (cache_stats({{launches, scene->hit1_fused_launches}, {written, n[1] - n[3]}, {elided, n[2]}, {unknown, n[3]}}) != PT_OK)
            fail(PT_ERR_INVALID, "pt_get_hit1_fused_stats: null argument");
    });
}
int pt_get_cont_cache_stats(const pt_scene* scene, uint64_t* bytes, uint64_t* items, uint64_t* items_cached, uint64_t* resets,
                            uint64_t* stores, uint64_t* loads, uint64_t* missing) {
    if (!scene) return PT_ERR_INVALID;
    return guarded([&] {
        uint64_t n[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // (pt_scene::hit1_unknown: word 6)
        if (scene->hit1_unknown.p) {                // (synchronises, like pt_get_hit1_cache_stats)
            HIP_CHECK(hipSetDevice(scene->device));
            HIP_CHECK(hipDeviceSynchronize());
            HIP_CHECK(hipMemcpy(n, scene->hit1_unknown.p, sizeof n, hipMemcpyDeviceToHost));
        }
        const pt_scene::FrameCache& fc = scene->cont_cache;
        if (cache_stats({{bytes, fc.buf.bytes}, {items, fc.items}, {items_cached, fc.mark}, {resets, fc.counter[0]}, {stores, fc.counter[1]},
                         {loads, fc.counter[2]}, {missing, n[6]}}) != PT_OK)
            fail(PT_ERR_INVALID, "pt_get_cont_cache_stats: null argument");
    });
}
int pt_get_cont_escape_stats(const pt_scene* scene, uint64_t* fill_launches, uint64_t* fill_items, uint64_t* flagged_launches,
                             uint64_t* fallback_lanes) {
    if (!scene) return PT_ERR_INVALID;
    return guarded([&] {
        uint64_t n[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // (pt_scene::hit1_unknown: word 7)
        if (scene->hit1_unknown.p) {                // (synchronises, like pt_get_hit1_cache_stats)
            HIP_CHECK(hipSetDevice(scene->device));
            HIP_CHECK(hipDeviceSynchronize());
            HIP_CHECK(hipMemcpy(n, scene->hit1_unknown.p, sizeof n, hipMemcpyDeviceToHost));
        }
        if (cache_stats({{fill_launches, scene->cont_fill_launches}, {fill_items, scene->cont_fill_items},
                         {flagged_launches, scene->cont_flagged_launches}, {fallback_lanes, n[7]}}) != PT_OK)
            fail(PT_ERR_INVALID, "pt_get_cont_escape_stats: null argument");
    });
}
int pt_get_b0_lean_stats(const pt_scene* scene, uint64_t* lean_launches, uint64_t* general_launches, uint64_t* guard_trips) {
    if (!scene) return PT_ERR_INVALID;
    return cache_stats({{lean_launches, scene->b0_lean_launches}, {general_launches, scene->b0_general_launches},
                        {guard_trips, scene->b0_lean_guard_trips}});
}
int pt_get_b1_lean_stats(const pt_scene* scene, uint64_t* lean_launches_b1, uint64_t* lean_launches_b2, uint64_t* general_launches,
                         uint64_t* handed_over) {
    if (!scene) return PT_ERR_INVALID;
    return guarded([&] {
        uint64_t handed = 0;   // (word 6 of the fused counter blocks of bounces 1 and 2: pt_scene::hits_unknown(2), (3))
        for (uint32_t b = 2; b <= 3u; ++b) {
            const DeviceBuffer& block = scene->hits_unknown(b);
            if (!block.p) continue;   // (synchronises, like pt_get_bounce1_fused_stats)
            uint64_t n = 0;
            HIP_CHECK(hipSetDevice(scene->device));
            HIP_CHECK(hipDeviceSynchronize());
            HIP_CHECK(hipMemcpy(&n, (const uint64_t*)block.p + 6, sizeof n, hipMemcpyDeviceToHost));
            handed += n;
        }
        if (cache_stats({{lean_launches_b1, scene->b1_lean_launches[0]}, {lean_launches_b2, scene->b1_lean_launches[1]},
                         {general_launches, scene->b1_general_launches}, {handed_over, handed}}) != PT_OK)
            fail(PT_ERR_INVALID, "pt_get_b1_lean_stats: null argument");
    });
}
int pt_scene_cont_states_copy(const pt_scene* scene, uint32_t* out, uint64_t count) {
    if (!scene || (!out && count)) return PT_ERR_INVALID;
    return guarded([&] {
        const pt_scene::FrameCache& fc = scene->cont_cache;
        if (count > fc.mark) fail(PT_ERR_INVALID, "pt_scene_cont_states_copy: more records than the cache holds");
        if (!count) return;
        HIP_CHECK(hipSetDevice(scene->device));
        HIP_CHECK(hipDeviceSynchronize());
        // (word 3 of every record of plane 0)
        HIP_CHECK(hipMemcpy2D(out, 4, (const uint32_t*)fc.buf.p + 3, 16, 4, (size_t)count, hipMemcpyDeviceToHost));
    });
}
int pt_get_hit2_cache_stats(const pt_scene* scene, uint64_t* bytes, uint64_t* items, uint64_t* items_cached, uint64_t* resets,
                            uint64_t* stores, uint64_t* loads, uint64_t* unknown_casts) {
    if (!scene) return PT_ERR_INVALID;
    return bounce_hits_stats(scene, scene->hit2_cache, scene->hit2_unknown, "pt_get_hit2_cache_stats", bytes, items, items_cached, resets,
                             stores, loads, unknown_casts);
}
int pt_get_bounce1_fused_stats(const pt_scene* scene, uint64_t* launches, uint64_t* inlined, uint64_t* deferred, uint64_t* next_written,
                               uint64_t* next_elided, uint64_t* next_unknown) {
    if (!scene) return PT_ERR_INVALID;
    return guarded([&] {
        uint64_t n[6] = {0, 0, 0, 0, 0, 0};   // (pt_scene::hit2_unknown)
        if (scene->hit2_unknown.p) {          // (synchronises, like pt_get_hit2_cache_stats)
            HIP_CHECK(hipSetDevice(scene->device));
            HIP_CHECK(hipDeviceSynchronize());
            HIP_CHECK(hipMemcpy(n, scene->hit2_unknown.p, sizeof n, hipMemcpyDeviceToHost));
        }
        if (cache_stats({{launches, scene->b1_fused_launches}, {inlined, n[4]}, {deferred, n[5]}, {next_written, n[1] - n[3]},
                         {next_elided, n[2]}, {next_unknown, n[3]}}) != PT_OK)
            fail(PT_ERR_INVALID, "pt_get_bounce1_fused_stats: null argument");
    });
}
int pt_get_vis_cache_stats(const pt_scene* scene, uint64_t* bytes, uint64_t* items, uint64_t* resets, uint64_t* launches) {
    if (!scene) return PT_ERR_INVALID;
    const pt_scene::FrameCache& fc = scene->vis_cache;
    return cache_stats({{bytes, fc.buf.bytes}, {items, fc.items}, {resets, fc.counter[0]}, {launches, fc.counter[1]}});
}
int pt_get_vis1_cache_stats(const pt_scene* scene, uint64_t* bytes, uint64_t* items, uint64_t* resets, uint64_t* launches) {
    if (!scene) return PT_ERR_INVALID;
    const pt_scene::FrameCache& fc = scene->vis1_cache;
    return cache_stats({{bytes, fc.buf.bytes}, {items, fc.items}, {resets, fc.counter[0]}, {launches, fc.counter[1]}});
}
// The same numbers by bounce (pt_scene::hits_cache, vis_cache_of, hits_unknown): hits 1-5, visibility and fused passes 1-4.
int pt_get_bounce_hits_cache_stats(const pt_scene* scene, uint32_t bounce, uint64_t* bytes, uint64_t* items, uint64_t* items_cached,
                                   uint64_t* resets, uint64_t* stores, uint64_t* loads, uint64_t* unknown_casts) {
    if (!scene || bounce < 1u || bounce >= pt_scene::HIT_BOUNCES) return PT_ERR_INVALID;
    return bounce_hits_stats(scene, scene->hits_cache(bounce), scene->hits_unknown(bounce), "pt_get_bounce_hits_cache_stats", bytes, items,
                             items_cached, resets, stores, loads, unknown_casts);
}
int pt_get_bounce_vis_cache_stats(const pt_scene* scene, uint32_t bounce, uint64_t* bytes, uint64_t* items, uint64_t* resets, uint64_t* launches) {
    if (!scene || bounce < 1u || bounce + 1u >= pt_scene::HIT_BOUNCES) return PT_ERR_INVALID;
    const pt_scene::FrameCache& fc = scene->vis_cache_of(bounce);
    return cache_stats({{bytes, fc.buf.bytes}, {items, fc.items}, {resets, fc.counter[0]}, {launches, fc.counter[1]}});
}
int pt_get_bounce_fused_stats(const pt_scene* scene, uint32_t bounce, uint64_t* launches, uint64_t* inlined, uint64_t* deferred,
                              uint64_t* next_written, uint64_t* next_elided, uint64_t* next_unknown) {
    if (!scene || bounce < 1u || bounce + 1u >= pt_scene::HIT_BOUNCES) return PT_ERR_INVALID;
    return guarded([&] {
        uint64_t n[6] = {0, 0, 0, 0, 0, 0};
        const DeviceBuffer& block = scene->hits_unknown(bounce + 1u);   // (behind the next bounce's counter of unknown casts)
        if (block.p) {                                                  // (synchronises, like pt_get_bounce1_fused_stats)
            HIP_CHECK(hipSetDevice(scene->device));
            HIP_CHECK(hipDeviceSynchronize());
            HIP_CHECK(hipMemcpy(n, block.p, sizeof n, hipMemcpyDeviceToHost));
        }
        if (cache_stats({{launches, scene->fused_launches(bounce)}, {inlined, n[4]}, {deferred, n[5]},
                         {next_written, n[1] - n[3]}, {next_elided, n[2]}, {next_unknown, n[3]}}) != PT_OK)
            fail(PT_ERR_INVALID, "pt_get_bounce_fused_stats: null argument");
    });
}
int pt_kernel_occupancy(int device, int which, int* blocks_per_cu) {
    return guarded([&] {
        if (!blocks_per_cu || which < 0 || which > 6) fail(PT_ERR_INVALID, "pt_kernel_occupancy: bad argument");
        HIP_CHECK(hipSetDevice(device));
        if (which == 0)
            HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks_per_cu, k_wf_shade<false, false, true, 3>, WF_SHADE_THREADS, 0));
        else if (which == 2)
            HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks_per_cu, (WfShadeHitsKernel)k_wf_shade_hits<(SB_B0_CACHED | SB_STORE)>, WF_SHADE_THREADS, 0));
        else if (which == 3)
            HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks_per_cu, (WfShadeHitsKernel)k_wf_shade_hits<(SB_B0_CACHED | SB_LOAD)>, WF_SHADE_THREADS, 0));
        else if (which == 4)
            HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks_per_cu, (WfShadeVisKernel)k_wf_shade_hits<(SB_B0_CACHED | SB_LOAD | SB_VIS)>, WF_SHADE_THREADS, 0));
        else if (which == 6)
            HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks_per_cu, (WfShadeContLoadKernel)k_wf_shade_hits<(SB_B0_CACHED | SB_LOAD | SB_VIS | SB_NEXT | SB_CONT_LOAD)>, WF_SHADE_THREADS, 0));
        else if (which == 5)
            HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks_per_cu, (WfShadeVisKernel)k_wf_shade_hits<(SB_B0_CACHED_DIRL | SB_LOAD | SB_VIS)>, WF_SHADE_THREADS, 0));
        else
            HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks_per_cu, k_wf_shade<false, false, true, SB_B0_CACHED>, WF_SHADE_THREADS, 0));
    });
}
int pt_scene_get_info(const pt_scene* scene, pt_scene_info* out) {
    if (!scene || !out) return PT_ERR_INVALID;
    *out = scene->info;
    grid_facts(scene->grids, *out);
    out->queue_bytes = scene->queue_bytes_last;
    out->queue_chunk_items = scene->queue_chunk_last;
    out->frame_planned = scene->frame_planned_last;
    return PT_OK;
}

int pt_trace_rays(const pt_scene* scene, const float* rays, uint64_t n, pt_hit* out) {
    return guarded([&] {
        if (!scene || !rays || !out) fail(PT_ERR_INVALID, "pt_trace_rays: null argument");
        if (n == 0) return;
        HIP_CHECK(hipSetDevice(scene->device));
        Staged<float> d_rays(rays, n * 6);
        Staged<pt_hit> d_out(nullptr, n);
        hipLaunchKernelGGL(k_trace, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, 0, scene->dev, d_rays.d, n, d_out.d);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipDeviceSynchronize());
        d_out.fetch(out, n);
    });
}

// The same through the WAVEFRONT integrator's own cast kernel (k_wf_trace: persistent lanes, resumable walk with the
// LDS stack and tree top, optional hand-over to k_wf_trace_wide) - the kernel the rays of bounces >= 1 of every frame
// go through.  mode bit 0: entry lists (trav_enter, the primitive each ray starts on in start_prims); bit 1: every
// cast is handed to k_wf_trace_wide as early as possible; bit 2: WITHOUT the hand-over of the rays the walker's slack does
// not cover to k_wf_trace_exact (study switch: the capped walk of round 3).
int pt_trace_rays_wavefront(const pt_scene* scene, const float* rays, const uint32_t* start_prims, uint64_t n, uint32_t mode, pt_hit* out) {
    return guarded([&] {
        if (!scene || !rays || !out) fail(PT_ERR_INVALID, "pt_trace_rays_wavefront: null argument");
        if ((mode & 1u) && !start_prims) fail(PT_ERR_INVALID, "pt_trace_rays_wavefront: mode 1 needs start_prims");
        if (n == 0) return;
        if (n >= (1ull << 28)) fail(PT_ERR_INVALID, "pt_trace_rays_wavefront: too many rays");
        HIP_CHECK(hipSetDevice(scene->device));
        const uint32_t cap = (uint32_t)((n + 63) & ~63ull);
        std::vector<float4> q((size_t)cap * 4 + (cap + 3) / 4, make_float4(0, 0, 0, 0));
        uint32_t* entry = (uint32_t*)(q.data() + (size_t)cap * 4);
        for (uint64_t i = 0; i < n; ++i) {
            const float* r = rays + 6 * i;
            uint32_t item = (uint32_t)i, draw = 1u << 16;
            float fi, fd;
            memcpy(&fi, &item, 4);
            memcpy(&fd, &draw, 4);
            q[2 * i] = make_float4(r[0], r[1], r[2], r[3]);
            q[2 * i + 1] = make_float4(r[4], r[5], fi, fd);
            if (mode & 1u) {
                if (start_prims[i] >= scene->dev.n_prims) fail(PT_ERR_INVALID, "pt_trace_rays_wavefront: start primitive out of range");
                entry[i] = scene->host_prim_entry[start_prims[i]];
            }
        }
        Staged<float4> d_q(q.data(), q.size());
        std::vector<WfCounters> ctr(3);
        memset(ctr.data(), 0, sizeof(WfCounters) * 3);
        ctr[1].queue_count = (uint32_t)n;
        Staged<WfCounters> d_ctr(ctr.data(), 3);
        Staged<uint4> d_hits(nullptr, (size_t)cap * 2);   // 4 B + 16 B per entry
        int n_cu = 0;
        HIP_CHECK(hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, scene->device));
        const uint32_t blocks = (uint32_t)std::max(1, n_cu) * 4u;
        Staged<uint32_t> d_def(nullptr, (size_t)blocks * WF_THREADS * 7);   // (index | carried hit | progress: wf_list_*)
        WfParams W{};
        W.n_items = (uint32_t)n;
        W.cap = W.qcap_in = W.qcap_out = W.hcap = W.scap = W.ecap = cap;
        W.bounce = 1;
        W.refill_min = 16;
        W.walk_steps = 12;
        W.defer_age = (mode & 2u) ? 1u : 0u;
        W.list_cap = blocks * WF_THREADS;
        W.use_entry = mode & 1u;
        W.exact_handover = (mode & 4u) ? 0u : 1u;   // (as in every frame: the rays the walker's slack does not cover go to k_wf_trace_exact)
        Staged<uint32_t> d_exact(nullptr, (size_t)cap * 2);
        hipLaunchKernelGGL((k_wf_trace<false, false, false>), dim3(blocks), dim3(WF_THREADS), 0, 0, scene->dev, W, (const uint32_t*)nullptr,
                           d_q.d, d_hits.d, (const uint4*)nullptr, (uint32_t*)nullptr, d_def.d, d_exact.d, d_ctr.d, (DevCounters*)nullptr);
        HIP_CHECK(hipGetLastError());
        if (W.exact_handover) {
            hipLaunchKernelGGL((k_wf_trace_exact<false, false, false>), dim3((uint32_t)std::max(1, n_cu) * 16u), dim3(WF_EXACT_THREADS), 0, 0, scene->dev, W,
                               (const uint32_t*)nullptr, (const float4*)d_q.d, d_hits.d, (const uint4*)nullptr, (uint32_t*)nullptr, d_exact.d,
                               (const WfCounters*)d_ctr.d, (DevCounters*)nullptr);
            HIP_CHECK(hipGetLastError());
        }
        if (W.defer_age) {
            hipLaunchKernelGGL((k_wf_trace_wide<false, false>), dim3((uint32_t)std::max(1, n_cu) * 4u * (WF_WIDE_LANES / 16u > 0u ? WF_WIDE_LANES / 16u : 1u)), dim3(WF_THREADS), 0, 0, scene->dev, W,
                               (const uint32_t*)nullptr, (const float4*)d_q.d, d_hits.d, (const uint4*)nullptr, (uint32_t*)nullptr,
                               (const uint32_t*)d_def.d, (const WfCounters*)d_ctr.d, (DevCounters*)nullptr);
            HIP_CHECK(hipGetLastError());
        }
        HIP_CHECK(hipDeviceSynchronize());
        std::vector<uint4> h((size_t)cap * 2);
        d_hits.fetch(h.data(), h.size());
        const uint32_t* word = (const uint32_t*)h.data();
        const uint4* rest = (const uint4*)(word + cap);
        for (uint64_t i = 0; i < n; ++i) {
            pt_hit& o = out[i];
            if (word[i] == 0xffffffffu) {
                o.prim = -1;
                o.flags = 0;
                o.dist = o.u = o.v = 0.f;
                continue;
            }
            const bool sphere = (word[i] & PT_PRIM_SPHERE) != 0;
            o.prim = (int32_t)(word[i] & 0x0fffffffu);
            o.flags = (int32_t)(((word[i] >> 30) & 1u) | (sphere ? 2u : 0u) | (((word[i] >> 29) & 1u) << 2));
            memcpy(&o.dist, &rest[i].x, 4);
            memcpy(&o.u, &rest[i].y, 4);
            memcpy(&o.v, &rest[i].z, 4);
            if (sphere) o.u = o.v = 0.f;
        }
    });
}

int pt_scene_escape_copy(const pt_scene* scene, void* out, uint64_t bytes) {
    return guarded([&] {
        if (!scene || !out) fail(PT_ERR_INVALID, "pt_scene_escape_copy: null argument");
        if (!scene->dev.escape && scene->escape_wanted && !scene->escape_tried) escape_masks_build(render_state(scene));
        if (!scene->dev.escape) fail(PT_ERR_INVALID, "pt_scene_escape_copy: the scene has no escape masks");
        if (bytes != (uint64_t)scene->dev.n_prims * 80u) fail(PT_ERR_INVALID, "pt_scene_escape_copy: %llu bytes expected", (unsigned long long)scene->dev.n_prims * 80ull);
        HIP_CHECK(hipSetDevice(scene->device));
        HIP_CHECK(hipMemcpy(out, scene->dev.escape, bytes, hipMemcpyDeviceToHost));
    });
}

int pt_escape_query(const pt_scene* scene, const uint32_t* prims, const float* rays, uint64_t n, uint8_t* proven) {
    return guarded([&] {
        if (!scene || !prims || !rays || !proven) fail(PT_ERR_INVALID, "pt_escape_query: null argument");
        if (!scene->dev.escape && scene->escape_wanted && !scene->escape_tried) escape_masks_build(render_state(scene));
        if (!scene->dev.escape) fail(PT_ERR_INVALID, "pt_escape_query: the scene has no escape masks");
        for (uint64_t i = 0; i < n; ++i)   // (before anything is launched: the kernel indexes the records with them)
            if (prims[i] >= scene->dev.n_prims) fail(PT_ERR_INVALID, "pt_escape_query: primitive %u out of range", prims[i]);
        if (n == 0) return;
        if (n >= (1ull << 31)) fail(PT_ERR_INVALID, "pt_escape_query: too many queries");
        HIP_CHECK(hipSetDevice(scene->device));
        Staged<uint32_t> d_prims(prims, n);
        Staged<float> d_rays(rays, n * 6);
        Staged<uint8_t> d_out(nullptr, n);
        hipLaunchKernelGGL(k_escape_query, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, 0, scene->dev, d_prims.d, d_rays.d, n, d_out.d);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipDeviceSynchronize());
        d_out.fetch(proven, n);
    });
}

int pt_scene_grid_header(const pt_scene* scene, uint32_t which, pth_origin_grid* out) {
    return guarded([&] {
        if (!scene || !out) fail(PT_ERR_INVALID, "pt_scene_grid_header: null argument");
        memset(out, 0, sizeof *out);
        const GridSlot* slot = scene->grids.slot(which);
        if (scene->grids.headers && slot) *out = slot->hdr;
        out->cell_off = nullptr;
        out->refs = nullptr;
    });
}

int pt_scene_grid_copy(const pt_scene* scene, uint32_t which, uint32_t* cell_off, pth_grid_ref* refs) {
    return guarded([&] {
        if (!scene || !cell_off || !refs) fail(PT_ERR_INVALID, "pt_scene_grid_copy: null argument");
        const GridSlot* slot = scene->grids.slot(which);
        if (!scene->grids.headers || !slot || !slot->hdr.enabled) fail(PT_ERR_INVALID, "pt_scene_grid_copy: no such grid");
        const pth_origin_grid& h = slot->hdr;
        const DevGrid& g = slot->dev;
        HIP_CHECK(hipSetDevice(scene->device));
        HIP_CHECK(hipMemcpy(cell_off, g.cell_off, (h.n_cells + 1) * 4, hipMemcpyDeviceToHost));
        if (h.n_refs) HIP_CHECK(hipMemcpy(refs, g.refs, h.n_refs * 8, hipMemcpyDeviceToHost));
    });
}

int pt_trace_rays_all(const pt_scene* scene, const float* rays, uint64_t n, uint32_t max_hits, pt_hit* out,
                      uint32_t* counts) {
    return guarded([&] {
        if (!scene || !rays || !out || !counts || !max_hits) fail(PT_ERR_INVALID, "pt_trace_rays_all: bad argument");
        if (n == 0) return;
        HIP_CHECK(hipSetDevice(scene->device));
        Staged<float> d_rays(rays, n * 6);
        Staged<pt_hit> d_out(nullptr, n * max_hits);
        Staged<uint32_t> d_cnt(nullptr, n);
        hipLaunchKernelGGL(k_trace_all, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, 0, scene->dev, d_rays.d, n,
                           max_hits, d_out.d, d_cnt.d);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipDeviceSynchronize());
        d_out.fetch(out, n * max_hits);
        d_cnt.fetch(counts, n);
    });
}

int pt_intersect_triangles(int device, const float* rays, const float* tris, uint64_t n, pt_hit* out) {
    return guarded([&] {
        if (!rays || !tris || !out) fail(PT_ERR_INVALID, "pt_intersect_triangles: null argument");
        if (n == 0) return;
        select_device(device);
        Staged<float> d_rays(rays, n * 6), d_tris(tris, n * 9);
        Staged<pt_hit> d_out(nullptr, n);
        hipLaunchKernelGGL(k_isect, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, 0, d_rays.d, d_tris.d, n, d_out.d);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipDeviceSynchronize());
        d_out.fetch(out, n);
    });
}

int pt_rng_words(int device, const uint64_t* seeds, uint64_t n_seeds, uint32_t n_words, uint32_t* out) {
    return guarded([&] {
        if (!seeds || !out) fail(PT_ERR_INVALID, "pt_rng_words: null argument");
        if (n_seeds == 0 || n_words == 0) return;
        select_device(device);
        Staged<uint64_t> d_seeds(seeds, n_seeds);
        Staged<uint32_t> d_out(nullptr, n_seeds * n_words);
        hipLaunchKernelGGL(k_rng, dim3((uint32_t)((n_seeds + 255) / 256)), dim3(256), 0, 0, d_seeds.d, n_seeds, n_words, d_out.d);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipDeviceSynchronize());
        d_out.fetch(out, n_seeds * n_words);
    });
}

int pt_eval_math(int device, int fn, const float* x, uint64_t n, float* out) {
    return guarded([&] {
        if (!x || !out) fail(PT_ERR_INVALID, "pt_eval_math: null argument");
        if (fn < 0 || fn > 3) fail(PT_ERR_INVALID, "pt_eval_math: unknown function %d", fn);
        if (n == 0) return;
        select_device(device);
        Staged<float> d_x(x, n), d_out(nullptr, n);
        hipLaunchKernelGGL(k_math, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, 0, fn, d_x.d, n, d_out.d);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipDeviceSynchronize());
        d_out.fetch(out, n);
    });
}

int pt_measure_copy_bandwidth(int device, uint64_t bytes, uint32_t reps, double* gb_per_s) {
    return guarded([&] {
        if (!gb_per_s) fail(PT_ERR_INVALID, "pt_measure_copy_bandwidth: null argument");
        if (bytes < 16 || reps == 0) fail(PT_ERR_INVALID, "pt_measure_copy_bandwidth: bytes >= 16 and reps >= 1 required");
        select_device(device);
        uint64_t n = bytes / 16;
        Staged<float4> src(nullptr, n), dst(nullptr, n);
        HIP_CHECK(hipMemset(src.d, 1, n * 16));
        if (n > (1ull << 40)) fail(PT_ERR_INVALID, "pt_measure_copy_bandwidth: at most 16 TiB");
        uint32_t grid = (uint32_t)((n + 1023) / 1024);
        hipEvent_t e0, e1;
        HIP_CHECK(hipEventCreate(&e0));
        HIP_CHECK(hipEventCreate(&e1));
        float best = INFINITY;
        for (uint32_t r = 0; r <= reps; ++r) {  // the first pass only touches the pages
            HIP_CHECK(hipEventRecord(e0, 0));
            hipLaunchKernelGGL(k_stream_copy, dim3(grid), dim3(256), 0, 0, src.d, dst.d, n);
            HIP_CHECK(hipEventRecord(e1, 0));
            HIP_CHECK(hipEventSynchronize(e1));
            float ms = 0.f;
            HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
            if (r > 0 && ms < best) best = ms;
        }
        (void)hipEventDestroy(e0);
        (void)hipEventDestroy(e1);
        HIP_CHECK(hipGetLastError());
        *gb_per_s = 2.0 * (double)(n * 16) / ((double)best * 1e-3) / 1e9;
    });
}

int pt_measure_gather_rate(int device, uint64_t table_bytes, uint32_t bytes_per_load, uint32_t loads_per_lane,
                           double* giga_loads_per_s) {
    return guarded([&] {
        if (!giga_loads_per_s) fail(PT_ERR_INVALID, "pt_measure_gather_rate: null argument");
        if (bytes_per_load != 8 && bytes_per_load != 16) fail(PT_ERR_INVALID, "pt_measure_gather_rate: 8 or 16 bytes per load");
        if (table_bytes < 4096 || loads_per_lane < 8) fail(PT_ERR_INVALID, "pt_measure_gather_rate: table >= 4 KiB, loads >= 8");
        select_device(device);
        uint64_t slots = 1;
        while (slots * 2 * 16 <= table_bytes) slots *= 2;   // power of two 16-byte slots
        Staged<uint4> table(nullptr, slots);
        Staged<uint32_t> sink(nullptr, 4);
        HIP_CHECK(hipMemset(table.d, 0x5a, slots * 16));
        int n_cu = 0;
        HIP_CHECK(hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, device));
        const uint32_t grid = (uint32_t)n_cu * 8u, rounds = loads_per_lane / 8u;   // 8 workgroups of 256 per CU
        hipEvent_t e0, e1;
        HIP_CHECK(hipEventCreate(&e0));
        HIP_CHECK(hipEventCreate(&e1));
        float best = INFINITY;
        for (int r = 0; r < 4; ++r) {
            HIP_CHECK(hipEventRecord(e0, 0));
            if (bytes_per_load == 16)
                hipLaunchKernelGGL(k_gather<16>, dim3(grid), dim3(256), 0, 0, table.d, (uint32_t)(slots - 1), rounds, sink.d);
            else
                hipLaunchKernelGGL(k_gather<8>, dim3(grid), dim3(256), 0, 0, table.d, (uint32_t)(slots - 1), rounds, sink.d);
            HIP_CHECK(hipEventRecord(e1, 0));
            HIP_CHECK(hipEventSynchronize(e1));
            float ms = 0.f;
            HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
            if (r > 0 && ms < best) best = ms;
        }
        (void)hipEventDestroy(e0);
        (void)hipEventDestroy(e1);
        HIP_CHECK(hipGetLastError());
        *giga_loads_per_s = (double)grid * 256.0 * (double)rounds * 8.0 / ((double)best * 1e-3) / 1e9;
    });
}

}  // extern "C"
