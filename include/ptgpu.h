/*
 * ptgpu.h — C ABI of the MI355X path-tracing integrator (libptgpu.so).
 *
 * This is the drop-in boundary for the per-pixel sampling hot path of
 * flomonster/path-tracer.  The reference has no FFI; the narrowest seam is
 *
 *     Renderer::new(&RenderConfig, Profile)            src/renderer/mod.rs:61-73
 *     Renderer::render(&self, &Scene) -> RgbImage      src/renderer/mod.rs:76-169
 *
 * called from run_render (src/main.rs:46-47) and the golden-image test helper
 * (src/main.rs:79).  A Rust host would bind exactly the functions declared
 * here (see INTEGRATION.md for the `extern "C"` block); the C++ host in
 * path-tracer_amd/host/ uses them the same way.
 *
 * Everything is plain C: POD structs, pointers and sizes.  The caller owns all
 * host buffers; the library copies the scene to the device in
 * pt_scene_create() and owns device memory until pt_scene_destroy().
 *
 * All functions return 0 on success and a negative pt_status on failure;
 * pt_last_error() returns a thread-local message (the CLI maps any failure to
 * exit code 2 like src/main.rs:14-22).
 */
#ifndef PTGPU_H
#define PTGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------ */
/* status codes                                                        */
/* ------------------------------------------------------------------ */
enum pt_status {
    PT_OK = 0,
    PT_ERR_INVALID = -1,   /* bad argument / malformed scene            */
    PT_ERR_IO = -2,        /* file could not be read / written          */
    PT_ERR_PARSE = -3,     /* JSON / YAML / PNG syntax                  */
    PT_ERR_DEVICE = -4,    /* HIP runtime failure, no GPU               */
    PT_ERR_NUMERIC = -5,   /* NaN hit distance etc. (reference panics:  */
                           /* src/renderer/utils.rs:19)                 */
    PT_ERR_UNSUPPORTED = -6
};

/* ------------------------------------------------------------------ */
/* scene description: flat mirror of src/scene/internal/{mod,model,    */
/* material,light,camera,vertex,triangle}.rs                           */
/* ------------------------------------------------------------------ */

enum { PT_MODEL_MESH = 0, PT_MODEL_SPHERE = 1 };     /* internal/model.rs:10-21 */
enum { PT_LIGHT_POINT = 0, PT_LIGHT_DIRECTIONAL = 1 }; /* internal/light.rs:6-17 */
enum { PT_BRDF_COOK_TORRANCE = 0 };                  /* renderer/brdf/mod.rs:50-55 */
enum { PT_TONEMAP_REINHARD = 0, PT_TONEMAP_FILMIC = 1, PT_TONEMAP_ACES = 2 }; /* tonemap.rs:5-13 */

/* One decoded texture (image crate: into_rgb8() → 3 channels,
 * into_luma8() → 1 channel; internal/texture_bank.rs:21-51).  Row 0 is the
 * top row; texels are tightly packed u8. */
typedef struct pt_texture {
    uint64_t offset;    /* byte offset into pt_scene_desc.texels */
    uint32_t width;
    uint32_t height;
    uint32_t channels;  /* 1 or 3 */
    uint32_t _pad;
} pt_texture;

/* internal/material.rs:11-26.  tex_* = index into textures or -1. */
typedef struct pt_material {
    float albedo[3];
    float emissive[3];
    float opacity;
    float metalness;
    float roughness;
    float ior;
    int32_t tex_albedo;     /* rgb  */
    int32_t tex_emissive;   /* rgb  */
    int32_t tex_opacity;    /* luma */
    int32_t tex_metalness;  /* luma */
    int32_t tex_roughness;  /* luma */
    int32_t tex_normal;     /* rgb  */
} pt_material;

/* internal/model.rs:10-21.  Meshes own triangles [tri_first, tri_first+tri_count)
 * of pt_scene_desc.triangles; spheres use center/radius. */
typedef struct pt_model {
    int32_t kind;       /* PT_MODEL_* */
    int32_t material;   /* index into materials */
    uint32_t tri_first;
    uint32_t tri_count;
    float center[3];
    float radius;
} pt_model;

/* internal/light.rs:6-17.  vec = position (point) or direction (directional). */
typedef struct pt_light {
    int32_t kind;       /* PT_LIGHT_* */
    float vec[3];
    float color[3];
    float size;         /* unused by the integrator (hard shadows) */
} pt_light;

/* internal/camera.rs:7-48.  transform[4*k + r] = column k, row r (ISF
 * "transform"[k] is column k, cgmath Matrix4 layout). */
typedef struct pt_camera {
    float transform[16];
    float fov;          /* radians */
    float zfar;
    float znear;
} pt_camera;

/* internal/mod.rs:26-32.  triangles: 24 f32 per triangle in ISF order
 * (position3, normal3, tex_coords2) x 3 vertices; models reference
 * contiguous ranges in model order, so the global triangle index is the
 * reference's (model index, triangle index) order. */
typedef struct pt_scene_desc {
    uint32_t n_models;
    uint32_t n_materials;
    uint32_t n_textures;
    uint32_t n_lights;
    uint64_t n_triangles;
    uint64_t n_texel_bytes;
    const pt_model* models;
    const pt_material* materials;
    const pt_texture* textures;
    const pt_light* lights;
    const float* triangles;
    const uint8_t* texels;
    pt_camera camera;
    float background[3];
    uint32_t _pad;
} pt_scene_desc;

/* config/profile.rs:10-25 (defaults 1920x1080, bounces 4, samples 64,
 * COOK_TORRANCE, FILMIC). */
typedef struct pt_profile {
    uint32_t width;
    uint32_t height;
    uint32_t samples;
    uint32_t bounces;
    int32_t brdf;
    int32_t tonemap;
} pt_profile;

/* pt_opts.flags */
enum {
    PT_FLAG_TIMING = 1u << 0,   /* record HIP events around every kernel launch */
    PT_FLAG_COUNTERS = 1u << 1, /* run the instrumented kernel variant (ray /
                                   node / triangle counters; not for timing)  */
    PT_FLAG_NO_GRIDS = 1u << 2, /* cast camera and shadow rays through the KD-tree like every other ray
                                   (A/B measurements; the parity tests compare the two paths)          */
    PT_FLAG_MEGAKERNEL = 1u << 3, /* the one-lane-per-pixel integrator (k_render): a second, independent
                                   implementation of the path for cross-checks; ~10x slower            */
};

/* Which pixels this call renders.  The image is cut into tile_w x tile_h
 * tiles numbered row-major (k = ty * tiles_x + tx); this call renders the tiles
 * with (tx + ty * s) % shard_count == shard_rank - diagonal
 * stripes, s = the smallest odd number >= 3 coprime to shard_count (1 for two
 * ranks: a checkerboard), so that every rank takes tiles from every column and
 * row of the image (pt_local_pixel_map gives the exact map).  Every pixel keeps its GLOBAL
 * index i = x + y*W in the seed formula (renderer/mod.rs:110-112), so any
 * sharding is bit-identical to the unsharded render.  Output buffers are
 * PACKED in local order: tiles in ascending k, row-major inside a tile
 * (clipped at the image border).  shard_count <= 1 means the whole image in
 * plain row-major order. */
typedef struct pt_opts {
    uint32_t flags;
    int32_t device;        /* HIP device ordinal; -1 = current */
    uint32_t shard_rank;
    uint32_t shard_count;
    uint32_t tile_w;       /* 0 -> 32 */
    uint32_t tile_h;       /* 0 -> 32 */
    uint32_t sample_batch; /* samples per kernel launch; 0 = library default */
    uint32_t _pad;
    void (*progress)(uint32_t done_samples, uint32_t total_samples, void* user);
    void* progress_user;
    /* Progressive output (the reference's viewer feed, renderer/mod.rs:133-141: every pixel is sent as
     * post_processing(pixel / current_sample)).  When set, pt_render() calls it after every sample batch
     * with the packed RGB8 image of the samples done so far (same layout as the rgb8 result, valid only
     * during the call).  Host-buffer entry point only. */
    void (*preview)(const uint8_t* rgb8, uint64_t n_pixels, uint32_t done_samples, uint32_t total_samples, void* user);
    void* preview_user;
} pt_opts;

typedef struct pt_scene pt_scene;

/* ------------------------------------------------------------------ */
/* the hot path                                                        */
/* ------------------------------------------------------------------ */

/* Upload a scene: builds the KD-tree (replaces kdtree-ray),
 * the sRGB->linear table, and copies everything to the device. */
int pt_scene_create(const pt_scene_desc* desc, int device, pt_scene** out);
void pt_scene_destroy(pt_scene* scene);

/* Give a scene another camera.  Afterwards every render entry point (pt_render, pt_render_device, pt_render_gathered,
 * sharded calls), pt_debug_render and the grid / escape-mask test hooks behave exactly as on a scene that pt_scene_create
 * made with this camera: the same images bit for bit.  Accepts the cameras pt_scene_create accepts; a null argument is
 * PT_ERR_INVALID.  Works on scenes made by pt_scene_create_from_prep, also after pt_prep_destroy (the scene keeps what the
 * camera grid needs, in host memory).
 * The call synchronises the scene's device before it replaces anything: a frame already queued by pt_render_device
 * completes with the old camera.  The caller must not enqueue work on the scene from another thread during the call.
 * The camera grid is rebuilt on the device; without the memory for it the camera goes without one (camera rays take
 * the KD-tree, as on a fresh scene in that situation) and the call succeeds.  Any other device failure returns
 * PT_ERR_DEVICE and leaves the scene rendering the OLD camera.  With PT_OG_HOST=1 (grids built on the host) a moved
 * camera goes without a camera grid.  Every later frame runs as the first frame of its configuration (no frame plan
 * carries over); the escape masks are kept where they still prove their misses, otherwise rebuilt on the schedule of a
 * fresh scene (PT_ESCAPE_AFTER). */
int pt_scene_set_camera(pt_scene* scene, const pt_camera* camera);

/* Replace ALL lights of a scene (n_lights may differ from the count it was made with; 0 is allowed, lights may be NULL only
 * then), or its material table (n_materials must equal the n_materials of the description the scene was made from; the
 * model -> material assignment and the textures are kept; a texture index must be -1 or name one of the scene's textures
 * with the channel count pt_scene_create demands).  Afterwards every entry point behaves exactly as on a scene that
 * pt_scene_create made from the edited description, with the same contract as pt_scene_set_camera: the device is
 * synchronised first (a frame already queued by pt_render_device completes with the old lights / materials), works on
 * scenes of pt_scene_create_from_prep also after pt_prep_destroy (scenes of one prep are edited independently), and no
 * frame plan or captured graph carries over.  A null pointer with a count > 0, a wrong material count, a light kind other
 * than PT_LIGHT_*, a texture index out of range or with the wrong channel count are PT_ERR_INVALID; any other device
 * failure is PT_ERR_DEVICE; in both cases the scene keeps rendering its old state bit for bit.
 * set_lights rebuilds the light origin grids on the device (all or none, as pt_scene_create: a light whose grid is not to
 * be had sends every shadow ray through the KD-tree) and the camera grid only if the new light count changes its
 * resolution (PT_OG_BUDGET_GIB).  With PT_OG_HOST=1 (grids built on the host) the edited scene goes without light grids.
 * set_materials replaces the per-model materials the device reads and re-evaluates has_translucent (the ALPHA variants).
 * The escape masks are kept by both: they depend on the geometry and the camera only. */
int pt_scene_set_lights(pt_scene* scene, const pt_light* lights, uint32_t n_lights);
int pt_scene_set_materials(pt_scene* scene, const pt_material* materials, uint32_t n_materials);

/* The host half of pt_scene_create (validation, KD build, origin grids) as an object of its own: build it ONCE
 * and upload it to every device of a multi-GPU render instead of repeating seconds of CPU work per device. */
typedef struct pt_prep pt_prep;
int pt_prep_create(const pt_scene_desc* desc, pt_prep** out);
void pt_prep_destroy(pt_prep* prep);
int pt_scene_create_from_prep(const pt_prep* prep, int device, pt_scene** out);

/* Number of pixels pt_render writes for (profile, opts). */
uint64_t pt_local_pixel_count(const pt_profile* profile, const pt_opts* opts);
/* local packed index -> global pixel index i = x + y*W; out has
 * pt_local_pixel_count entries.  Host helper (no GPU needed). */
int pt_local_pixel_map(const pt_profile* profile, const pt_opts* opts, uint32_t* out);

/* Renderer::render (renderer/mod.rs:76-169) for this call's pixels.
 * rgb8:  n_local*3 bytes, tone-mapped + gamma + u8 (mod.rs:335-353)  [may be NULL]
 * accum: n_local*3 f32, SUM of sample radiance before the division by
 *        `samples` (the reference's `buffer`, mod.rs:81,130)          [may be NULL]
 * Both are HOST pointers; the call blocks until the image is complete. */
int pt_render(const pt_scene* scene, const pt_profile* profile, const pt_opts* opts,
              uint8_t* rgb8, float* accum);

/* Same, with DEVICE pointers (hipMalloc'd or torch CUDA tensors) and a
 * hipStream_t passed as void*.  Asynchronous with respect to the host
 * unless PT_FLAG_TIMING is set; the caller synchronises the stream. */
int pt_render_device(const pt_scene* scene, const pt_profile* profile, const pt_opts* opts,
                     void* d_rgb8, void* d_accum, void* hip_stream);

/* Scatter packed per-rank framebuffers (as produced by an all-gather of
 * equal-sized, zero-padded packed slices; slice r starts at r*slice_pixels)
 * into a row-major W*H image.  elem_bytes = 3 (rgb8) or 12 (f32 rgb).
 * Device pointers; hip_stream as above. */
int pt_assemble_tiles(const pt_profile* profile, uint32_t shard_count, uint32_t tile_w,
                      uint32_t tile_h, uint64_t slice_pixels, uint32_t elem_bytes,
                      const void* d_gathered, void* d_image, void* hip_stream);

/* The exchange step of a multi-GPU render inside the library: one RCCL ncclAllGather over xGMI of
 * the packed, zero-padded u8 (or f32) framebuffer slices + the scatter of pt_assemble_tiles, on `hip_stream`.
 * Communicators: one process per GPU - rank 0 calls pt_comm_unique_id, the host's own bootstrap (MPI, a TCP
 * store, torch.distributed) hands the 128 bytes to the other ranks, every rank calls pt_comm_create; one process
 * driving several GPUs - pt_comm_create_all (ncclCommInitAll; `out` receives n handles, devices must be distinct).
 * librccl.so is loaded on first use.  The reference has no counterpart (single process, rayon). */
enum { PT_COMM_ID_BYTES = 128 };
typedef struct pt_comm pt_comm;
int pt_comm_unique_id(uint8_t id[PT_COMM_ID_BYTES]);
int pt_comm_create(const uint8_t id[PT_COMM_ID_BYTES], int rank, int size, int device, pt_comm** out);
int pt_comm_create_all(const int* devices, int n, pt_comm** out);
void pt_comm_destroy(pt_comm* comm);
/* d_local: this rank's slice_pixels * elem_bytes packed slice; d_gathered: scratch of size * that; d_image: the
 * row-major W*H*elem_bytes frame, complete on every rank when the stream has drained.  Device pointers. */
int pt_gather_tiles(pt_comm* comm, const pt_profile* profile, uint32_t tile_w, uint32_t tile_h,
                    uint64_t slice_pixels, uint32_t elem_bytes, const void* d_local, void* d_gathered,
                    void* d_image, void* hip_stream);

/* Renderer::render on this rank's shard + the gather, host-buffer form: renders (profile, opts) on the device,
 * all-gathers the slices (slice_pixels = the largest pt_local_pixel_count of any rank) and, when rgb8_frame is not
 * NULL, copies the complete row-major RGB8 frame (W*H*3 bytes) to the host.  Every rank of the communicator must
 * call it; opts->shard_rank / shard_count must be the communicator's rank / size. */
int pt_render_gathered(const pt_scene* scene, pt_comm* comm, const pt_profile* profile, const pt_opts* opts,
                       uint64_t slice_pixels, uint8_t* rgb8_frame);

/* `--debug-textures` (src/renderer/debug_renderer.rs:11-105): one pixel-centre primary ray per
 * pixel, first entry of ray_cast() only, seven RGB8 planes of width*height*3 bytes each, in this
 * order: normal (n*0.5+0.5), albedo, opacity, metalness, roughness, emissive, ior/3 — each channel
 * `(v * 255.) as u8`, pixels without a hit stay 0.  *any_hit = 0 means no pixel hit anything (the
 * reference then writes no file at all).  planes is a HOST pointer. */
enum { PT_DEBUG_PLANES = 7 };
int pt_debug_render(const pt_scene* scene, uint32_t width, uint32_t height, uint8_t* planes, int* any_hit);

/* ------------------------------------------------------------------ */
/* denoised previews (no reference counterpart)             */
/* ------------------------------------------------------------------ */

/* Guide planes: the first hit of the pixel-centre ray at float precision (what pt_debug_render quantises to u8).
 * Per pixel i = x + y*W, 8 f32: [0..2] shading normal exactly as the debug pass computes it (NOT normalised for
 * triangles, flipped on back faces), [3] depth = the `dist` pt_trace_rays reports for the first entry of ray_cast() of the
 * pixel-centre ray (r1 = r2 = 0.5), [4..6] MaterialSample albedo, [7] the global primitive index (pt_hit.prim) as int32 bits.
 * A pixel whose ray hits nothing: floats 0, depth -1.0f, prim -1.  Translucent first surfaces are reported as they are.
 * Follows pt_scene_set_camera and the scene edits like pt_debug_render.  d_guides: 16-byte aligned device memory. */
enum { PT_GUIDE_FLOATS = 8 };
int pt_render_guides(const pt_scene* scene, uint32_t width, uint32_t height, float* guides /* host */);
int pt_render_guides_device(const pt_scene* scene, uint32_t width, uint32_t height, void* d_guides, void* hip_stream);

/* Edge-avoiding a-trous wavelet filter (Dammertz et al. 2010) over the accumulator, steered by the guides.  All f32, one
 * IEEE operation per step in the order written, no transcendental function (tests/denoise_model.py restates it bit for bit):
 *   prep    valid = depth >= 0;  c = accum / (float)samples;  an invalid pixel outputs c and is never a tap.
 *           u = normalize(n) (0 when n.n is 0 or not finite);  d = albedo + 0.01 (1 with NO_DEMODULATE);  x = c / d;
 *           gx = min(|z(x+1) - z|, |z - z(x-1)|) over the valid in-image neighbours (one: that difference; none: 0), gy alike.
 *   pass i  s = 2^i.  acc = 0, wsum = 0; dy = -2..2 outer, dx = -2..2 inner, q = p + s*(dx, dy) in the image and valid:
 *           k = h[|dx|] * h[|dy|], h = {3/8, 1/4, 1/16};  centre tap: w = k;  any other tap:
 *             wn = max(0, u_p.u_q) squared normal_power_log2 times
 *             den = sigma_depth * (gx_p * (float)(s*|dx|) + gy_p * (float)(s*|dy|)) + 1e-4f * z_p;  wz = wexp(|z_p - z_q| / den)
 *             sc = sigma_color * 2^-i;  wc = sigma_color == 0 ? 1 : wexp(|x_p - x_q|^2 / (sc * sc))  (x of this pass's input)
 *             w = ((k * wn) * wz) * wc
 *           acc += x_q * w, wsum += w;  the pass writes acc / wsum.
 *           wexp(e): r = max(0, 1 - e * 0.125f), squared three times (compact-support stand-in for exp(-e); NaN / inf: 0)
 *   finish  out = x * d (x with NO_DEMODULATE);  rgb8 = as_u8(pow(tonemap(out), 1/2.2) * 255) like pt_render.
 * iterations = 0: out = c for every pixel (no demodulation round trip): out_rgb8 equals pt_render's rgb8 bit for bit.
 * Non-finite accumulator values are outside the contract (a NaN sample spreads to the pixels whose taps reach it). */
enum { PT_DENOISE_NO_DEMODULATE = 1 };
typedef struct pt_denoise_params {
    uint32_t iterations;         /* a-trous passes, pass i has step 2^i; 0..8; 0 = no filtering at all */
    uint32_t flags;              /* PT_DENOISE_NO_DEMODULATE = 1 */
    uint32_t normal_power_log2;  /* normal weight = max(0, n_p.n_q)^(2^this); 0..10 */
    int32_t  tonemap;            /* PT_TONEMAP_* for the rgb8 output */
    float sigma_color;           /* 0 = colour weight off */
    float sigma_depth;           /* > 0 */
} pt_denoise_params;
/* The defaults: the best of the grid tools/measure_denoise_gain.py searched (tests/golden/denoise_gain.json), FILMIC. */
#define PT_DENOISE_DEFAULT_ITERATIONS 1
#define PT_DENOISE_DEFAULT_NORMAL_POWER_LOG2 3
#define PT_DENOISE_DEFAULT_SIGMA_COLOR 0.5f
#define PT_DENOISE_DEFAULT_SIGMA_DEPTH 0.5f
void pt_denoise_params_default(pt_denoise_params* params);

uint64_t pt_denoise_scratch_bytes(uint32_t width, uint32_t height);
/* accum: W*H*3 f32 SUM of samples (pt_render's accum, row-major, unsharded); guides: W*H*8 f32 as above;
 * out_color: W*H*3 f32 mean radiance [may be NULL]; out_rgb8: W*H*3 [may be NULL].  The host form allocates its own scratch
 * and blocks; the device form takes the caller's scratch (pt_denoise_scratch_bytes, 256-byte aligned), allocates nothing and
 * is asynchronous on hip_stream.  device: HIP ordinal, -1 = current.  PT_ERR_INVALID: a null required pointer,
 * width * height == 0, samples == 0, a parameter outside its range, sigma_depth not positive and finite, sigma_color negative
 * or not finite. */
int pt_denoise(int device, uint32_t width, uint32_t height, uint32_t samples, const pt_denoise_params* params,
               const float* accum, const float* guides, float* out_color, uint8_t* out_rgb8);
int pt_denoise_device(int device, uint32_t width, uint32_t height, uint32_t samples, const pt_denoise_params* params,
                      const void* d_accum, const void* d_guides, void* d_out_color, void* d_out_rgb8,
                      void* d_scratch, void* hip_stream);
/* pt_render + guides + denoise without leaving the device; rgb8 / color are host pointers, either may be NULL.  The preview
 * callback of opts receives the RAW frames.  shard_count > 1 is PT_ERR_UNSUPPORTED (the filter needs the whole image). */
int pt_render_denoised(const pt_scene* scene, const pt_profile* profile, const pt_opts* opts,
                       const pt_denoise_params* params, uint8_t* rgb8, float* color);
/* Measurement: pt_denoise_device on the null stream with HIP events between its kernels; blocks.  ms[0] = prep,
 * ms[1 + i] = pass i, ms[9] = finish; stages that did not run are 0. */
enum { PT_DENOISE_STAGES = 10 };
int pt_denoise_stage_times(int device, uint32_t width, uint32_t height, uint32_t samples, const pt_denoise_params* params,
                           const void* d_accum, const void* d_guides, void* d_out_color, void* d_out_rgb8,
                           void* d_scratch, float* ms);

/* ------------------------------------------------------------------ */
/* sample moments and the variance-guided filter           */
/* ------------------------------------------------------------------ */

/* pt_render / pt_render_device that also report the first two moments of every pixel's sample LUMINANCE,
 *     lum(a) = (0.2126f*a.r + 0.7152f*a.g) + 0.0722f*a.b.
 * moments: n_local x 2 f32 in the packed local order of accum (shards as in pt_render): [0] = m1, [1] = m2.  Both start at 0.f
 * and are built in sample order s = 0..N-1 from the radiance c_s of the sample (the value that is added to accum):
 *     L = lum(c_s);  m1 = m1 + L;  m2 = m2 + L*L        (each step one f32 operation, in this order)
 * A pixel of a block the camera-grid cull found empty uses the background value that accum gets for it, once per sample.
 * rgb8 and accum [either may be NULL] equal pt_render's bit for bit; moments is required.  The device form has the contract of
 * pt_render_device (d_moments: 8-byte aligned).  The frame runs the same launches on the same queues as pt_render's (one
 * kernel, k_accumulate_moments, takes the place of k_accumulate), so later frames - planned ones included - are unchanged.
 * Pipelines that stage no samples (PT_FLAG_MEGAKERNEL) return PT_ERR_UNSUPPORTED before any device work. */
int pt_render_moments(const pt_scene* scene, const pt_profile* profile, const pt_opts* opts,
                      uint8_t* rgb8, float* accum, float* moments);
int pt_render_moments_device(const pt_scene* scene, const pt_profile* profile, const pt_opts* opts,
                             void* d_rgb8, void* d_accum, void* d_moments, void* hip_stream);
/* Test hook: the radiance of every sample on its own.  samples (HOST): profile.samples x n_local x 3 f32, sample s of packed
 * pixel p at (s*n_local + p)*3; pixels of culled blocks hold the background value.  Summed in sample order they give accum;
 * the moments above are held to a restatement over these planes bit for bit.  PT_ERR_INVALID when the planes would exceed
 * 256 MiB, PT_ERR_UNSUPPORTED as for pt_render_moments. */
int pt_render_samples(const pt_scene* scene, const pt_profile* profile, const pt_opts* opts, float* samples /* host */);

/* The a-trous filter of pt_denoise with a colour weight steered by the per-pixel variance of the mean (SVGF's guide, Schied et
 * al. 2017, without its temporal part).  All f32, one IEEE operation per step in the order written (IEEE divide and sqrt;
 * tests/denoise_var_model.py restates it bit for bit):
 *   prep    valid, c, u, d, x, gx, gy exactly as pt_denoise's prep.
 *           N = (float)samples;  mu = m1 / N;  e2 = m2 / N;  s2 = max(0, e2 - mu*mu);  vL = s2 / (float)(samples - 1)
 *           v = vL / (lum(d) * lum(d))   (NO_DEMODULATE: v = vL);  an invalid pixel: v = 0
 *   pass i  s = 2^i.  Variance blur at UNIT spacing: b = 0, bs = 0; dy = -1..1 outer, dx = -1..1 inner, q = p + (dx, dy) in the
 *           image and valid: g = {1/4, 1/8, 1/16}[|dx| + |dy|];  b += v_q * g;  bs += g.   vb = b / bs
 *           lden = sigma_color * sqrt(vb) + 1e-6f
 *           taps, k, wn, wz, the skipping of invalid / out-of-image taps and the tap order as in pt_denoise's pass i;
 *           wl = wexp(|lum(x_p) - lum(x_q)| / lden);  centre tap w = k, any other w = ((k * wn) * wz) * wl
 *           acc += x_q * w;  wsum += w;  vacc += v_q * (w * w)
 *           the pass writes x = acc / wsum and v = vacc / (wsum * wsum)   (x and v of this pass's INPUT on the right-hand sides)
 *   finish  as pt_denoise.   iterations = 0: as pt_denoise with iterations = 0.
 * The functions take pt_denoise_params; for them sigma_color is the LUMINANCE sigma in standard deviations of the pixel mean
 * and must be positive and finite.  moments: W*H*2 f32 (pt_render_moments', row-major, unsharded), after accum.  samples >= 2,
 * otherwise PT_ERR_INVALID; every other argument rule, the scratch and the stage times are pt_denoise's.  Non-finite accumulator
 * or moment values are outside the contract. */
/* The defaults: the best of the grid tools/measure_denoise_var_gain.py searched (tests/golden/denoise_var_gain.json), FILMIC. */
#define PT_DENOISE_VAR_DEFAULT_ITERATIONS 1
#define PT_DENOISE_VAR_DEFAULT_FLAGS PT_DENOISE_NO_DEMODULATE
#define PT_DENOISE_VAR_DEFAULT_NORMAL_POWER_LOG2 3
#define PT_DENOISE_VAR_DEFAULT_SIGMA_COLOR 4.0f
#define PT_DENOISE_VAR_DEFAULT_SIGMA_DEPTH 4.0f
void pt_denoise_var_params_default(pt_denoise_params* params);
uint64_t pt_denoise_var_scratch_bytes(uint32_t width, uint32_t height);
int pt_denoise_var(int device, uint32_t width, uint32_t height, uint32_t samples, const pt_denoise_params* params,
                   const float* accum, const float* moments, const float* guides, float* out_color, uint8_t* out_rgb8);
int pt_denoise_var_device(int device, uint32_t width, uint32_t height, uint32_t samples, const pt_denoise_params* params,
                          const void* d_accum, const void* d_moments, const void* d_guides, void* d_out_color,
                          void* d_out_rgb8, void* d_scratch, void* hip_stream);
/* pt_render_moments + guides + pt_denoise_var without leaving the device, like pt_render_denoised (same outputs, the preview
 * callback receives the RAW frames, shard_count > 1 is PT_ERR_UNSUPPORTED). */
int pt_render_denoised_var(const pt_scene* scene, const pt_profile* profile, const pt_opts* opts,
                           const pt_denoise_params* params, uint8_t* rgb8, float* color);
/* Measurement, as pt_denoise_stage_times: ms[0] = prep, ms[1 + i] = pass i, ms[9] = finish. */
int pt_denoise_var_stage_times(int device, uint32_t width, uint32_t height, uint32_t samples, const pt_denoise_params* params,
                               const void* d_accum, const void* d_moments, const void* d_guides, void* d_out_color,
                               void* d_out_rgb8, void* d_scratch, float* ms);

/* ------------------------------------------------------------------ */
/* light mixer (no reference counterpart)                   */
/* ------------------------------------------------------------------ */

/* A frame is linear in every light's colour: lights are not sampled stochastically, Russian roulette and the throughput
 * cut-off look at the BRDF throughput only, and the tone map comes after the accumulation.  So, per channel,
 *     accum(colours) = E + sum_l colour_l * T_l
 * with E the frame with every light black and T_l the transport of light l at unit colour.  A pt_lightmix holds these
 * n_lights + 1 planes for ONE (view, geometry, materials, light kinds / positions, profile, opts); every colour, intensity,
 * mute or solo edit of that view is then one streaming kernel instead of a render.
 *
 * pt_lightmix_capture renders the n_lights + 1 accumulators of (profile, opts) with the scene's own frames (any flags, any
 * sharding; the planes are in the packed local order of pt_render; the progress and preview callbacks are not invoked):
 *   plane 0      E: every light's colour (0,0,0), kind, position and size kept
 *   unit[l]      m_l = the largest channel of light l's current colour, or 1.0f if that is 0
 *   plane 1 + l  D_l = F_l - E, one f32 subtraction per float; F_l = the frame with light l at (m_l, m_l, m_l), the others black
 * (the basis is taken at the light's own magnitude: a unit-white basis of a light of colour 1000 would amplify E's rounding
 * by that factor).  During the call the scene's lights change COLOUR only - the state change of pt_scene_set_lights (the
 * device is synchronised, no frame plan carries over) without its grid rebuild, and the position-keyed visibility planes are
 * kept; the caller must not use the scene from another thread meanwhile.  Afterwards - and after any failure, in which case
 * no object is returned - the scene has its original lights and renders the bits it rendered before.  More than
 * PT_LIGHTMIX_MAX_LIGHTS lights: PT_ERR_UNSUPPORTED; a null pointer, samples == 0, a rank without pixels or a light colour
 * that is not finite: PT_ERR_INVALID; both before any device work.
 * The object owns its planes (device memory on the scene's device) and outlives the scene.  It does not watch the scene: after
 * any edit other than light colours the caller captures again.
 *
 * pt_lightmix_create_from_planes makes the object from host planes ((n_lights + 1) x n_local x 3 f32, plane 0 = E, then D_l)
 * and units (finite, not 0) - for tests and for planes kept on disk.  device: HIP ordinal, -1 = current.
 *
 * pt_lightmix_apply: all f32, one IEEE operation per step in the order written, uncontracted (tests/lightmix_model.py
 * restates it bit for bit):
 *   host       f[l][ch] = colors[l][ch] / unit[l]
 *   per float k of a plane, ch = k mod 3:   a = E[k];  for l = 0 .. n_lights-1 in order:  a = a + f[l][ch] * D_l[k]
 *   accum[k] = a          (n_local x 3 f32: what pt_render's accum is for the edited lights, within rounding)
 *   rgb8[k]  = as_u8(pow(tonemap(a / (float)samples), 1/2.2) * 255), pt_render's post-processing of a
 * With 0 lights a = E[k].  A null object, null colors (with n_lights > 0), a colors entry that is not finite, an unknown tone
 * map, or rgb8 and accum both null: PT_ERR_INVALID before any device work.  The host form blocks; the device form is
 * asynchronous on hip_stream, allocates nothing, and wants d_rgb8 4-byte and d_accum 16-byte aligned (PT_ERR_INVALID otherwise);
 * colors is a HOST pointer in both (the factors travel in the kernel arguments).
 * pt_lightmix_basis copies plane `plane` (0 .. n_lights) to the host. */
enum { PT_LIGHTMIX_MAX_LIGHTS = 16 };
typedef struct pt_lightmix pt_lightmix;
typedef struct pt_lightmix_info {
    uint32_t n_lights, samples;
    uint64_t n_local;                       /* pixels, packed local order of (profile, opts) */
    uint64_t device_bytes;
    float unit[PT_LIGHTMIX_MAX_LIGHTS];     /* m_l */
} pt_lightmix_info;

int  pt_lightmix_capture(const pt_scene* scene, const pt_profile* profile, const pt_opts* opts, pt_lightmix** out);
int  pt_lightmix_create_from_planes(int device, uint32_t n_lights, uint32_t samples, uint64_t n_local,
                                    const float* unit, const float* planes /* host, (n_lights+1) x n_local x 3 */,
                                    pt_lightmix** out);
void pt_lightmix_destroy(pt_lightmix* mix);
int  pt_lightmix_get_info(const pt_lightmix* mix, pt_lightmix_info* info);
int  pt_lightmix_basis(const pt_lightmix* mix, uint32_t plane, float* host /* n_local x 3 */);
int  pt_lightmix_apply(const pt_lightmix* mix, const float* colors /* host, n_lights x 3 */, int tonemap,
                       uint8_t* rgb8, float* accum);                       /* host, either may be NULL */
int  pt_lightmix_apply_device(const pt_lightmix* mix, const float* colors /* host */, int tonemap,
                              void* d_rgb8, void* d_accum, void* hip_stream);   /* asynchronous, allocates nothing */

/* ------------------------------------------------------------------ */
/* progressive film (no reference counterpart)              */
/* ------------------------------------------------------------------ */

/* A film adds whole frames of ONE view (profile, opts) until the image is clean enough: it holds the sum of their accumulators
 * (n_local x 3 f32) and of their luminance moments (n_local x 2 f32, pt_render_moments), in the packed local order of pt_render
 * for (profile, opts), and makes a noise figure from the moments.  It is an add-on like the denoiser and the light mixer:
 * every pass is an ordinary frame with the moments tap, exactly what pt_render_moments_device launches.
 *
 * What a pass is.  The seed of sample s of global pixel i in a frame of `samples` samples is s + i * samples
 * (renderer/mod.rs:110-112), so two frames of the same `samples` are the same frame.  A pass is therefore a whole frame whose
 * `samples` is AT LEAST TWICE the pass's before it.  Pixel i of a pass of a samples uses the seeds [i*a, i*a + a); for passes a
 * and b >= 2a the ranges of one pixel overlap only for i < a / (b - a) <= 1:
 *   - global pixel 0 is the only pixel that ever sees a seed twice (the first a samples of its larger pass repeat the smaller
 *     pass).  Its mean stays unbiased; only its variance estimate is slightly off.
 *   - seeds ARE shared between different pixels of different passes (pixel j of pass b and pixel ~ j*b/a of pass a).  That
 *     correlates the noise of two distant pixels and biases nothing.
 * No sample is rendered twice, so the doubling costs nothing.  Every pass is the first frame of its configuration (a new
 * `samples`): unplanned, no frame cache is keyed - the situation of a camera path.  (A WINDOWED film - pt_film_create_windowed,
 * further down - has neither caveat and no doubling rule: its passes are windows of one enumeration.)
 *
 * pt_film_create copies profile (its samples is ignored) and opts (the progress and preview callbacks are dropped) and allocates
 * on `device` (HIP ordinal, -1 = current): the film's accum and moments, pass buffers of the same size, one err plane (n_local
 * f32) and the block arrays.  PT_FLAG_MEGAKERNEL (no staged samples): PT_ERR_UNSUPPORTED; a null pointer, a rank without pixels
 * or an option pt_render refuses: PT_ERR_INVALID.  pt_film_create_from_planes makes a film from host planes (accum n_local x 3,
 * moments n_local x 2; samples = their total, 1 .. PT_FILM_MAX_SAMPLES; last_pass_samples in 1 .. samples; n_local in
 * 1 .. 2^31 - 1) - for tests and for planes kept on disk.  Such a film counts one pass and has no profile (info: width =
 * height = 0): pt_film_add_pass and pt_film_render_until on it are PT_ERR_INVALID.
 * pt_film_reset: back to zero passes and zero planes, the allocations stay.  pt_film_read: host copies, either pointer may be
 * NULL.  pt_film_planes_device: the device planes (256-byte aligned), for pt_denoise_device / pt_denoise_var_device with
 * samples = info.samples (unsharded films; the planes are the film's, valid until pt_film_destroy, and change with every pass).
 *
 * pt_film_add_pass renders the frame (profile with `samples`, opts) of `scene` into the pass buffers, waits for it and only
 * then merges, per float of accum and of moments alike:   film = film + pass   (one f32 addition; a film of one pass holds that
 * frame's bits).  PT_ERR_INVALID before any device work: a null pointer, a film without a profile, samples < 1,
 * samples < 2 * last_pass_samples when a pass exists, a total above PT_FILM_MAX_SAMPLES, a scene on another device than the
 * film's.  Any failure before the merge leaves the film's planes and counters as they were.  The film does not watch the scene:
 * edits between passes are the caller's business, as with pt_lightmix.  The call blocks.
 * pt_film_add_planes merges a pass that was rendered elsewhere or earlier (host planes of pt_render_moments for the film's
 * view: accum n_local x 3, moments n_local x 2, `samples` theirs) with the same kernel, under the same rules for `samples`; it
 * works on every film.
 *
 * pt_film_noise: all f32, one IEEE operation per step in this order, uncontracted, IEEE divide and sqrt
 * (tests/film_model.py restates it bit for bit); n = the film's total samples, (m1, m2) = the film's moments of the pixel:
 *   per pixel p   N = (float)n;  mu = m1 / N;  e2 = m2 / N;  s2 = max(0, e2 - mu*mu);  vL = s2 / (float)(n - 1);
 *                 se = sqrt(vL);  den = max(mu, lum_floor);  err = se / den
 *                 (the standard error of the pixel's mean luminance relative to that mean; a pixel darker than lum_floor is
 *                 judged as if it had that brightness)
 *   per block b   the packed pixels [256 b, 256 b + 256):  v[i] = err of pixel 256 b + i, or 0.f beyond n_local;
 *                 for stride = 128, 64, 32, 16, 8, 4, 2, 1:  for i < stride:  v[i] = v[i] + v[i + stride]
 *                 block_sum[b] = v[0];  block_max[b] = the largest err of the block's pixels
 *   on the host, in f64, b ascending:   S = S + (double)block_sum[b];   mean_b = (double)block_sum[b] / pixels_in_block(b)
 *                 mean_error = S / n_local;  max_block_error = the largest mean_b;  fraction_over = (blocks with
 *                 mean_b > target) / n_blocks;  converged = mean_error <= target
 * err_host (n_local f32), block_sum_host and block_max_host (n_blocks f32 each, n_blocks = ceil(n_local / 256)) may be NULL.
 * PT_ERR_INVALID: a null film or out, a total n < 2, lum_floor not positive and finite, target negative or not finite.
 * Non-finite planes are outside the contract.  PT_FILM_MAX_SAMPLES keeps (float)n exact.
 *
 * pt_film_resolve: color = accum / (float)n per float [n_local x 3 f32]; rgb8 = pt_render's post-processing of accum with
 * samples = n [n_local x 3].  Either output may be NULL, not both (PT_ERR_INVALID, as n = 0 and an unknown tone map).  The host
 * form blocks; the device form is asynchronous on hip_stream and allocates nothing.
 *
 * pt_film_render_until adds passes until the noise target is met: the next pass has first_pass_samples on an empty film and
 * 2 * last_pass_samples otherwise.  It adds the pass, computes the noise (lum_floor, target), calls on_pass(info, noise, user) if
 * set, and goes on; it stops when the noise has converged or when the total plus the next pass would exceed max_samples (or
 * PT_FILM_MAX_SAMPLES).  out = the last noise; out->converged tells why it stopped.  A film that can take no pass at all gets
 * the noise of what it holds.  PT_ERR_INVALID before any device work: what pt_film_add_pass and pt_film_noise refuse,
 * first_pass_samples < 2, an empty film with first_pass_samples > max_samples. */
typedef struct pt_film pt_film;
typedef struct pt_film_info {
    uint32_t width, height, passes, last_pass_samples;
    uint64_t n_local, samples /* total */, device_bytes;
} pt_film_info;
typedef struct pt_film_noise_stats {
    double mean_error;        /* sum of the block sums / n_local                                   */
    double max_block_error;   /* largest block_sum[b] / pixels_in_block(b)                         */
    double fraction_over;     /* share of blocks whose mean error exceeds target                   */
    uint64_t samples;         /* total samples the figures are for                                 */
    uint32_t n_blocks, converged /* mean_error <= target */;
} pt_film_noise_stats;
enum { PT_FILM_MAX_SAMPLES = 1u << 24 };   /* (float)n stays exact */
#define PT_FILM_DEFAULT_LUM_FLOOR 0.01f
typedef void (*pt_film_pass_fn)(const pt_film_info* info, const pt_film_noise_stats* noise, void* user);

int  pt_film_create(int device, const pt_profile* profile, const pt_opts* opts, pt_film** out);
int  pt_film_create_from_planes(int device, uint64_t n_local, uint64_t samples, uint32_t last_pass_samples,
                                const float* accum /* host */, const float* moments /* host */, pt_film** out);
void pt_film_destroy(pt_film* film);
int  pt_film_reset(pt_film* film);
int  pt_film_get_info(const pt_film* film, pt_film_info* info);
int  pt_film_read(const pt_film* film, float* accum, float* moments);                  /* host, either may be NULL */
int  pt_film_planes_device(const pt_film* film, void** d_accum, void** d_moments);
int  pt_film_add_pass(pt_film* film, const pt_scene* scene, uint32_t samples);
int  pt_film_add_planes(pt_film* film, uint32_t samples, const float* accum /* host */, const float* moments /* host */);
int  pt_film_noise(const pt_film* film, float lum_floor, double target, pt_film_noise_stats* out, float* err_host,
                   float* block_sum_host, float* block_max_host);
int  pt_film_resolve(const pt_film* film, int tonemap, uint8_t* rgb8, float* color);   /* host */
int  pt_film_resolve_device(const pt_film* film, int tonemap, void* d_rgb8, void* d_color, void* hip_stream);
int  pt_film_render_until(pt_film* film, const pt_scene* scene, uint32_t first_pass_samples, uint64_t max_samples,
                          float lum_floor, double target, pt_film_pass_fn on_pass, void* user, pt_film_noise_stats* out);
/* Measurement: the two kernels between HIP events on the null stream, `reps` times each (blocks): ms_merge[r] = k_film_merge
 * adding the film's planes to its PASS buffers (scratch between passes; the film is unchanged), ms_noise[r] = k_film_noise
 * (lum_floor, with the err plane written when with_err is not 0).  The film's total must be >= 2. */
int  pt_film_kernel_times(const pt_film* film, float lum_floor, int with_err, uint32_t reps, float* ms_merge, float* ms_noise);

/* ------------------------------------------------------------------ */
/* tile-list frames and the adaptive film                  */
/* ------------------------------------------------------------------ */

/* A tile-list frame renders the listed tiles of the frame (profile, opts) and nothing else - a region re-render, and what an
 * adaptive film's later passes are made of.
 *   tiles     n_tiles global tile numbers ty * tiles_x + tx of the tiling opts.tile_w x opts.tile_h (0: 32; the rules of
 *             pt_opts), tiles_x = ceil(width / tile_w); STRICTLY ASCENDING.
 *   outputs   packed: the tiles one after the other in list order, each row-major and clipped to the image - the packed order
 *             of a shard.  pt_tiles_pixel_count gives the number of packed pixels (0 for a list or options that are refused),
 *             pt_tiles_pixel_map (a host helper, no GPU) the global index x + y * width of every packed pixel.
 *             rgb8 [n x 3 u8], accum [n x 3 f32], moments [n x 2 f32]; each may be NULL, not all of them.
 *   contract  every packed pixel's accum, moments and rgb8 equal, bit for bit, those of the same global pixel in
 *             pt_render_moments(scene, profile, opts) of the whole frame: the seed of a sample depends on the GLOBAL pixel index
 *             and profile.samples only.  This holds for the default pipeline and for PT_FLAG_NO_GRIDS; with PT_FLAG_MEGAKERNEL for
 *             accum and rgb8 (moments != NULL there: PT_ERR_UNSUPPORTED, as in pt_render_moments).
 *   refusals  PT_ERR_INVALID before any device work, the outputs untouched: a null list or n_tiles == 0, a list that is not
 *             strictly ascending, a tile number >= tiles_x * tiles_y, shard_count > 1, anything pt_render refuses.
 * The host form blocks.  The device form copies the list before it returns and is asynchronous on hip_stream after that - but,
 * UNLIKE pt_render_device, it may wait for the whole device and allocate when it is entered (the list's table is rewritten in
 * place).  A tile-list frame leaves the scene's steady state alone: it is a first frame every time (unplanned, no frame cache
 * read, written, keyed or counted), and the whole frames before and after it run what they would have run without it. */
uint64_t pt_tiles_pixel_count(const pt_profile* profile, const pt_opts* opts, const uint32_t* tiles, uint32_t n_tiles);
int  pt_tiles_pixel_map(const pt_profile* profile, const pt_opts* opts, const uint32_t* tiles, uint32_t n_tiles, uint32_t* out);
int  pt_render_tiles(const pt_scene* scene, const pt_profile* profile, const pt_opts* opts, const uint32_t* tiles, uint32_t n_tiles,
                     uint8_t* rgb8, float* accum, float* moments);   /* host */
int  pt_render_tiles_device(const pt_scene* scene, const pt_profile* profile, const pt_opts* opts, const uint32_t* tiles,
                            uint32_t n_tiles, void* d_rgb8, void* d_accum, void* d_moments, void* hip_stream);

/* The adaptive film.  A film that has a profile and shard_count <= 1 may take TILE PASSES: a pass of `samples` samples over a
 * list of tiles of the film's own tiling (its opts' tile size).  The first tile pass allocates a count plane - n_local u32,
 * 256-byte aligned, filled with the film's uniform total - and the film is NON-UNIFORM from then on, until pt_film_reset.  A film
 * that never takes a tile pass allocates nothing new, and every call above runs on it what it ran before.
 *
 * The rule for `samples` is the film's: at least twice the last pass's (whole or tile), info.samples + samples at most
 * PT_FILM_MAX_SAMPLES - pixel i of a pass of a samples uses the seeds [i*a, i*a + a) whether or not its neighbours are rendered.
 * info.samples of a non-uniform film is the LARGEST count (what a pixel has if it took every pass).
 *
 * pt_film_add_tile_pass renders the tile-list frame (pt_render_tiles_device) into the pass buffers, waits for it and only then
 * merges: per pixel of the listed tiles   film = film + pass   on the 3 + 2 floats (one f32 addition each), count += samples.
 * No other pixel is read or written.  A failure before the merge leaves the film as it was.  pt_film_add_tile_planes merges a
 * pass rendered elsewhere (host planes in the packed order of pt_render_tiles for the list).  PT_ERR_INVALID before any device
 * work: what pt_film_add_pass and pt_render_tiles refuse, a film without a profile, a sharded film.
 * pt_film_read_counts: every pixel's count (a uniform film: its total everywhere).
 *
 * On a non-uniform film: pt_film_add_pass adds a whole frame - the tile pass that lists every tile; pt_film_read is unchanged;
 * pt_film_reset makes the film uniform (and empty) again; pt_film_resolve / _device give color = accum / (float)count[p] and
 * rgb8 = pt_render's post-processing with samples = count[p] (PT_ERR_INVALID while some tile holds no samples);
 * pt_film_noise, pt_film_add_planes, pt_film_planes_device (and pt_film_render_until, pt_film_kernel_times, which are made of
 * them) are PT_ERR_UNSUPPORTED and change nothing: their contracts assume one n.
 *
 * pt_film_tile_noise (uniform films too; the film needs a profile): all f32, one IEEE operation per step in this order,
 * uncontracted, IEEE divide and sqrt (tests/film_adaptive_model.py restates it bit for bit):
 *   per pixel p   pt_film_noise's err with n = count[p] (the uniform total on a uniform film)
 *   per tile t    of clipped size cw x ch, its pixels numbered j = y * cw + x, P = cw * ch:
 *                 for i in 0 .. 255:  v[i] = 0.f;  for j = i; j < P; j += 256:  v[i] = v[i] + err_j
 *                 for stride = 128, 64, 32, 16, 8, 4, 2, 1:  for i < stride:  v[i] = v[i] + v[i + stride]
 *                 tile_sum[t] = v[0];  tile_max[t]: the same steps with max in place of + (the largest err of the tile)
 *                 (a full 16 x 16 tile: pt_film_noise's block, addition for addition)
 *   on the host, in f64, t ascending:   mean_t = (double)tile_sum[t] / P;  mean_error = (sum of (double)tile_sum[t]) / n_local;
 *                 max_tile_error = the largest mean_t;  over_tiles = tiles with mean_t > target;  converged = no such tile;
 *                 samples = the largest count;  pixel_samples = the sum of every pixel's count
 * err_host (n_local f32, image order), tile_sum_host and tile_max_host (n_tiles f32 each) may be NULL.  The tile arrays are
 * allocated on first use.  PT_ERR_INVALID: what pt_film_noise refuses, a pixel with fewer than 2 samples, no profile, shards.
 *
 * pt_film_render_until_adaptive.  Loop: (1) the next pass has first_pass_samples (>= 2) on an empty film, 2 * last_pass_samples
 * otherwise; (2) stop for budget if info.samples + that would exceed max_samples (or PT_FILM_MAX_SAMPLES); (3) render the pass
 * over the active set - EVERY tile while the film is empty or info.samples < uniform_samples; a pass over every tile is
 * pt_film_add_pass, so the film stays uniform for as long as that holds; (4) pt_film_tile_noise(lum_floor, target); (5) the
 * candidates are the tiles with mean_t > target; (6) the next active set is the candidates, with dilate = 1 grown by their 8
 * neighbours; (7) on_pass(info, noise, user) if set - noise.mean_error and .max_block_error are the tile figures, .fraction_over
 * = over_tiles / n_tiles, .n_blocks = n_tiles, .converged = no candidate; (8) stop as converged when there is no candidate.
 * out = the last tile statistics, out->active_tiles the tiles of the pass just rendered.  The selection is a pure function of the
 * film's current planes: a tile that was dropped comes back only through dilation.  A film that already has passes (and
 * info.samples >= uniform_samples) starts with step 4.  max_samples bounds the largest per-pixel count.
 * uniform_samples (default 24) and dilate (default 1) are design choices, not measured optima: the variance of a few samples
 * underestimates the error, and a hard tile edge in the sample density can show in the image. */
typedef struct pt_film_tile_stats {
    double mean_error;        /* sum of the tile sums / n_local                                    */
    double max_tile_error;    /* largest tile_sum[t] / pixels of tile t                            */
    uint64_t samples;         /* the largest per-pixel count                                       */
    uint64_t pixel_samples;   /* the sum of every pixel's count                                    */
    uint32_t n_tiles, over_tiles /* mean_t > target */, active_tiles /* pt_film_render_until_adaptive: of the last pass */,
             converged /* over_tiles == 0 */;
} pt_film_tile_stats;
typedef struct pt_film_adaptive_info {
    uint32_t uniform /* 1: no tile pass since the film was made or reset */, tile_w, tile_h, tiles_x, tiles_y, n_tiles, tile_passes,
             last_pass_tiles /* tiles of the last pass (n_tiles: a whole frame; 0: no pass yet) */;
    uint64_t min_samples, max_samples /* the smallest and the largest per-pixel count */, pixel_samples, device_bytes;
} pt_film_adaptive_info;
typedef struct pt_film_adaptive_params {
    double target;
    uint64_t max_samples;
    float lum_floor;
    uint32_t first_pass_samples, uniform_samples, dilate /* 0 or 1 */;
} pt_film_adaptive_params;
void pt_film_adaptive_params_default(pt_film_adaptive_params* params);   /* floor 0.01, target 0.02, first 8, uniform 24, dilate 1, max 512 */
int  pt_film_add_tile_pass(pt_film* film, const pt_scene* scene, uint32_t samples, const uint32_t* tiles, uint32_t n_tiles);
int  pt_film_add_tile_planes(pt_film* film, uint32_t samples, const uint32_t* tiles, uint32_t n_tiles,
                             const float* accum /* host, packed */, const float* moments /* host, packed */);
int  pt_film_read_counts(const pt_film* film, uint32_t* counts /* host, n_local */);
int  pt_film_tile_noise(const pt_film* film, float lum_floor, double target, pt_film_tile_stats* out, float* err_host,
                        float* tile_sum_host, float* tile_max_host);
int  pt_film_get_adaptive_info(const pt_film* film, pt_film_adaptive_info* out);
int  pt_film_render_until_adaptive(pt_film* film, const pt_scene* scene, const pt_film_adaptive_params* params,
                                   pt_film_pass_fn on_pass, void* user, pt_film_tile_stats* out);
/* Measurement, like pt_film_kernel_times, on a non-uniform film whose every pixel has >= 2 samples: ms_merge[r] =
 * k_film_merge_tiles over every tile with a pass of zeros and zero samples (the pass buffers are scratch; the film's planes and
 * counts keep their values), ms_noise[r] = k_film_tile_noise with the err plane, ms_resolve[r] = the u8 resolve with counts. */
int  pt_film_adaptive_kernel_times(pt_film* film, float lum_floor, int tonemap, uint32_t reps, float* ms_merge, float* ms_noise,
                                   float* ms_resolve);

/* ------------------------------------------------------------------ */
/* film filter                                             */
/* ------------------------------------------------------------------ */

/* The a-trous filters on a film's own device planes, uniform or not, and the error figure of the filtered mean.  The film needs a
 * profile and shard_count <= 1 (its planes are then in image order, width x height).  variance = 0 is pt_denoise's filter,
 * variance = 1 pt_denoise_var's; params are theirs, with their rules.  guides: the planes of pt_render_guides for the film's view.
 *
 *   prep     exactly pt_denoise's / pt_denoise_var's prep with the pixel's own count for `samples`: N = (float)count[p], and the
 *            divisor of the sample variance is (float)(count[p] - 1); count[p] is the film's total on a uniform film.
 *   passes   theirs, unchanged.
 *   finish   theirs: color [n_local x 3 f32] the filtered mean radiance, rgb8 its tone-mapped form (params->tonemap).
 *   ferr     [n_local f32], variance = 1 only (variance = 0 with ferr != NULL: PT_ERR_INVALID).  All f32, one IEEE operation per
 *            step in this order, uncontracted, IEEE divide and sqrt (tests/film_denoise_model.py restates it bit for bit):
 *              a filtered pixel (depth >= 0, iterations > 0):   vf = v of the last pass (v = vacc / (wsum * wsum));
 *                  if demodulating:  ld = lum(d);  vf = vf * (ld * ld);
 *                  se = sqrt(vf);  den = max(lum(out), lum_floor);  ferr = se / den       (out: the pixel's color)
 *              any other pixel (depth < 0, or iterations = 0):  pt_film_noise's err with n = count[p].
 *   iterations = 0: color and rgb8 are pt_film_resolve's (params->tonemap), on any film.
 *   On a uniform film color and rgb8 equal, bit for bit, pt_denoise_device / pt_denoise_var_device on pt_film_planes_device with
 *   samples = info.samples.
 *
 * WHAT ferr IS NOT.  It is the standard error the filter's own weights would give the filtered mean if the taps were
 * independent and the filter unbiased.  It ignores the filter's bias (blur across detail the guides do not see), and it
 * ignores the correlation between neighbouring filtered pixels (after the first pass the taps share samples; v is propagated
 * as if they did not, as in SVGF).  It is a stopping heuristic, not an error bound.
 *
 * PT_ERR_INVALID before any device work, the outputs untouched: a null film, params, guides / scene, or no output at all; a
 * null scratch with iterations > 0; a film without a profile; a sharded film; a pixel with no samples; variance = 1 with a pixel
 * below 2 samples; a scene on another device than the film's; what pt_denoise / pt_denoise_var refuse in params; a lum_floor
 * that is not positive and finite; variance other than 0 or 1.
 *
 * pt_film_denoise_device takes the caller's scratch (pt_film_denoise_scratch_bytes, 256-byte aligned: the filter's planes, a
 * ferr plane and two tile arrays; 0 for a film that is refused), allocates nothing and is asynchronous on hip_stream; each of
 * d_out_color, d_out_rgb8, d_out_ferr may be NULL, not all.  The host forms render the guides from `scene` and block; their
 * scratch (the same bytes and a plane of guides) is allocated inside the film by the first such call, counted in
 * info.device_bytes from then on, kept by pt_film_reset and freed by pt_film_destroy.  A film that never calls them allocates
 * nothing new.
 *
 * pt_film_tile_reduce_device (a test and measurement hook: the reduction pt_film_filtered_noise runs, on a plane of the caller's):
 * pt_film_tile_noise's "per tile t" steps, word for word, over an error plane d_err [n_local f32,
 * image order] that exists already, into d_tile_sum and d_tile_max [n_tiles f32 each]; asynchronous on hip_stream.
 *
 * pt_film_filtered_noise: the guides of `scene`, the variance filter, ferr, the tile reduction over ferr, then the host f64 step
 * of pt_film_tile_noise (mean_t, mean_error, max_tile_error, over_tiles, converged, samples, pixel_samples).  ferr_host,
 * tile_sum_host, tile_max_host may be NULL.  Refusals: pt_film_denoise's with variance = 1, and pt_film_tile_noise's target.
 *
 * pt_film_render_until_filtered is pt_film_render_until_adaptive's loop, step for step, with params->adaptive - except that step
 * (4) is pt_film_filtered_noise(params->filter, lum_floor, target): tiles are selected by the error of the FILTERED image.  The
 * guides are rendered once, when the function is entered (the film does not watch the scene).  The selection is a pure
 * function of the film's planes, the guides and the parameters - the guides stay in the film's scratch for the whole call, so
 * on_pass MUST NOT call pt_film_denoise, pt_film_filtered_noise or pt_film_denoise_kernel_times on this film (they render
 * their own guides into the same plane); the device form with the caller's scratch, pt_film_read, pt_film_read_counts and
 * pt_film_resolve are fine there.  Refusals, before any device work and before the scratch is made:
 * pt_film_render_until_adaptive's, pt_denoise_var's parameter rules, and - on a film that is measured as it stands (it has
 * uniform_samples already, or no pass fits the budget) - a pixel below 2 samples. */
typedef struct pt_film_filtered_params {
    pt_film_adaptive_params adaptive;
    pt_denoise_params filter;
} pt_film_filtered_params;
void pt_film_filtered_params_default(pt_film_filtered_params* params);   /* adaptive defaults + pt_denoise_var defaults */
uint64_t pt_film_denoise_scratch_bytes(const pt_film* film);
int  pt_film_denoise_device(const pt_film* film, int variance /* 0 plain, 1 variance-guided */, const pt_denoise_params* params,
                            float lum_floor, const void* d_guides, void* d_out_color, void* d_out_rgb8,
                            void* d_out_ferr /* variance only, may be NULL */, void* d_scratch, void* hip_stream);
int  pt_film_denoise(const pt_film* film, const pt_scene* scene /* guides are rendered from it */, int variance,
                     const pt_denoise_params* params, float lum_floor, uint8_t* rgb8, float* color, float* ferr);   /* host */
/* test / measurement hook */
int  pt_film_tile_reduce_device(const pt_film* film, const void* d_err, void* d_tile_sum, void* d_tile_max, void* hip_stream);
int  pt_film_filtered_noise(const pt_film* film, const pt_scene* scene, const pt_denoise_params* params, float lum_floor,
                            double target, pt_film_tile_stats* out, float* ferr_host, float* tile_sum_host, float* tile_max_host);
int  pt_film_render_until_filtered(pt_film* film, const pt_scene* scene, const pt_film_filtered_params* params,
                                   pt_film_pass_fn on_pass, void* user, pt_film_tile_stats* out);
/* Measurement, like the other *_times: the variance filter with ferr and the tile reduction on the null stream, HIP events
 * between the stages; blocks.  ms_prep[r], ms_passes[r] (all passes), ms_finish[r] (finish + ferr), ms_reduce[r], reps each. */
int  pt_film_denoise_kernel_times(const pt_film* film, const pt_scene* scene, const pt_denoise_params* params, float lum_floor,
                                  uint32_t reps, float* ms_prep, float* ms_passes, float* ms_finish, float* ms_reduce);

/* ------------------------------------------------------------------ */
/* window frames and windowed films                        */
/* ------------------------------------------------------------------ */

/* A window frame renders the samples [s0, s1) of the frame (profile, opts), 0 <= s0 < s1 <= N = profile.samples: sample s of
 * pixel i uses the seed of pt_render(samples = N), whatever the windows are.  accum (and moments, where given) are IN-OUT: with
 * s0 == 0 the sums start from zero and the buffers' contents are ignored; with s0 > 0 they hold the sums of [0, s0) and the call
 * continues them sample by sample with the additions pt_render / pt_render_moments perform.
 *   chaining   after any chain [0,a), [a,b), .., [y,N) on the same buffers accum, moments and rgb8 equal pt_render_moments(scene,
 *              profile, opts) bit for bit.
 *   prefixes   after a chain ending at k < N: accum is the in-order f32 running sum of the first k planes of pt_render_samples
 *              for the N-sample profile, moments their luminance moments, rgb8 pt_render's post-processing of accum with
 *              samples = k.
 *   layout     tiles == NULL: the whole frame (n_tiles is ignored) - pt_render's buffers, shards in packed local order.
 *              tiles != NULL: the rules, layout and refusals of pt_render_tiles; each packed pixel equals the same global pixel
 *              of the whole-frame window.
 *   pipelines  the default pipeline and PT_FLAG_NO_GRIDS: everything.  PT_FLAG_MEGAKERNEL: accum and rgb8 (its kernel carries
 *              its sums the same way); moments != NULL there is PT_ERR_UNSUPPORTED, as in pt_render_moments.
 *   refusals   PT_ERR_INVALID before any device work, the outputs untouched: s0 >= s1, s1 > N, a null accum, anything
 *              pt_render / pt_render_tiles refuses.
 * opts.sample_batch (and the staging budget) split a window into batches internally; that changes no bit.  The progress and
 * preview callbacks of opts see the absolute sample numbers.  The host form blocks.  The device form is asynchronous on
 * hip_stream but, like pt_render_tiles_device, may wait for the whole device and allocate when it is entered.
 * A window frame leaves the scene's steady state alone, exactly as a tile-list frame does: it is a first frame every time
 * (unplanned, no frame cache read, written, keyed or counted, the statistics slot of the tile-list frames), and the whole frames
 * before and after it run what they would have run without it.  Planned or cached windows are not built: a film renders every
 * sample once, and plans and caches pay only on the second rendering of the same items. */
int  pt_render_window(const pt_scene* scene, const pt_profile* profile, const pt_opts* opts, uint32_t s0, uint32_t s1,
                      const uint32_t* tiles /* NULL: the whole frame */, uint32_t n_tiles, uint8_t* rgb8, float* accum /* in-out */,
                      float* moments /* in-out, may be NULL */);   /* host */
int  pt_render_window_device(const pt_scene* scene, const pt_profile* profile, const pt_opts* opts, uint32_t s0, uint32_t s1,
                             const uint32_t* tiles, uint32_t n_tiles, void* d_rgb8, void* d_accum, void* d_moments, void* hip_stream);

/* A windowed film: every pass is a window of ONE enumeration of N = profile.samples samples per pixel (2 .. PT_FILM_MAX_SAMPLES),
 * so a pixel at count c holds the sums of the samples [0, c) of pt_render(samples = N): pixel i uses only its own seeds
 * [i*N, i*N + N), a window may have any length, and a film that reaches N everywhere equals pt_render_moments(N) bit for bit.
 * Its planes mean what a film's planes mean (sums, moments, a count plane once it is non-uniform): pt_film_noise,
 * pt_film_tile_noise, pt_film_resolve[_device], pt_film_read, pt_film_read_counts, pt_film_planes_device,
 * pt_film_denoise[_device], pt_film_filtered_noise, pt_film_get_info / _adaptive_info and pt_film_reset work on it unchanged and
 * follow the same uniform / non-uniform rules.  Mixing is PT_ERR_INVALID and changes nothing: pt_film_add_pass,
 * pt_film_add_tile_pass, pt_film_add_planes, pt_film_add_tile_planes, pt_film_render_until, _adaptive and _filtered on a
 * windowed film; the calls below (but pt_film_get_window_info and pt_film_window_params_default) on a film that is not.
 *
 * pt_film_add_window: the window [n, n + samples) of every pixel, n = info.samples; PT_ERR_INVALID when n + samples > N (a film
 * at n == N is full).  The frame renders into the pass buffers, seeded with a copy of the film, and the film adopts them when
 * it has completed: a failure leaves the film's planes and counters as they were.  Sharded films work.  On a non-uniform film it
 * is the tile window that lists every tile.
 * pt_film_add_tile_window (unsharded films): every listed tile t gets the window [count_t, count_t + samples) - counts are
 * uniform inside a tile; PT_ERR_INVALID when any listed tile would pass N, and what pt_render_tiles refuses in the list.  The
 * tiles are grouped by count, counts ascending; every group is gathered into a run of the pass buffers (k_film_gather_tiles),
 * rendered there as one tile-list window frame, and when EVERY group's frame has completed the runs are written back and
 * `samples` is added to the counts (k_film_scatter_tiles).  No pixel outside the list is read or written; a failure before the
 * first write-back leaves the film as it was.  The first tile window makes the film non-uniform, as the first tile pass does.
 *
 * pt_film_render_until_windowed (unsharded films).  Loop: (1) the active tiles that are full (count == N) take no more; the
 * next window has window_samples samples, clipped to N - the largest count among the rest; (2) stop for budget when none is
 * left; (3) render the window over the active set - EVERY tile while the film is empty, while adaptive == 0 or while
 * info.samples < uniform_samples; a window over every tile of a uniform film is pt_film_add_window; (4) pt_film_tile_noise;
 * (5) - (7) the candidates, their dilation and on_pass as in pt_film_render_until_adaptive; (8) stop as converged when there is
 * no candidate.  A film that has windows (every pixel >= 2 samples; adaptive: info.samples >= uniform_samples) starts with
 * step 4.  A loop that runs out of budget with every tile active leaves the film equal to pt_render_moments(N), bit for bit.
 * PT_ERR_INVALID before any device work: what pt_film_tile_noise refuses in lum_floor and target, window_samples < 1 (< 2 on an
 * empty film: a sample variance needs two), dilate or adaptive above 1, a film that is not windowed, a sharded film, a scene on
 * another device.  window_samples (default PT_FILM_DEFAULT_WINDOW_SAMPLES) is a design choice, not a measured optimum
 * (DESIGN 4k): a short window stops closer to the target and pays a frame's fixed cost more often. */
#define PT_FILM_DEFAULT_WINDOW_SAMPLES 32u
typedef struct pt_film_window_info {
    uint32_t windowed /* 0 / 1 */, enumeration /* N; 0: not windowed */, windows /* whole-frame windows since the film was made
             or reset */, tile_windows;
} pt_film_window_info;
typedef struct pt_film_window_params {
    double target;
    float lum_floor;
    uint32_t window_samples, adaptive /* 0: every window covers every tile; 1: the tiles above the target */, uniform_samples,
             dilate /* 0 or 1 */;
} pt_film_window_params;
int  pt_film_create_windowed(int device, const pt_profile* profile /* samples = N */, const pt_opts* opts, pt_film** out);
int  pt_film_add_window(pt_film* film, const pt_scene* scene, uint32_t samples);
int  pt_film_add_tile_window(pt_film* film, const pt_scene* scene, uint32_t samples, const uint32_t* tiles, uint32_t n_tiles);
int  pt_film_get_window_info(const pt_film* film, pt_film_window_info* out);
void pt_film_window_params_default(pt_film_window_params* params);   /* floor 0.01, target 0.02, window 32, adaptive 1, uniform 24, dilate 1 */
int  pt_film_render_until_windowed(pt_film* film, const pt_scene* scene, const pt_film_window_params* params,
                                   pt_film_pass_fn on_pass, void* user, pt_film_tile_stats* out);
/* Measurement, like the other *_times, on a non-uniform film: ms_gather[r] = k_film_gather_tiles over every tile into the pass
 * buffers (scratch between passes), ms_scatter[r] = k_film_scatter_tiles writing the same values back with zero samples (the
 * film's planes and counts keep their values). */
int  pt_film_window_kernel_times(pt_film* film, uint32_t reps, float* ms_gather, float* ms_scatter);

/* ------------------------------------------------------------------ */
/* sharded films                                           */
/* ------------------------------------------------------------------ */

/* A SHARD FILM is one rank's part of an adaptive or windowed film that opts->shard_count ranks hold together.  A film's tiling
 * is its opts' tile size, which is the sharding's tile size too, so every tile of the film belongs whole to one rank - rank
 * (tx + ty * s) % shard_count, the rule of pt_opts.  pt_film_create_shard makes the part of rank opts->shard_rank; windowed = 1:
 * a windowed film of N = profile.samples (pt_film_create_windowed), 0: a film of doubling passes (pt_film_create); it refuses
 * what they refuse.  The planes are in the packed local order of pt_local_pixel_map (profile, opts): the rank's tiles in
 * ascending tile number, each row-major and clipped.  shard_count <= 1 is allowed: one rank holds every tile, in image order,
 * and everything below is its N = 1 case.  pt_film_get_shard_info works on every film.
 *
 * TILE LISTS ARE GLOBAL on a shard film: the rules of pt_render_tiles, tile numbers of the image, any rank's tiles.  The rank
 * renders and merges the listed tiles it holds and skips the others; host planes (pt_film_add_tile_planes) hold the rank's
 * listed tiles only, packed in list order.  A list with none of the rank's tiles still counts as the pass: passes,
 * last_pass_samples, tile_passes / tile_windows advance, and nothing is rendered or merged.  The film keeps the sample count of
 * EVERY tile of the image, updated from the lists, so info.samples, adaptive_info.min_samples / max_samples / pixel_samples /
 * n_tiles / tiles_x / tiles_y / last_pass_tiles are the whole film's on every rank; info.n_local and the planes are the rank's.
 *   work            pt_film_add_pass, pt_film_add_window (whole frames: the sharded frame of pt_render, the film stays uniform),
 *                   pt_film_add_tile_pass, pt_film_add_tile_planes, pt_film_add_tile_window (the rank's listed tiles, grouped by
 *                   count), pt_film_add_planes, pt_film_read, pt_film_read_counts, pt_film_resolve[_device], pt_film_reset, the
 *                   info calls, pt_film_adaptive_kernel_times and pt_film_window_kernel_times (the packed kernels over the rank's
 *                   tiles).  A tile pass renders the rank's listed tiles as an UNSHARDED tile-list frame: its buffers come in
 *                   list order, which is the film's own order for those tiles.
 *   PT_ERR_INVALID  and nothing changes - their figures are defined over one device's planes: pt_film_tile_noise,
 *                   pt_film_render_until, _adaptive, _windowed and _filtered, pt_film_denoise[_device],
 *                   pt_film_denoise_kernel_times, pt_film_tile_reduce_device, pt_film_filtered_noise
 *                   (pt_film_denoise_scratch_bytes: 0).
 * The calls below marked (shard) are PT_ERR_INVALID on a film that is not a shard film.  Films of pt_film_create[_windowed] with
 * shard_count > 1 are what they were: whole passes only.
 *
 * pt_film_shard_tile_noise (shard): pt_film_tile_noise's per-pixel and per-tile steps on the rank's tiles - a tile's sum and
 * maximum are made from that tile's pixels only, addition for addition the steps of pt_film_tile_noise, so they do not depend on
 * who holds the tile.  tile_sum and tile_max hold one entry per tile of the IMAGE; the entries of other ranks' tiles are +0.f.
 * err_host (n_local f32, packed local order) may be NULL.  Refusals: pt_film_tile_noise's; "every pixel >= 2 samples" is checked
 * over all tiles of the image.
 * pt_film_tile_stats_from_sums (any film with a profile): the host f64 step of pt_film_tile_noise over a COMPLETE tile_sum array
 * (n_tiles entries), n_local = width * height, the counts the film's.  On the sums of an unsharded film it equals that film's
 * pt_film_tile_noise statistics field for field.
 * pt_film_select_tiles (any film with a profile; no device work): steps 5 - 6 of the adaptive loops - the tiles with
 * mean_t > target and, dilate = 1, their 8 neighbours, ascending, into tiles (room for n_tiles entries); *n_out their number.
 *
 * The exchange.  pt_film_exchange_fn is a blocking collective the host supplies: in, this rank's arrays; out, the element-wise
 * combination over all ranks.  Unowned entries are +0.f and errors are not negative, so an element-wise sum, an element-wise
 * maximum and "take the owner's" all give the same bits.  Every rank calls it once per measurement, in the same order.
 * pt_film_exchange_comm (user: a pt_comm*) is a ready-made one over the library's communicator: one ncclAllGather of the two
 * arrays, then the largest of every entry.
 *
 * pt_film_render_until_adaptive_sharded / _windowed_sharded (shard) are pt_film_render_until_adaptive / _windowed step for step
 * - the same loop code - with step 4 = pt_film_shard_tile_noise, exchange, pt_film_tile_stats_from_sums.  Every decision is a
 * pure function of the complete arrays and of the counts of all tiles, so the ranks take the same passes over the same lists and
 * stop together without any other communication, and the shards, assembled, are the film the unsharded loop makes: accum,
 * moments and counts bit for bit, the same statistics, the same stop.  exchange == NULL: shard_count <= 1 only.  A non-zero
 * return of the exchange ends the loop with PT_ERR_DEVICE (the callback's code is in the message); the film keeps the passes
 * merged so far.  Refusals: those of the unsharded loops.
 *
 * pt_film_assemble: `whole` - an empty or reset unsharded film of the same profile, tile size and kind (pt_film_create or
 * pt_film_create_windowed with the same N) - receives the planes (and counts) of the n shard films of one sharded film in image
 * order (k_film_import_shard) and their counters; shards on other devices are staged through the host.  shards: every rank of
 * n == shard_count once, in any order, equal in every counter and in the tile counts.  Afterwards `whole` is an ordinary film
 * (uniform if the shards are): resolve, tile noise, the filter, further passes or windows.  Any mismatch is PT_ERR_INVALID
 * before any device work, `whole` untouched.  One process; shard planes do not travel between processes. */
typedef struct pt_film_shard_info {
    uint32_t shard /* 0 / 1 */, rank, count, n_tiles /* of the image */, own_tiles, _pad;
    uint64_t n_pixels /* of the image */;
} pt_film_shard_info;
typedef int (*pt_film_exchange_fn)(float* tile_sum, float* tile_max, uint32_t n_tiles, void* user);
int  pt_film_create_shard(int device, const pt_profile* profile, const pt_opts* opts, uint32_t windowed, pt_film** out);
int  pt_film_get_shard_info(const pt_film* film, pt_film_shard_info* out);
int  pt_film_shard_tile_noise(const pt_film* film, float lum_floor, float* tile_sum, float* tile_max, float* err_host);
int  pt_film_tile_stats_from_sums(const pt_film* film, const float* tile_sum, double target, pt_film_tile_stats* out);
int  pt_film_select_tiles(const pt_film* film, const float* tile_sum, double target, uint32_t dilate, uint32_t* tiles, uint32_t* n_out);
int  pt_film_render_until_adaptive_sharded(pt_film* film, const pt_scene* scene, const pt_film_adaptive_params* params,
                                           pt_film_exchange_fn exchange, void* exchange_user, pt_film_pass_fn on_pass, void* user,
                                           pt_film_tile_stats* out);
int  pt_film_render_until_windowed_sharded(pt_film* film, const pt_scene* scene, const pt_film_window_params* params,
                                           pt_film_exchange_fn exchange, void* exchange_user, pt_film_pass_fn on_pass, void* user,
                                           pt_film_tile_stats* out);
int  pt_film_exchange_comm(float* tile_sum, float* tile_max, uint32_t n_tiles, void* user /* pt_comm* */);
int  pt_film_assemble(pt_film* whole, const pt_film* const* shards, uint32_t n);

/* ------------------------------------------------------------------ */
/* measurement                                                         */
/* ------------------------------------------------------------------ */

typedef struct pt_timing {
    uint32_t launches;        /* launches of the dominant kernel in the last render
                                 (k_wf_trace for the wavefront integrator)         */
    float integrate_ms;       /* sum of their HIP-event durations                  */
    float postprocess_ms;     /* tone-map kernel                                   */
    float total_ms;           /* first launch -> last kernel done                  */
    float generate_ms;        /* per-stage sums (wavefront integrator)             */
    float trace_ms;
    float shade_ms;
    float shadow_ms;
    float accumulate_ms;
    uint32_t stage_launches;  /* all integrator launches                           */
    uint32_t bounce0_launches; /* launches of the fused bounce-0 kernel (k_wf_shade<GRID >= 2>: ChaCha block,
                                  camera cast, shading, shadow casts); 0 when the scene has no such kernel */
    float bounce0_ms;         /* sum of their HIP-event durations                  */
} pt_timing;

/* Exact work counters from the instrumented variant (PT_FLAG_COUNTERS);
 * they feed the algorithmic-bytes formula of SURVEY §8-d. */
typedef struct pt_counters {
    uint64_t samples;         /* path samples started                  */
    uint64_t segments;        /* closest-hit ray casts (R_seg)         */
    uint64_t shadow_rays;     /* get_light_info evaluations (R_sh)     */
    uint64_t nodes_visited;   /* KD nodes touched (V)                  */
    uint64_t tris_tested;     /* primitive tests (T)                   */
    uint64_t shaded_hits;     /* material fetches (H)                  */
    uint64_t rng_draws;
    uint64_t restarts;        /* alpha-walk continuation casts         */
    uint64_t max_nodes_per_cast;   /* longest single KD walk (wavefront integrator) */
    uint64_t casts_over_1k_nodes;
    uint64_t trace_nodes;          /* share of nodes_visited / tris_tested spent in  */
    uint64_t trace_tris;           /* closest-hit casts (the rest: shadow casts)      */
    uint64_t shadow_skipped;       /* of shadow_rays: not cast, because the light's BRDF term is exactly 0
                                    * and the visibility cannot change the colour                     */
    uint64_t bounce0_hits;         /* camera rays that hit a surface (shaded at bounce 0)             */
    uint64_t bounce0_shadow_rays;  /* shadow rays cast by the fused bounce-0 kernel (k_wf_shade<GRID >= 2>)  */
    uint64_t bounce0_tris;         /* primitive tests of that kernel (camera casts + shadow casts)    */
    uint64_t grid_tris;            /* of tris_tested: made through origin grids (camera / point lights) */
    uint64_t bounce0_cam_tris;     /* of bounce0_tris: the camera casts (also part of trace_tris)       */
    uint64_t deferred_casts;       /* closest-hit casts finished by k_wf_trace_wide (drain phase of k_wf_trace) */
    uint64_t exact_casts;          /* closest-hit casts k_wf_trace left to k_wf_trace_exact: rays whose direction has a component
                                    * below 8e-4, which the wavefront walker's slack does not cover (csrc/pt_integrator.h) */
    uint64_t masked_casts;         /* of segments: ray_cast calls of bounces >= 1 that were NOT cast because the escape mask of the
                                    * primitive the ray leaves proves them empty (csrc/pt_escape.h) */
    uint64_t bounce0_masked;       /* of masked_casts: found by the bounce-0 kernel (paths that never enter a queue) */
} pt_counters;

int pt_get_timing(const pt_scene* scene, pt_timing* out);
int pt_get_counters(const pt_scene* scene, pt_counters* out);
/* The camera-grid cull of the last frame rendered with this scene (synchronises the device): the number of 8x8 pixel
 * blocks of the rank's tiles and how many of them no camera ray can hit anything in - their samples are the background
 * (Renderer::render's miss branch, renderer/mod.rs:184-186) without an RNG block or a cast.  0 blocks: no cull ran
 * (no camera grid, PT_FLAG_NO_GRIDS / PT_FLAG_MEGAKERNEL / PT_FLAG_COUNTERS, PT_CAM_CULL=0). */
int pt_get_cull_stats(const pt_scene* scene, uint32_t* n_blocks, uint32_t* n_empty);
/* The scene's cache of ChaCha words (words 0-7 of block 0 of every work item; they depend on the item enumeration -
 * image size, samples, shard, tiling, sample batch - and on nothing else, so consecutive frames of one enumeration share
 * them): its device bytes, the work items of the enumeration it is keyed to (0: none - it is keyed when a frame directly
 * follows another of the same enumeration), how many of them are cached so far, and the fill launches since the scene
 * was made.  PT_RNG_CACHE=0 switches the cache off, PT_RNG_CACHE_GIB (16) is its budget; both are read per frame.  The
 * bytes are not part of pt_scene_info's queue_bytes or device_bytes. */
int pt_get_rng_cache_stats(const pt_scene* scene, uint64_t* bytes, uint64_t* items, uint64_t* items_cached, uint64_t* fills);
/* The scene's cache of camera hits (the closest hit of every work item's camera ray, 16 B per item; it depends on the
 * item enumeration, the camera and the geometry - not on the lights, the bounce count or, in an opaque scene, the
 * materials - so the frames of light and material edits and of a steady state read it instead of casting): its device
 * bytes, the work items of the view it is keyed to (0: none - it is keyed when a frame directly follows another of the
 * same enumeration and camera), how many of them are cached so far, and the launches of the storing and of the loading
 * variant of the bounce-0 kernel since the scene was made.  Only opaque, uninstrumented frames of the default pipeline
 * whose words come from the word cache use it; pt_scene_set_camera empties it (the allocation stays), a camera path
 * never stores and never allocates.  PT_HIT_CACHE=0 switches the cache off, PT_HIT_CACHE_GIB (8) is its budget; both are
 * read per frame.  The bytes are not part of pt_scene_info's queue_bytes or device_bytes. */
int pt_get_hit_cache_stats(const pt_scene* scene, uint64_t* bytes, uint64_t* items, uint64_t* items_cached, uint64_t* stores,
                           uint64_t* loads);
/* The scene's cache of bounce-0 shadow visibility (one byte per work item: two bits per light - unknown, not blocked,
 * blocked; in an opaque scene that answer depends on the camera hit, the light's kind and position and the geometry -
 * not on the materials, the light's colour or the bounce count - so the frames of material and light-colour edits and of
 * a steady state read it instead of casting): its device bytes, the work items of the view and lights it is keyed to
 * (0: none - it is keyed, and zeroed, when a frame directly follows another of the same view and light positions), how
 * often it was zeroed, and the launches of the bounce-0 variant that reads it and fills in what is unknown, since the
 * scene was made.  Only frames that load their camera hits, of scenes with one to four lights, use it; a moved light or
 * camera re-keys it (the allocation stays), a light orbit or camera path never zeroes and never allocates.
 * PT_VIS_CACHE=0 switches the cache off, PT_VIS_CACHE_GIB (1) is its budget; both are read per frame.  The bytes are
 * not part of pt_scene_info's queue_bytes or device_bytes. */
int pt_get_vis_cache_stats(const pt_scene* scene, uint64_t* bytes, uint64_t* items, uint64_t* resets, uint64_t* launches);
/* The scene's cache of bounce-1 hits (the closest hit of every work item's bounce-1 ray, 16 B per item; in an opaque scene
 * that ray is made from the camera hit, the material there and the item's random words - not from a light's position,
 * kind, colour or count, nor from the bounce count - so the frames of light edits and of a steady state read its hit
 * instead of casting): its device bytes, the work items of the view and material table it is keyed to (0: none - it is
 * keyed, and zeroed, when a frame directly follows another of the same view and materials), how many of them are cached
 * so far, how often it was zeroed, the storing and the loading launches, and the casts the loading launches found no
 * record for and left to the exact walker, since the scene was made.  Only frames that use the camera-hit cache and have
 * at least one bounce use it; pt_scene_set_materials and pt_scene_set_camera re-key it (the allocation stays), light
 * edits keep it.  PT_HIT1_CACHE=0 switches the cache off, PT_HIT1_CACHE_GIB (8) is its budget; both are read per frame.
 * The call waits for the device.  The bytes are not part of pt_scene_info's queue_bytes or device_bytes. */
int pt_get_hit1_cache_stats(const pt_scene* scene, uint64_t* bytes, uint64_t* items, uint64_t* items_cached, uint64_t* resets,
                            uint64_t* stores, uint64_t* loads, uint64_t* unknown_casts);
/* The bounce-0 launches that read the cache of bounce-1 hits themselves (a chunk that loads its camera hits, its bounce-0
 * shadow visibility and its bounce-1 hits: the kernel that makes the bounce-1 ray looks its hit up where the ray is made,
 * and a path whose ray is known to miss, behind a colour that is final, ends there without a queue record), since the scene
 * was made: those launches, the bounce-1 queue records they wrote with a known hit or miss, the records they did not write
 * (elided), and the records they wrote for items the cache has no record of (unknown; part of pt_get_hit1_cache_stats'
 * unknown_casts as well).  written + elided + unknown is what a frame that casts writes.  PT_HIT1_FUSED=0 (read per frame)
 * switches these launches off: bounce 1 then loads its hits in a launch of its own.  The call waits for the device. */
int pt_get_hit1_fused_stats(const pt_scene* scene, uint64_t* launches, uint64_t* written, uint64_t* elided, uint64_t* unknown);
/* The scene's cache of bounce-0 continuations (the direction the BRDF samples at every work item's camera hit and the
 * throughput behind it: 32 B per item in two planes; they are made from the camera hit, the material there and the item's
 * random words - the key of the bounce-1 hits - so the launches that look the bounce-1 hit up in the bounce-0 kernel load
 * them instead of sampling): its device bytes, the work items of the view and material table it is keyed to, how many of
 * them are cached so far, how often the planes were zeroed, the storing and the loading launches, and the hit lanes a
 * loading launch found without a record (missing: never, by construction - a check), since the scene was made.  The frame
 * that stores the bounce-1 hits stores it, from the bounce-0 kernel that frame runs anyway; only frames that use the
 * bounce-1 hit cache use it; pt_scene_set_materials and pt_scene_set_camera re-key it (the allocation stays), light edits
 * keep it.  PT_CONT_CACHE=0 switches the cache off, PT_CONT_CACHE_GIB (8) is its budget; PT_CONT_ESCAPE (default 1) lets the
 * loading launches take the escape-mask test's answer from the record too, where the scene's masks are those the records were
 * stored under or refilled for (pt_get_cont_escape_stats); all three are read per frame.  The call
 * waits for the device.  The bytes are not part of pt_scene_info's queue_bytes or device_bytes. */
int pt_get_cont_cache_stats(const pt_scene* scene, uint64_t* bytes, uint64_t* items, uint64_t* items_cached, uint64_t* resets,
                            uint64_t* stores, uint64_t* loads, uint64_t* missing);
/* The escape answers in those records (PT_CONT_ESCAPE).  Records stored before the scene's escape masks existed - a fresh view
 * stores in its second frame, the masks are built before the third - get their answers from a launch of their own, chunk by
 * chunk in the first frame that finds masks the records were not stored under: fill_launches and fill_items count those
 * launches and the items they went over; flagged_launches the loading launches that were told the records have answers;
 * fallback_lanes the lanes of such launches that ran the escape test themselves all the same (0 once the records are
 * refilled), since the scene was made.  The call waits for the device. */
int pt_get_cont_escape_stats(const pt_scene* scene, uint64_t* fill_launches, uint64_t* fill_items, uint64_t* flagged_launches,
                             uint64_t* fallback_lanes);
/* The lean variant of the loading bounce-0 launch (PT_B0_LEAN, default 1, read per frame).  A configuration - profile, options,
 * chunking - whose last counted frame was a planned one in which every bounce-0 launch loaded camera hits, visibility,
 * bounce-1 hits and continuations with the escape answers in the records, and in which no lane cast for a light, lacked a
 * record, ran the escape test or wrote a shadow record, launches a variant of that kernel without any of that code, at more
 * waves per SIMD (scenes without an orthographic light grid).  Any pt_scene_set_* call, a re-keyed cache or a moved mark, new
 * or dropped escape masks, and an unplanned, counting or tile-list frame put the configuration back on the general variant
 * until a frame has been counted clean again.  lean_launches / general_launches: the loading launches by variant;
 * guard_trips: frames in which a lean launch met a lane it has no code for - it writes nothing for the lane and flags the
 * frame, and the configuration's next render call fails with PT_ERR_DEVICE (never, by the rule above - a check) -, since the
 * scene was made.  The call does not wait for the device. */
int pt_get_b0_lean_stats(const pt_scene* scene, uint64_t* lean_launches, uint64_t* general_launches, uint64_t* guard_trips);
/* The lean variant of the fused shade pass of bounces 1 and 2 (PT_B1_LEAN, default 1, read per frame; independent of
 * PT_B0_LEAN).  A bounce whose shade pass adds the lights of known visibility itself, in a configuration whose last counted
 * frame was a planned one that wrote at that bounce fewer shadow records than 1/64 of the records it shaded, launches a
 * variant of that kernel without the shadow-record, sorting, exact-list, roulette and ChaCha code, at more waves per SIMD.  A
 * queue entry it cannot shade - a light of unknown visibility, a normal too long for the light grids - it writes nothing for
 * and appends to a list; a launch of the general kernel over that list follows on the same stream and shades the record
 * whole, so eligibility decides speed only and the frame is the same bit for bit.  Any pt_scene_set_* call, a re-keyed cache
 * or a moved mark, new or dropped escape masks, and an unplanned, counting or tile-list frame put the bounce back on the
 * general variant until a frame has been counted again.  PT_B1_LEAN_TEST_FORCE=1 (a hook for tests) takes the lean variant
 * wherever the plain fused pass would run at those bounces.  lean_launches_b1 / _b2: lean launches by bounce;
 * general_launches: general fused launches at those bounces; handed_over: entries the list passes shaded, since the scene was
 * made.  The call waits for the device. */
int pt_get_b1_lean_stats(const pt_scene* scene, uint64_t* lean_launches_b1, uint64_t* lean_launches_b2, uint64_t* general_launches,
                         uint64_t* handed_over);
/* The state words of the first `count` cached continuation records (at most pt_get_cont_cache_stats' items_cached), one
 * uint32 each: bit 0 - the record was written, bit 1 - it carries the escape test's answer, bit 2 - that answer.  A check
 * for tests.  The call waits for the device. */
int pt_scene_cont_states_copy(const pt_scene* scene, uint32_t* out, uint64_t count);
/* The scene's cache of bounce-2 hits: the bounce-1 hit cache one bounce later - the bounce-2 ray is made from the bounce-1
 * hit, the material there and the item's random words, so it has the same key (view and material table, no light, no
 * bounce count) and the same rules, values and meaning of every field.  Only frames that use the bounce-1 hit cache and
 * have at least two bounces use it; both planes are keyed, zeroed and stored by the same frame.  PT_HIT2_CACHE=0 switches
 * the cache off (PT_HIT1_CACHE=0 takes it out of use too), PT_HIT2_CACHE_GIB (8) is its budget; both are read per frame.
 * The call waits for the device.  The bytes are not part of pt_scene_info's queue_bytes or device_bytes. */
int pt_get_hit2_cache_stats(const pt_scene* scene, uint64_t* bytes, uint64_t* items, uint64_t* items_cached, uint64_t* resets,
                            uint64_t* stores, uint64_t* loads, uint64_t* unknown_casts);
/* The bounce-1 shade launches that read the bounce-1 shadow-visibility bytes themselves, and - where the chunk loads its
 * bounce-2 hits - the bounce-2 hit cache too, since the scene was made: chunks that took that kernel (launches), the
 * records whose lights it added itself because every live light's visibility was known (inlined: no shadow record), the
 * records it left to the shadow queue whole - an unknown bit, or a normal too long for the light grids - (deferred), the
 * bounce-2 records it wrote with a known hit word (next_written), the survivors that got no bounce-2 record because their
 * colour was final and their next cast is known to miss - from the plane or from the escape masks - (next_elided), and
 * the records it wrote for items the bounce-2 cache has no record of (next_unknown; part of pt_get_hit2_cache_stats'
 * unknown_casts as well).  PT_VIS1_FUSED (default 1) and PT_HIT2_FUSED (default 0: measured slower), read per frame, switch the
 * two steps: with the first off the launches are k_wf_shade's, with the second off bounce 2 loads its hits in a launch of
 * its own and next_written and next_unknown stay zero.  Scenes with a
 * directional light's orthographic grid never take the kernel.  The call waits for the device. */
int pt_get_bounce1_fused_stats(const pt_scene* scene, uint64_t* launches, uint64_t* inlined, uint64_t* deferred, uint64_t* next_written,
                               uint64_t* next_elided, uint64_t* next_unknown);
/* The scene's cache of bounce-1 shadow visibility (one byte per work item, the encoding of the bounce-0 one; the answer
 * of a shadow cast from a bounce-1 hit depends on that hit - the view, the material table, the item's words - and on the
 * light's kind and position, not on its colour or intensity): the fields of pt_get_vis_cache_stats - device bytes, work
 * items of the view, materials and lights it is keyed to, how often it was zeroed, launches of the shadow kernel that reads
 * it and fills in what is unknown.  Only frames that use the bounce-1 hit cache, of scenes with one to four lights that
 * all have a light grid, use it, for the sample batches that lie below its budget and whose bounce-1 shadow casts are a
 * launch of their own; a moved light, a new light count, a material edit and a camera move re-key it (the allocation
 * stays), colour and intensity edits keep it.  PT_VIS1_CACHE=0 switches the cache off, PT_VIS1_CACHE_GIB (1) is its
 * budget; both are read per frame.  The bytes are not part of pt_scene_info's queue_bytes or device_bytes. */
int pt_get_vis1_cache_stats(const pt_scene* scene, uint64_t* bytes, uint64_t* items, uint64_t* resets, uint64_t* launches);
/* The same caches by bounce.  Besides bounces 1 and 2 (above; they answer here too, with the same numbers) a scene keeps the
 * closest hits of bounces 3, 4 and 5 and the shadow visibility of bounces 2, 3 and 4: no light enters a later bounce's ray,
 * and the roulette of bounces 4+ draws from the item's words, so every later bounce's hits have the bounce-1 hits' key and
 * the visibility at bounce b that key plus the lights' kinds and positions.  A hit plane is in use where the plane one
 * bounce earlier is and the frame has that bounce; a visibility plane where that bounce's hit plane is, under
 * pt_get_vis1_cache_stats' conditions.  All hit planes are keyed, zeroed and stored by the same frame; a frame with more
 * than 5 bounces casts bounces 6+.
 *   pt_get_bounce_hits_cache_stats: bounce 1-5, the fields of pt_get_hit1_cache_stats (unknown_casts: that bounce's own).
 *   pt_get_bounce_vis_cache_stats:  bounce 1-4, the fields of pt_get_vis1_cache_stats.
 *   pt_get_bounce_fused_stats:      bounce 1-4, the fields of pt_get_bounce1_fused_stats for the shade launches of that
 *                                   bounce that add the lights of known visibility themselves; next_written and
 *                                   next_unknown are bounce 1's alone (PT_HIT2_FUSED).
 * Any other bounce: PT_ERR_INVALID.  The first and third wait for the device.
 * Switches, read per frame: PT_TAIL_HIT_CACHE (default 1) and PT_TAIL_HIT_CACHE_GIB (8, PER PLANE) for the hit planes of
 * bounces 3-5 as a group; PT_TAIL_VIS_CACHE (1) and PT_TAIL_VIS_CACHE_GIB (1, per plane) for the visibility planes of
 * bounces 2-4; PT_TAIL_VIS_FUSED for the shade pass of bounces 2-4.  A plane is 16 bytes (hits) or 1 byte (visibility)
 * per work item of the frame, however few items reach the bounce; a plane the device cannot provide is switched off for
 * the scene, and with it the planes of the bounces behind it.  The bytes are not part of pt_scene_info's queue_bytes or
 * device_bytes. */
int pt_get_bounce_hits_cache_stats(const pt_scene* scene, uint32_t bounce, uint64_t* bytes, uint64_t* items, uint64_t* items_cached,
                                   uint64_t* resets, uint64_t* stores, uint64_t* loads, uint64_t* unknown_casts);
int pt_get_bounce_vis_cache_stats(const pt_scene* scene, uint32_t bounce, uint64_t* bytes, uint64_t* items, uint64_t* resets,
                                  uint64_t* launches);
int pt_get_bounce_fused_stats(const pt_scene* scene, uint32_t bounce, uint64_t* launches, uint64_t* inlined, uint64_t* deferred,
                              uint64_t* next_written, uint64_t* next_elided, uint64_t* next_unknown);
/* Workgroups of the fused bounce-0 kernel of opaque scenes that the runtime places on one compute unit of `device`
 * (hipOccupancyMaxActiveBlocksPerMultiprocessor at the kernel's workgroup size): which = 0 the variant that computes
 * its ChaCha words, 1 the variant that reads them from the word cache, 2 and 3 the variants of 1 that store and that
 * load the camera hits, 4 the variant of 3 with the shadow-visibility cache, 5 that variant of scenes with a
 * directional light and 6 the variant that also reads the bounce-1 hits and loads the bounce-0 continuation.  One
 * workgroup is one wave per SIMD. */
int pt_kernel_occupancy(int device, int which, int* blocks_per_cu);

/* Scene statistics after the KD build. */
typedef struct pt_scene_info {
    uint64_t n_prims;         /* triangles + spheres              */
    uint64_t n_kd_nodes;
    uint64_t n_kd_leaves;
    uint64_t n_leaf_refs;     /* primitive references in leaves   */
    uint32_t kd_depth;
    uint32_t has_translucent; /* any opacity != 1 or opacity texture */
    float kd_build_seconds;
    float upload_seconds;
    uint64_t device_bytes;
    /* origin grids (cube maps of primitive lists around the camera / the point lights, csrc/pt_grid.h) */
    uint32_t cam_grid_res;    /* cells per face edge; 0 = camera rays use the KD-tree */
    uint32_t light_grids;     /* lights whose shadow rays use a grid (all or none)    */
    uint64_t grid_refs;       /* list entries of all grids                            */
    float grid_build_seconds;
    /* escape masks (csrc/pt_escape.h): proofs of misses for the rays that leave a primitive.  Built on the device when the
     * scene is about to render its third frame of the default pipeline (PT_ESCAPE_AFTER; a one-shot render is better off
     * without them) or when pt_scene_escape_copy asks for them: zero until then */
    float escape_build_seconds;
    uint32_t escape_prims;      /* primitives with a mask (the others: all directions "may hit") */
    float escape_clear_fraction; /* of those primitives' 384 direction cells: proven empty */
    /* the path queues of the LAST frame rendered from this scene (csrc/pt_gpu.hip, "frame plan"): the first frame of a
     * configuration runs in chunks of a fixed budget (PT_QUEUE_GIB, default 8; later frames: what their records need, at most PT_QUEUE_STEADY_GIB, 32) with every queue as long as the chunk and
     * counts what each bounce produces; later frames of the same configuration get queues of exactly those lengths */
    uint64_t queue_bytes;        /* device memory held by the queues, hit / shadow records, RNG planes and lists */
    uint32_t queue_chunk_items;  /* work items (pixel samples) per pass over the bounces                        */
    uint32_t frame_planned;      /* 1: sized from an earlier frame's counts; 0: first frame of its configuration */
} pt_scene_info;
int pt_scene_get_info(const pt_scene* scene, pt_scene_info* out);

/* ------------------------------------------------------------------ */
/* test hooks (parity tests call the device code piecewise)            */
/* ------------------------------------------------------------------ */

/* One record per ray: the reference's first entry of ray_cast()
 * (renderer/utils.rs:11-21): prim = global primitive index in (model,
 * triangle) order (spheres count as one primitive each, interleaved in
 * model order), or -1 for a miss. */
typedef struct pt_hit {
    int32_t prim;
    int32_t flags;   /* bit0 backface (det<0), bit1 sphere, bit2 sphere exit hit */
    float dist;
    float u;
    float v;
} pt_hit;

/* rays: n x 6 f32 (origin3, direction3), HOST pointers. */
int pt_trace_rays(const pt_scene* scene, const float* rays, uint64_t n, pt_hit* out);

/* The first entry of ray_cast() through the wavefront integrator's own cast kernel (k_wf_trace; the rays of bounces
 * >= 1 of every frame go through it).  mode bit 0: start at the home node of the primitive the ray leaves
 * (start_prims[i], entry lists); bit 1: hand every cast to the cooperative kernel k_wf_trace_wide; bit 2 (study switch):
 * WITHOUT the hand-over of the rays the walker's slack does not cover (a direction component below 8e-4) to k_wf_trace_exact. */
int pt_trace_rays_wavefront(const pt_scene* scene, const float* rays, const uint32_t* start_prims, uint64_t n,
                            uint32_t mode, pt_hit* out);

/* The origin grids of a scene as the DEVICE built them (csrc/pt_grid_build.h): which = 0 the camera grid, 1 + i the grid
 * of light i.  pt_scene_grid_header fills the header fields of a pth_origin_grid (include/pthost.h; enabled = 0: the
 * scene has no such grid; cell_off / refs are left null), pt_scene_grid_copy copies the n_cells + 1 cell offsets and
 * the n_refs list entries into caller-provided host arrays - for the tests, which compare them with the host builder's
 * (pth_origin_grid_build: the same lists byte for byte) and run the conservativeness checks on them. */
/* The escape masks of a scene (csrc/pt_escape.h) as the device built them: 80 bytes per primitive - f32 normal (0 0 0: the
 * primitive has no mask), f32 v0, two spare words, then six faces x 64 direction bits (bit = row * 8 + column, set = "may
 * hit").  For the tests, which aim rays through clear cells and require brute force to find nothing. */
int pt_scene_escape_copy(const pt_scene* scene, void* out, uint64_t bytes);

/* The lookup the shade kernel makes before it casts a bounce ray (escape_proves_miss, csrc/pt_escape.h), run on the device for
 * n queries: proven[i] = 1 where the mask of primitive prims[i] proves that the ray rays[i] (origin3, direction3) hits nothing -
 * the height of the origin above the primitive's plane within [5e-6, 1e-3] and the direction's cell clear - else 0.  HOST
 * pointers.  Builds the masks if the scene has none yet, as pt_scene_escape_copy does.  PT_ERR_INVALID: a null pointer, a
 * primitive index >= n_prims (checked before anything runs on the device), a scene that cannot have masks. */
int pt_escape_query(const pt_scene* scene, const uint32_t* prims, const float* rays /* n x 6 */, uint64_t n, uint8_t* proven);

struct pth_origin_grid;
struct pth_grid_ref;
int pt_scene_grid_header(const pt_scene* scene, uint32_t which, struct pth_origin_grid* out);
int pt_scene_grid_copy(const pt_scene* scene, uint32_t which, uint32_t* cell_off, struct pth_grid_ref* refs);

/* Up to max_hits hits per ray in the reference's sorted order (all hits,
 * stable by (dist, primitive order)); counts[i] = number written. */
int pt_trace_rays_all(const pt_scene* scene, const float* rays, uint64_t n, uint32_t max_hits,
                      pt_hit* out, uint32_t* counts);

/* Triangle::intersect (internal/triangle.rs:37-82) on the device for n
 * independent (ray, triangle) pairs: rays n x 6, tris n x 9 (v0,v1,v2). */
int pt_intersect_triangles(int device, const float* rays, const float* tris, uint64_t n,
                           pt_hit* out);

/* First n_words of StdRng::seed_from_u64(seed) (rand 0.8.5 = ChaCha12,
 * PCG32 key expansion) generated ON THE DEVICE for each seed. */
int pt_rng_words(int device, const uint64_t* seeds, uint64_t n_seeds, uint32_t n_words,
                 uint32_t* out);

/* Device libm restatements evaluated on the GPU (bit-exactness checks
 * against glibc): fn 0 = powf(x, 1/2.2f), 1 = acosf, 2 = sinf, 3 = cosf. */
int pt_eval_math(int device, int fn, const float* x, uint64_t n, float* out);

/* Measurement aid for the roofline ("achievable-copy figure with a
 * stream kernel on the box"): copies `bytes` of device memory with a plain
 * 16-byte-per-lane grid-stride kernel `reps` times and returns the best
 * read+write rate in GB/s (2 * bytes / time).  No reference counterpart. */
int pt_measure_copy_bandwidth(int device, uint64_t bytes, uint32_t reps, double* gb_per_s);

/* Second yardstick: scattered loads.  Every lane of every wavefront reads `bytes_per_load` (8 or 16) bytes at
 * pseudo-random 16-byte-aligned offsets of a `table_bytes` table, `loads_per_lane` times with eight independent
 * loads in flight; returns lane-loads per second in units of 1e9.  This is the access pattern of the KD walk, and
 * its ceiling (not HBM bandwidth) is what k_wf_trace / k_wf_shadow run against.  No reference counterpart. */
int pt_measure_gather_rate(int device, uint64_t table_bytes, uint32_t bytes_per_load, uint32_t loads_per_lane,
                           double* giga_loads_per_s);

/* ------------------------------------------------------------------ */
/* sample-coherent AOVs (no reference counterpart)          */
/* ------------------------------------------------------------------ */

/* Feature planes that are sample-coherent with the beauty frame: the pass replays, for every sample of the frame, the camera
 * cast and the alpha walk of render_pixel (mod.rs:107-124, 182-205) - and nothing after them - and sums the features of the
 * surfaces the walks stop at.  Every step is one f32 IEEE operation, uncontracted, in the order written.
 *
 * The sample record.  Pixel i (global index x + y*W), sample s = 1..N (N = profile.samples): the generator is
 * StdRng::seed_from_u64(s + i*N); draws 0 and 1 are the jitter (r1, r2), the ray is primary_ray's; the surface is the one
 * render_pixel shades at bounce 0: ray_cast, then the alpha walk with its draws taken from index 2 on (an entry of opacity
 * >= 1 ends the walk, one of opacity > 0.001 ends it when its draw < opacity, and a walk that skips every entry keeps the
 * last one; a walk of more than 14 draws goes on into ChaCha block 1).  16 f32:
 *   [0..2]   unit shading normal: n = shading_normal; nn = (n.x*n.x + n.y*n.y) + n.z*n.z; n * (1/sqrt(nn)) when
 *            0 < nn < inf, else 0 (the rule of pt_denoise's prep)
 *   [3]      depth: the hit's `dist` (the sort key pt_trace_rays reports)
 *   [4..6]   MaterialSample albedo            [7] 1.0 (coverage)
 *   [8..10]  hit position (o + d*dist; spheres: o + d*t as Model::intersect computes it)
 *   [11,12]  roughness (after the max(1e-4) clamp), metalness
 *   [13]     lum(emissive) = (0.2126f*r + 0.7152f*g) + 0.0722f*b
 *   [14]     global primitive index as int32 bits      [15] 1.0
 * A sample without a surface: sixteen +0.0f, [14] = int32 -1.  Non-finite features propagate (outside the contract).
 * aov_flags: PT_AOV_FIRST_ENTRY - the first list entry, no walk, no draws; PT_AOV_CENTRE - r1 = r2 = 0.5 instead of the
 * jitter draws (the walk still draws from index 2).
 *
 * The pixel record, 16 f32:
 *   [0..13]  the sum of the samples' floats 0..13 in a fixed order, a pure function of N: the samples are taken in blocks of
 *            64 consecutive sample numbers; inside a block a missing sample is +0.0f and the 64 values are reduced by the
 *            pairwise tree x[j] = x[2j] + x[2j+1], six levels; the total is the first block's sum, then + the next block's,
 *            in block order (tests/aov_model.py reduce_records)
 *   [14]     the primitive of the lowest-numbered covered sample (int32 bits, -1: none)
 *   [15]     how many covered samples have that primitive, as a float ([15] < [7]: an edge pixel)
 *
 * pt_render_aov / _device: n_local x 16 f32 in the packed local order of pt_render (shard fields of opts as there: the
 * global index goes into the seed).  Of the profile only width, height and samples are used; of opts the device, the shard
 * fields and PT_FLAG_NO_GRIDS (the cast goes through the KD-tree instead of the camera grid: the same bits); the other flags,
 * sample_batch and the callbacks are ignored.  The device form is asynchronous on hip_stream and allocates nothing (sharded:
 * the scene's tile table, as pt_render_device); d_aov: 16-byte aligned.  They follow pt_scene_set_camera and the scene edits
 * like pt_render_guides, read none of the scene's frame caches and leave its frame plan, caches and statistics untouched.
 * pt_render_aov_samples (test hook): the sample records, N planes of n_local x 16 f32 (plane s - 1 = sample s), at most
 * 256 MiB.  PT_ERR_INVALID before any device work: a null pointer, samples == 0, unknown flag bits, a rank without pixels,
 * a misaligned d_aov, sample planes above 256 MiB. */
enum { PT_AOV_FLOATS = 16, PT_AOV_FIRST_ENTRY = 1, PT_AOV_CENTRE = 2 };
int pt_render_aov(const pt_scene* scene, const pt_profile* profile, const pt_opts* opts, uint32_t aov_flags,
                  float* aov /* host, n_local x 16 */);
int pt_render_aov_device(const pt_scene* scene, const pt_profile* profile, const pt_opts* opts, uint32_t aov_flags,
                         void* d_aov, void* hip_stream);
int pt_render_aov_samples(const pt_scene* scene, const pt_profile* profile, const pt_opts* opts, uint32_t aov_flags,
                          float* records /* host, N x n_local x 16, <= 256 MiB */);

/* Guides (PT_GUIDE_FLOATS per pixel, the layout of pt_render_guides) from pixel records r of a frame of `samples` samples.
 * cov = r[7]; the pixel is valid iff cov > 0 and cov + cov >= (float)samples.  A valid pixel: normal = r[0..2] (left
 * unnormalised: the filters' prep normalises it), depth = r[3] / cov, albedo = r[4..6] / (float)samples, prim = r[14].
 * An invalid pixel is pt_render_guides' miss record: floats 0, depth -1.0f, prim -1.  The device form is asynchronous,
 * allocates nothing and wants 16-byte aligned planes; device: HIP ordinal, -1 = current. */
int pt_aov_guides(int device, uint64_t n_pixels, uint32_t samples, const float* aov, float* guides /* host */);
int pt_aov_guides_device(int device, uint64_t n_pixels, uint32_t samples, const void* d_aov, void* d_guides, void* hip_stream);

/* pt_render_denoised (variance = 0) / pt_render_denoised_var (variance != 0: a moments frame) with the guides of
 * pt_render_aov + pt_aov_guides in place of pt_render_guides': frame, AOV pass, conversion and filter on one stream.  Their
 * arguments, their rules; shard_count > 1 is PT_ERR_UNSUPPORTED. */
int pt_render_denoised_aov(const pt_scene* scene, const pt_profile* profile, const pt_opts* opts,
                           const pt_denoise_params* params, int variance, uint32_t aov_flags, uint8_t* rgb8, float* color);

/* ------------------------------------------------------------------ */
/* temporal history (no reference counterpart)              */
/* ------------------------------------------------------------------ */

/* A history carries the sample sums of the frames of a camera path from view to view.  It is for one image size W x H,
 * unsharded, on one device, and for a STATIC scene: the surface point a pixel's AOV record (pt_render_aov) holds is projected
 * into the previous camera, the nearest pixel there (or one of its 2x2 footprint) gives its sums and its count when its
 * surface agrees, and the new frame's sums are added.  It holds two sets of planes - accum (3 f32, sums of sample radiance),
 * moments (2 f32, pt_render_moments' sums), count (u32), surf (2 x float4: (P.xyz, dist), (u.xyz, prim as int bits); no
 * surface: (0,0,0,-1.f), (0,0,0,int -1)) - and one plane of guides (PT_GUIDE_FLOATS, pt_aov_guides of the newest frame).
 * Every step is one f32 IEEE operation, uncontracted, in the order written (tests/history_model.py restates it bit for bit).
 *
 * View constants of a camera (host): c0..c3 = columns of `transform`, rows 0..2; A = (c0 c1 c2) in f64; cofactors C[i][j] as
 * 2x2 determinants p*q - r*s; det = a00*C00 + a01*C01 + a02*C02 (0 or not finite: PT_ERR_INVALID); M[r][c] =
 * (float)(C[c][r] / det); ty = tanf(fov / 2.f) (the host libm call of the scene's tan_half_fov); tx = ty * ((float)W /
 * (float)H).
 *
 * pt_history_advance, a frame of N samples with AOV records r rendered from `camera`, per destination pixel p:
 *   surface   cov = r[7]; valid iff cov > 0 && cov + cov >= (float)N (pt_aov_guides' rule).  P = r[8..10] / cov; dist =
 *             r[3] / cov; nn = (nx*nx + ny*ny) + nz*nz; u = n * (1.f / sqrt(nn)) when 0 < nn < inf, else 0; prim = r[14].
 *             surf[p] of the new view is written in either case (invalid: the no-surface record).
 *   project   with the PREVIOUS view's constants: v = P - c3; qx = (M00*v.x + M01*v.y) + M02*v.z, qy, qz alike; w = -qz;
 *             OUTSIDE when !(w > 0).  fx = ((qx / w / tx + 1.f) * 0.5f) * (float)W; fy = ((1.f - qy / w / ty) * 0.5f) *
 *             (float)H; OUTSIDE when !(fx >= 0 && fx < (float)W && fy >= 0 && fy < (float)H) (in float: NaN and huge values
 *             end here).  x0 = (int)floorf(fx), y0 alike.
 *   taps      sx = (fx - (float)x0 >= 0.5f) ? 1 : -1, sy alike; (x0,y0), (x0+sx,y0), (x0,y0+sy), (x0+sx,y0+sy) in this
 *             order, a tap outside the image skipped.  Tap q passes iff, in this order: 1. count_prev[q] > 0; 2.
 *             surf_prev[q].dist >= 0; 3. (u.x*uq.x + u.y*uq.y) + u.z*uq.z >= normal_cos; 4. e = Pq - P, fabsf((e.x*u.x +
 *             e.y*u.y) + e.z*u.z) <= plane_tol * dist.  The first tap that passes is the source.  No primitive test.
 *   merge     a source q: c = count_prev[q] with its sums; if c > max_samples: f = (float)max_samples / (float)c, every
 *             float of the sums times f, c = max_samples; accum[p] = A + a_frame[p], moments[p] = m + m_frame[p],
 *             count[p] = c + N.  No source (no surface, OUTSIDE, no tap passes, an empty history): the frame's values, bits
 *             unchanged, count[p] = N.
 *   map       (optional, int32 per pixel) the source's pixel index, or -1 no surface, -2 OUTSIDE, -3..-6: which of the
 *             tests 1-4 the PRIMARY tap (x0,y0) failed.
 * The first frame after create / reset has no previous view: the new camera's constants stand for it and every count is 0.
 * The guides of the new view come from the same records (pt_aov_guides).  The sets swap when the launch is enqueued.
 * PT_ERR_INVALID before any device work: a null pointer (map excepted), N < 1, max_samples + N > PT_FILM_MAX_SAMPLES, a
 * singular camera, misaligned device planes (16 bytes; d_map 4).  The host form takes planes in pt_render_moments' and
 * pt_render_aov's unsharded layouts and blocks; the device form is asynchronous on hip_stream and allocates nothing.
 *
 * pt_history_add_frame renders the frame for the scene's CURRENT camera on the scene's device and advances: with j =
 * frame_index % K (K = params.rotate, N = profile.samples), K == 1: pt_render_moments_device; K > 1:
 * pt_render_window_device of profile.samples = K*N, [j*N, j*N + N) on zeroed buffers; then pt_render_aov_device (samples = N,
 * flags 0) and pt_history_advance_device.  PT_FLAG_MEGAKERNEL and shard_count > 1: PT_ERR_UNSUPPORTED.  The history does not
 * watch the scene: after a light, material or geometry edit the caller resets it (as with pt_film and pt_lightmix).
 *
 * pt_history_resolve: accum / (float)count and pt_render's post-processing, every pixel by its own count (the non-uniform
 * film resolve).  pt_history_denoise: the film filter (pt_film_denoise: prep, passes, finish) on the history's planes, counts
 * and its own guides; variance 0 plain, 1 variance-guided.  Refused (PT_ERR_INVALID): an empty history, variance = 1 with any
 * count below 2, and what pt_film_denoise refuses of params and lum_floor.  The device forms are asynchronous on hip_stream
 * (denoise: the scratch is the history's, made on the first call).
 * pt_history_kernel_times: `reps` timings (ms) of k_hist_advance on the history's current planes (nothing is swapped). */
typedef struct pt_history pt_history;
typedef struct pt_history_params {
    float normal_cos;       /* test 3 */
    float plane_tol;        /* test 4, relative to the pixel's depth */
    uint32_t max_samples;   /* the cap on a history count before a frame is added */
    uint32_t rotate;        /* K of pt_history_add_frame, >= 1 */
} pt_history_params;
typedef struct pt_history_info {
    uint32_t width, height;
    uint32_t frames;          /* advances since create / reset */
    uint32_t last_samples;    /* N of the last one */
    uint32_t min_count, max_count;   /* bounds of the count plane (0, 0: empty) */
    uint64_t device_bytes;
    pt_history_params params;
} pt_history_info;
typedef struct pt_history_view {
    float c3[3];
    float M[9];   /* row-major */
    float tx, ty;
} pt_history_view;
/* The best point of the grid of tools/measure_temporal_gain.py (tests/golden/temporal_gain.json: four golden scenes, 64x48,
 * 4 spp, one degree of orbit a frame; max_samples = 4 frames x 4 spp). */
#define PT_HISTORY_DEFAULT_NORMAL_COS 0.97f
#define PT_HISTORY_DEFAULT_PLANE_TOL 0.01f
#define PT_HISTORY_DEFAULT_MAX_SAMPLES 16u
#define PT_HISTORY_DEFAULT_ROTATE 8u
void pt_history_params_default(pt_history_params* params);
int  pt_history_create(int device, uint32_t width, uint32_t height, const pt_history_params* params, pt_history** out);
void pt_history_destroy(pt_history* hist);
int  pt_history_reset(pt_history* hist);
int  pt_history_get_info(const pt_history* hist, pt_history_info* out);
int  pt_history_get_view(const pt_history* hist, int which /* 0 previous, 1 current */, pt_history_view* out);
int  pt_history_advance(pt_history* hist, const pt_camera* camera, uint32_t samples, const float* accum, const float* moments,
                        const float* aov, int32_t* map /* may be NULL */);   /* host */
int  pt_history_advance_device(pt_history* hist, const pt_camera* camera, uint32_t samples, const void* d_accum,
                               const void* d_moments, const void* d_aov, void* d_map, void* hip_stream);
int  pt_history_add_frame(pt_history* hist, const pt_scene* scene, const pt_profile* profile, const pt_opts* opts,
                          uint32_t frame_index);
int  pt_history_read(const pt_history* hist, float* accum, float* moments, uint32_t* counts, float* surf /* n x 8 */,
                     float* guides /* n x 8 */, int32_t* map /* of the last pt_history_add_frame */);   /* host, each may be NULL */
int  pt_history_resolve(const pt_history* hist, int tonemap, uint8_t* rgb8, float* color);   /* host */
int  pt_history_resolve_device(const pt_history* hist, int tonemap, void* d_rgb8, void* d_color, void* hip_stream);
int  pt_history_denoise(const pt_history* hist, int variance, const pt_denoise_params* params, float lum_floor, uint8_t* rgb8,
                        float* color);   /* host */
int  pt_history_denoise_device(const pt_history* hist, int variance, const pt_denoise_params* params, float lum_floor,
                               void* d_rgb8, void* d_color, void* hip_stream);
int  pt_history_kernel_times(const pt_history* hist, uint32_t reps, float* ms_advance);

const char* pt_last_error(void);
const char* pt_version(void);

#ifdef __cplusplus
}
#endif
#endif /* PTGPU_H */
