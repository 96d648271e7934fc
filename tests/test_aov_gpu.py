"""Sample-coherent AOVs on the GPU (include/ptgpu.h pt_render_aov): the sample records against the float64 model
and the oracle's hit lists, the pixel records against the numpy tree bit for bit, the anchor to pt_render_guides, the
coherence with the beauty frame's own walk, the paths and partitions, the scene left alone, the composition, the refusals."""
import ctypes as C
import json

import numpy as np
import pytest

import aov_model as am
import scene_builder as sb
from conftest import GOLDEN, SCENES

f32 = np.float32
pytestmark = pytest.mark.gpu
OPAQUE, TRANSLUCENT = "albedo-none", "none-point_dir"


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def prim_of(records):
    return np.ascontiguousarray(records[..., 14]).view(np.int32)


def lum32(rgb):
    rgb = np.asarray(rgb, f32)
    return ((f32(0.2126) * rgb[..., 0] + f32(0.7152) * rgb[..., 1]).astype(f32) + f32(0.0722) * rgb[..., 2]).astype(f32)


def built(pta, name):
    return sb.build(sb.case_by_name(name), pta=pta)


@pytest.fixture(scope="module")
def gpu_built(pta):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = pta.GpuScene(built(pta, name))
        return cache[name]
    yield get
    for g in cache.values():
        g.close()


# ------------------------------------------------------------------------------------------------ 1. samples against the model
@pytest.mark.parametrize("name", am.CASES)
def test_sample_records_equal_the_model(pta, oracle, scene_cache, name):
    """Non-fragile samples: the primitive and dist are the oracle's list entry the model's walk selects, bit for bit; the
    fields without a texture behind them are the material's factors exactly; every other field is within twice the deviation
    float32 arithmetic showed on the CPU (tests/golden/aov_tolerance.json)."""
    tol = json.loads((GOLDEN / "aov_tolerance.json").read_text())["fields"]
    model, scene, camera = am.model_of(name, pta, oracle, scene_cache)
    prof = am.sample_profile(pta)
    rec = am.records_f64(model, prof)
    assert rec.fragile.mean() <= am.FRAGILE_CAP
    g = pta.GpuScene(scene)
    got = g.render_aov_samples(prof)
    g.close()
    assert got.shape == (am.SAMPLES, prof.width * prof.height, pta.PT_AOV_FLOATS)
    ok = ~rec.fragile
    prim = prim_of(got)
    covered = prim >= 0
    assert np.array_equal(prim[ok], rec.prim[ok]), (name, int((prim != rec.prim)[ok].sum()))
    assert np.array_equal(bits(got[..., 3])[ok & covered], bits(rec.dist)[ok & covered]), name
    assert np.array_equal(got[..., 7], covered.astype(f32)) and np.array_equal(got[..., 15], covered.astype(f32)), name
    assert (bits(got[~covered][:, [k for k in range(16) if k != 14]]) == 0).all(), (name, "a sample without a surface is +0.0f")
    dev = am.deviation(got, rec, am.origin_of(camera))
    for field, d in dev.items():
        worst = float(d[ok].max())
        print(f"{name}: {field} deviates by {worst:.3e} (bound {2.0 * tol[field]:.3e})")
        assert worst <= 2.0 * tol[field], (name, field, worst, 2.0 * tol[field])
    plain = ok & covered & ~rec.textured
    for sl in (am.FIELDS["albedo"], am.FIELDS["roughness"], am.FIELDS["metalness"]):
        assert np.array_equal(got[..., sl].astype(np.float64)[plain], rec.values[..., sl][plain]), (name, sl)


# ------------------------------------------------------------------------------------------------ 2. the reduction
def aov_on_device(pta, g, prof, opts=None, flags=0):
    import torch
    n = len(pta.local_pixel_map(prof, opts)) if opts is not None else prof.width * prof.height
    d = torch.full((n, pta.PT_AOV_FLOATS), -7.0, dtype=torch.float32, device="cuda")
    assert d.data_ptr() % 16 == 0
    g.render_aov_device(prof, opts, d.data_ptr(), flags, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return d.cpu().numpy()


@pytest.mark.parametrize("name", [OPAQUE, TRANSLUCENT])
def test_pixel_records_are_the_tree_over_the_sample_records(pta, gpu_built, name):
    g = gpu_built(name)
    for n_samples in (1, 2, 3, 5, 64, 65, 130):
        prof = pta.Profile.make(9, 7, n_samples, 0)      # 63 pixels: no multiple of any pixels-per-wavefront count
        want = am.reduce_records(g.render_aov_samples(prof))
        host = g.render_aov(prof)
        assert np.array_equal(bits(host), bits(want)), (name, n_samples, np.argwhere(bits(host) != bits(want))[:4].tolist())
        assert np.array_equal(bits(aov_on_device(pta, g, prof)), bits(want)), (name, n_samples)
        assert (host[:, 7] > 0).any() and (host[:, 15] <= host[:, 7]).all()
    assert (host[:, 15] < host[:, 7]).any(), (name, "130 samples: some pixel is an edge pixel")


# ------------------------------------------------------------------------------------------------ 3. the existing guides
@pytest.mark.parametrize("name", ["normal-point", "spheres-dir", "all-point"])
def test_centre_first_entry_records_are_the_guides(pta, gpu_built, name):
    """PT_AOV_CENTRE | PT_AOV_FIRST_ENTRY with one sample is k_guides' ray and k_guides' surface: depth, albedo and primitive
    bit for bit, the normal normalised (the one-sample tree adds +0.0f: a negative zero component comes out positive)."""
    g = gpu_built(name)
    w, h = 16, 12
    guides = g.render_guides(w, h)
    aov = g.render_aov(pta.Profile.make(w, h, 1, 0), aov_flags=pta.PT_AOV_CENTRE | pta.PT_AOV_FIRST_ENTRY)
    hit = guides[:, 7].view(np.int32) >= 0
    assert np.array_equal(prim_of(aov), guides[:, 7].view(np.int32))
    assert np.array_equal(aov[:, 7], hit.astype(f32)) and np.array_equal(aov[:, 15], hit.astype(f32))
    assert np.array_equal(bits(aov[hit, 3]), bits(guides[hit, 3])) and np.array_equal(bits(aov[hit, 4:7]), bits(guides[hit, 4:7] + f32(0)))
    n = guides[:, 0:3]
    with np.errstate(all="ignore"):
        nn = ((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]).astype(f32) + n[:, 2] * n[:, 2]).astype(f32)
        unit = (n * (f32(1.0) / np.sqrt(nn))[:, None]).astype(f32) + f32(0.0)
    unit = np.where(((nn > 0) & (nn < np.inf) & hit)[:, None], unit, f32(0))
    assert np.array_equal(bits(aov[:, 0:3]), bits(unit)), name
    assert (bits(aov[~hit][:, [k for k in range(16) if k != 14]]) == 0).all()
    if name == "spheres-dir":
        assert hit.any() and not hit.all(), "a frame with misses"
    # ... and through pt_aov_guides: k_guides' planes but for the normal's length
    conv = pta.aov_guides(1, aov)
    assert np.array_equal(bits(conv), bits(am.guides_of(aov, 1)))
    assert np.array_equal(bits(conv[~hit]), bits(guides[~hit])), "k_guides' miss record"
    assert np.array_equal(bits(conv[hit, 3]), bits(guides[hit, 3])) and np.array_equal(conv[:, 7].view(np.int32), guides[:, 7].view(np.int32))


# ------------------------------------------------------------------------------------------------ 4. the beauty's walk
def glow_scene(pta):
    """The `open` geometry under no light and a black background: translucent floor, panel and ball, distinct emissive
    factors, an emissive texture on the floor and the wall."""
    case = sb.Case("aov-glow", "open", "emissive", "none", "alpha", 0, "FILMIC", 0, False)
    mats = sb.case_materials(case, pta)
    for k, m in enumerate(mats):
        m.emissive = (C.c_float * 3)(0.3 + 0.1 * k, 0.9 - 0.11 * k, 0.05 + 0.07 * k)
        if sb.MATERIALS[k] not in ("floor", "wall"):
            m.tex_emissive = -1
    tris, models = sb.make_geometry(pta, case.geometry)
    tex, texels, _ = sb._TEX["t"]
    return sb.BuiltScene(pta, tris, models, mats, tex, texels, [], sb.make_camera(pta), (0.0, 0.0, 0.0))


def test_the_replayed_walk_is_the_frames_walk(pta):
    """bounces = 0, no lights, background 0: a sample's radiance is the emissive colour of the surface its alpha walk stopped
    at, so its luminance is float 13 of the sample record, bit for bit, and it is the background exactly where no surface is."""
    scene = glow_scene(pta)
    g = pta.GpuScene(scene)
    assert g.info().has_translucent
    for w, h, n_samples in ((16, 12, 3), (9, 7, 5)):
        prof = pta.Profile.make(w, h, n_samples, 0)
        rec = g.render_aov_samples(prof)
        for flags in (0, pta.PT_FLAG_NO_GRIDS):
            rad = g.render_samples(prof, pta.Opts.make(flags=flags))
            assert np.array_equal(bits(lum32(rad)), bits(rec[..., 13])), (w, h, flags)
            covered = rec[..., 15] > 0
            assert (bits(rad[~covered]) == 0).all() and covered.any() and not covered.all()
            assert (covered | ~(rad != 0).any(axis=-1)).all(), "radiance only where a surface is"
        first = g.render_aov_samples(prof, aov_flags=pta.PT_AOV_FIRST_ENTRY)
        assert not np.array_equal(bits(first[..., 13]), bits(rec[..., 13])), "the walk skips translucent first entries"
    g.close()


# ------------------------------------------------------------------------------------------------ 5. paths and partitions
@pytest.mark.parametrize("name", [OPAQUE, TRANSLUCENT])
def test_kd_path_and_shards_give_the_same_bits(pta, gpu_built, name):
    # (16 x 16 tiles: the smallest pt_opts takes - tile_w * tile_h must be a multiple of 256; 3 x 3 of them, clipped on two sides)
    g = gpu_built(name)
    w, h = 37, 35
    for n_samples in (3, 65):
        prof = pta.Profile.make(w, h, n_samples, 0)
        whole = g.render_aov(prof)
        assert g.info().cam_grid_res > 0
        assert np.array_equal(bits(g.render_aov(prof, pta.Opts.make(flags=pta.PT_FLAG_NO_GRIDS))), bits(whole)), (name, n_samples)
        seen = np.zeros(w * h, bool)
        for rank in range(3):
            o = pta.Opts.make(shard_rank=rank, shard_count=3, tile_w=16, tile_h=16)
            where = pta.local_pixel_map(prof, o)
            part = g.render_aov(prof, o)
            assert np.array_equal(bits(part), bits(whole[where])), (name, n_samples, rank)
            if n_samples == 3:
                assert np.array_equal(bits(aov_on_device(pta, g, prof, o)), bits(part))
                assert np.array_equal(bits(g.render_aov_samples(prof, o)), bits(g.render_aov_samples(prof)[:, where]))
            seen[where] = True
        assert seen.all()


def test_culled_blocks_have_no_coverage_and_set_camera_is_followed(pta, scene_cache):
    hs = scene_cache("cube")
    cam = pta.make_camera(hs.camera)
    for k in range(3):
        cam.transform[12 + k] += f32(8.0) * cam.transform[8 + k]
    g = pta.GpuScene(hs)
    prof = pta.Profile.make(40, 24, 3, 0)
    near = g.render_aov(prof)
    g.set_camera(cam)
    g.render(prof)
    blocks, n_empty = g.cull_stats()
    assert blocks > 0 and 0 < n_empty < blocks, (blocks, n_empty)
    far = g.render_aov(prof)
    fresh_host = pta.HostScene.load_isf(SCENES / "cube" / "scene.isf")
    fresh_host.set_camera(cam)
    fresh = pta.GpuScene(fresh_host)
    assert np.array_equal(bits(far), bits(fresh.render_aov(prof))) and not np.array_equal(bits(far), bits(near))
    assert np.array_equal(bits(far), bits(fresh.render_aov(prof, pta.Opts.make(flags=pta.PT_FLAG_NO_GRIDS))))
    # bounce 0, no lights to speak of in the check: a pixel whose samples all missed has the background's radiance
    rad = fresh.render_samples(prof)
    bg = np.array(list(hs.desc.contents.background), f32)
    missed = far[:, 7] == 0
    # (the cull counts the 8 x 8 blocks of whole 32 x 32 tiles: those outside the 5 x 3 blocks of the image are empty too)
    in_image = (prof.width // 8) * (prof.height // 8)
    assert n_empty > blocks - in_image and missed.sum() >= 64 * (n_empty - (blocks - in_image)) and (far[:, 7] > 0).any()
    assert (rad[:, missed] == bg).all()
    assert (bits(far[missed][:, [k for k in range(16) if k != 14]]) == 0).all() and (prim_of(far)[missed] == -1).all()
    g.close()
    fresh.close()


# ------------------------------------------------------------------------------------------------ 6. the scene is left alone
def cache_state(g):
    return (g.rng_cache_stats(), g.hit_cache_stats(), g.vis_cache_stats(), g.hit1_cache_stats(), g.cull_stats(),
            g.info().as_dict())


def test_the_aov_pass_leaves_the_scene_alone(pta):
    case = sb.case_by_name("metalness-point")     # opaque, a point light: the fused pipeline with every frame cache
    g = pta.GpuScene(sb.build(case, pta=pta))
    prof = sb.profile(case, 64, 48, 4, bounces=3)
    first = g.render(prof)
    second = g.render(prof)
    assert g.info().frame_planned
    before = cache_state(g)
    aov = g.render_aov(prof)
    assert cache_state(g) == before, "frame plan, caches and their statistics are untouched"
    third = g.render(prof)
    assert g.info().frame_planned
    for a, b in zip(first + second, third + third):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    assert np.array_equal(bits(g.render_aov(prof)), bits(aov))
    g.close()


# ------------------------------------------------------------------------------------------------ 7. the composition
@pytest.mark.parametrize("name,w,h", [("cube", 64, 48), ("alpha_transparency", 33, 17)])
def test_render_denoised_aov_equals_its_steps(pta, gpu_scene_cache, name, w, h):
    g = gpu_scene_cache(name)
    n_samples = 4
    prof = pta.Profile.make(w, h, n_samples, 2, "ACES")
    raw_rgb, accum, moments = g.render_moments(prof)
    aov = g.render_aov(prof)
    guides = pta.aov_guides(n_samples, aov)
    assert np.array_equal(bits(guides), bits(am.guides_of(aov, n_samples)))
    centre = g.render_guides(w, h)
    plain = pta.DenoiseParams.default(iterations=3, tonemap="ACES")
    rgb, col = g.render_denoised_aov(prof, plain)
    want_col, want_rgb = pta.denoise(w, h, n_samples, plain, accum, guides)
    assert np.array_equal(bits(col), bits(want_col)) and np.array_equal(rgb, want_rgb)
    assert not np.array_equal(bits(col), bits(pta.denoise(w, h, n_samples, plain, accum, centre)[0])), "other guides, another image"
    var = pta.DenoiseParams.default_var(iterations=3, tonemap="ACES")
    rgb, col = g.render_denoised_aov(prof, var, variance=True)
    want_col, want_rgb = pta.denoise_var(w, h, n_samples, var, accum, moments, guides)
    assert np.array_equal(bits(col), bits(want_col)) and np.array_equal(rgb, want_rgb)
    rgb, col = g.render_denoised_aov(prof, pta.DenoiseParams.default(iterations=0, tonemap="ACES"))
    assert np.array_equal(rgb, raw_rgb) and np.array_equal(bits(col), bits(accum / f32(n_samples)))
    # first-entry guides through the same entry point
    rgb, col = g.render_denoised_aov(prof, plain, aov_flags=pta.PT_AOV_FIRST_ENTRY)
    want_col, want_rgb = pta.denoise(w, h, n_samples, plain, accum, pta.aov_guides(n_samples, g.render_aov(prof, aov_flags=pta.PT_AOV_FIRST_ENTRY)))
    assert np.array_equal(bits(col), bits(want_col)) and np.array_equal(rgb, want_rgb)


# ------------------------------------------------------------------------------------------------ 8. the refusals
def test_refusals_leave_the_outputs_and_the_next_frame_alone(pta, gpu_scene_cache):
    g = gpu_scene_cache("cube")
    lib = pta.gpu_lib()
    w, h = 33, 17
    prof = pta.Profile.make(w, h, 2, 2)
    before = g.render(prof)
    aov_before = g.render_aov(prof)
    out = np.full((2, w * h, 16), -7.0, f32)
    guides = np.full((w * h, 8), -7.0, f32)
    rgb, col = np.full((w * h, 3), 7, np.uint8), np.full((w * h, 3), -7.0, f32)
    p, o, dn = C.byref(prof), None, C.byref(pta.DenoiseParams.default())
    zero = C.byref(pta.Profile.make(w, h, 0, 2))
    idle = C.byref(pta.Opts.make(shard_rank=5, shard_count=6, tile_w=32, tile_h=32))   # 2 tiles, 6 ranks: rank 5 has no pixels
    big = C.byref(pta.Profile.make(2048, 2048, 2, 2))                                   # 2 x 4 Mi x 64 B = 512 MiB
    INV = pta.PT_ERR_INVALID
    for fn in (lib.pt_render_aov, lib.pt_render_aov_samples):
        assert fn(None, p, o, 0, out.ctypes.data) == INV
        assert fn(g.handle, None, o, 0, out.ctypes.data) == INV
        assert fn(g.handle, p, o, 0, None) == INV
        assert fn(g.handle, zero, o, 0, out.ctypes.data) == INV
        assert fn(g.handle, p, o, 4, out.ctypes.data) == INV
        assert fn(g.handle, p, idle, 0, out.ctypes.data) == INV
        assert lib.pt_last_error()
    assert lib.pt_render_aov_samples(g.handle, big, o, 0, out.ctypes.data) == INV
    assert lib.pt_render_aov_device(g.handle, p, o, 0, None, None) == INV
    assert lib.pt_render_aov_device(g.handle, p, o, 8, 16, None) == INV
    assert lib.pt_render_aov_device(g.handle, p, o, 0, 24, None) == INV, "16-byte alignment"
    a = out[0].ctypes.data
    assert lib.pt_aov_guides(0, w * h, 2, None, guides.ctypes.data) == INV
    assert lib.pt_aov_guides(0, w * h, 2, a, None) == INV
    assert lib.pt_aov_guides(0, 0, 2, a, guides.ctypes.data) == INV
    assert lib.pt_aov_guides(0, w * h, 0, a, guides.ctypes.data) == INV
    assert lib.pt_aov_guides_device(0, w * h, 2, None, None, None) == INV
    assert lib.pt_aov_guides_device(0, w * h, 2, 8, 16, None) == INV
    r, c = rgb.ctypes.data, col.ctypes.data
    assert lib.pt_render_denoised_aov(None, p, o, dn, 0, 0, r, c) == INV
    assert lib.pt_render_denoised_aov(g.handle, None, o, dn, 0, 0, r, c) == INV
    assert lib.pt_render_denoised_aov(g.handle, p, o, None, 0, 0, r, c) == INV
    assert lib.pt_render_denoised_aov(g.handle, zero, o, dn, 0, 0, r, c) == INV
    assert lib.pt_render_denoised_aov(g.handle, p, o, dn, 0, 4, r, c) == INV
    assert lib.pt_render_denoised_aov(g.handle, p, o, C.byref(pta.DenoiseParams.default(iterations=9)), 0, 0, r, c) == INV
    one = C.byref(pta.Profile.make(w, h, 1, 2))
    assert lib.pt_render_denoised_aov(g.handle, one, o, dn, 1, 0, r, c) == INV, "a sample variance needs two samples"
    shards = C.byref(pta.Opts.make(shard_rank=0, shard_count=2, tile_w=16, tile_h=16))
    assert lib.pt_render_denoised_aov(g.handle, p, shards, dn, 0, 0, r, c) == pta.PT_ERR_UNSUPPORTED
    assert (out == f32(-7.0)).all() and (guides == f32(-7.0)).all() and (rgb == 7).all() and (col == f32(-7.0)).all()
    after = g.render(prof)
    assert np.array_equal(after[0], before[0]) and np.array_equal(bits(after[1]), bits(before[1]))
    assert np.array_equal(bits(g.render_aov(prof)), bits(aov_before))
