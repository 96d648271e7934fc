"""Denoised previews on the GPU: the a-trous kernels against tests/denoise_model.py bit for bit, the guide planes against
pt_debug_render and pt_trace_rays, pt_render_denoised against its three steps, the CLI flags."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import denoise_model as dm
import scene_builder as sb
from conftest import ROOT, SCENES

f32 = np.float32
EXE = ROOT / "path-tracer_amd" / "path-tracer"
GOLDEN_SCENES = ("alpha_transparency", "cube", "head", "reflection", "spheres", "white_furnace_direct", "white_furnace_indirect")
BUILT = ("all-point", "none-point_dir")   # scene_builder cases: every texture kind (a normal map among them); none
SIZES = ((1, 1), (2, 3), (5, 4), (17, 9), (64, 48), (70, 33), (130, 67))
ITERATIONS = (0, 1, 3, 5, 8)


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def as_u8(v):
    """Rust's `v as u8` for float32: saturating, NaN -> 0."""
    v = np.asarray(v, f32)
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(v) | (v <= 0), 0, np.where(v >= 255, 255, np.trunc(np.nan_to_num(v)))).astype(np.uint8)


def denoise_on_device(pta, w, h, samples, params, accum, guides):
    """pt_denoise_device on torch tensors and torch's current stream."""
    import torch
    n = w * h
    d_acc, d_g = torch.from_numpy(np.ascontiguousarray(accum)).cuda(), torch.from_numpy(np.ascontiguousarray(guides)).cuda()
    d_col = torch.empty((n, 3), dtype=torch.float32, device="cuda")
    d_rgb = torch.empty((n, 3), dtype=torch.uint8, device="cuda")
    d_scratch = torch.empty(max(1, pta.denoise_scratch_bytes(w, h)), dtype=torch.uint8, device="cuda")
    assert d_scratch.data_ptr() % 256 == 0 and d_g.data_ptr() % 16 == 0
    pta.check_gpu(pta.gpu_lib().pt_denoise_device(0, w, h, samples, C.byref(params), d_acc.data_ptr(), d_g.data_ptr(),
                                                  d_col.data_ptr(), d_rgb.data_ptr(), d_scratch.data_ptr(),
                                                  torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return d_col.cpu().numpy(), d_rgb.cpu().numpy()


# ------------------------------------------------------------------------------------------------ the filter
@pytest.mark.gpu
@pytest.mark.parametrize("w,h", SIZES)
def test_filter_equals_the_model_bit_for_bit(pta, oracle, w, h):
    samples, accum, guides = dm.synthetic_inputs(w, h, 100 + w)
    combos = [(it, fl, sc) for it in ITERATIONS for fl in (0, pta.PT_DENOISE_NO_DEMODULATE) for sc in (0.0, 0.75)]
    for k, (it, fl, sc) in enumerate(combos):
        params = pta.DenoiseParams.default(iterations=it, flags=fl, sigma_color=sc, sigma_depth=(0.5, 2.0)[k % 2],
                                           normal_power_log2=(0, 3, 10)[k % 3], tonemap=k % 3)
        want = dm.denoise_with(params, w, h, samples, accum, guides)
        want_rgb = oracle.post_process(pta.Profile.make(w, h, 1, 1, int(params.tonemap)), want)
        for form, (col, rgb) in (("host", pta.denoise(w, h, samples, params, accum, guides)),
                                 ("device", denoise_on_device(pta, w, h, samples, params, accum, guides))):
            same = (bits(col) == bits(want)) | (np.isnan(col) & np.isnan(want))
            assert same.all(), (form, w, h, it, fl, sc, int((~same).any(axis=1).sum()), np.argwhere(~same)[0].tolist())
            assert np.array_equal(rgb, want_rgb), (form, w, h, it, fl, sc)


@pytest.mark.gpu
def test_lds_tile_passes_give_the_same_bits(pta, monkeypatch):
    """Steps 1 and 2 gather from an LDS tile with a halo, PT_DN_LDS=0 sends them through global memory like the later
    steps: the same bits, for images smaller than a tile, not a multiple of it, and of several tiles."""
    for w, h in ((5, 4), (70, 33), (130, 67)):
        samples, accum, guides = dm.synthetic_inputs(w, h, 7)
        params = pta.DenoiseParams.default(iterations=3, sigma_color=0.75, sigma_depth=1.0, normal_power_log2=3)
        monkeypatch.setenv("PT_DN_LDS", "0")
        plain, _ = pta.denoise(w, h, samples, params, accum, guides)
        monkeypatch.delenv("PT_DN_LDS")
        tiled, _ = pta.denoise(w, h, samples, params, accum, guides)
        assert np.array_equal(bits(tiled), bits(plain)), (w, h)
        assert np.array_equal(bits(plain), bits(dm.denoise_with(params, w, h, samples, accum, guides))), (w, h)


# ------------------------------------------------------------------------------------------------ the guides
def guide_scenes(pta, scene_cache):
    for name in GOLDEN_SCENES:
        yield name, scene_cache(name), scene_cache(name).camera
    for name in BUILT:
        scene = sb.build(sb.case_by_name(name))
        yield name, scene, scene.desc.contents.camera


def check_guides(pta, g, camera, w, h, name):
    guides = g.render_guides(w, h)
    assert guides.shape == (w * h, pta.PT_GUIDE_FLOATS)
    prim = guides[:, 7].view(np.int32)
    planes = g.debug_render(w, h)
    if not planes:
        assert (prim == -1).all(), name
        planes = {k: np.zeros((w * h, 3), np.uint8) for k in pta.DEBUG_PLANES}
    n = guides[:, 0:3]
    hit = prim >= 0
    assert np.array_equal(np.where(hit[:, None], as_u8((n * f32(0.5) + f32(0.5)) * f32(255.0)), 0), planes["normal"]), name
    assert np.array_equal(np.where(hit[:, None], as_u8(guides[:, 4:7] * f32(255.0)), 0), planes["albedo"]), name
    lit = np.zeros(w * h, bool)
    for k in pta.DEBUG_PLANES:
        lit |= planes[k].any(axis=1)
    assert np.array_equal(lit, hit), (name, "debug planes are zero exactly where no primitive was hit")
    miss = guides[~hit]
    assert (bits(miss[:, 0:3]) == 0).all() and (miss[:, 3] == -1).all() and (bits(miss[:, 4:7]) == 0).all() and (prim[~hit] == -1).all()
    hits = g.trace(dm.primary_rays(camera, w, h))
    assert np.array_equal(hits["prim"], prim), name
    assert np.array_equal(bits(hits["dist"][hit]), bits(guides[hit, 3])), name
    return guides


@pytest.mark.gpu
def test_guides_are_the_debug_pass_at_float_precision(pta, scene_cache):
    for name, scene, camera in guide_scenes(pta, scene_cache):
        g = pta.GpuScene(scene)
        for w, h in ((64, 48), (33, 17)):
            check_guides(pta, g, camera, w, h, name)
        g.close()


@pytest.mark.gpu
def test_guides_follow_set_camera(pta, scene_cache):
    hs = scene_cache("cube")
    cam = pta.make_camera(hs.camera)
    cam.transform[12] += 0.75
    cam.transform[13] -= 0.5
    cam.fov *= 0.8
    g = pta.GpuScene(hs)
    before = g.render_guides(64, 48)
    g.set_camera(cam)
    moved = check_guides(pta, g, cam, 64, 48, "cube, moved camera")
    fresh_host = pta.HostScene.load_isf(SCENES / "cube" / "scene.isf")
    fresh_host.set_camera(cam)
    fresh = pta.GpuScene(fresh_host)
    assert np.array_equal(bits(moved), bits(fresh.render_guides(64, 48)))
    assert not np.array_equal(bits(moved), bits(before))
    g.close()
    fresh.close()


# ------------------------------------------------------------------------------------------------ pt_render_denoised
@pytest.mark.gpu
@pytest.mark.parametrize("name,w,h", [("cube", 64, 48), ("head", 70, 33)])
def test_render_denoised_equals_its_three_steps(pta, gpu_scene_cache, name, w, h):
    g = gpu_scene_cache(name)
    prof = pta.Profile.make(w, h, 4, 3, "ACES")
    raw_rgb, accum = g.render(prof)
    guides = g.render_guides(w, h)
    for params in (pta.DenoiseParams.default(tonemap="ACES"),
                   pta.DenoiseParams.default(iterations=4, sigma_color=1.0, flags=pta.PT_DENOISE_NO_DEMODULATE, tonemap="ACES")):
        rgb, col = g.render_denoised(prof, params)
        want_col, want_rgb = pta.denoise(w, h, 4, params, accum, guides)
        assert np.array_equal(bits(col), bits(want_col)) and np.array_equal(rgb, want_rgb)
        assert not np.array_equal(bits(col), bits(accum / f32(4)))
    rgb, col = g.render_denoised(prof, pta.DenoiseParams.default(iterations=0, tonemap="ACES"))
    assert np.array_equal(rgb, raw_rgb) and np.array_equal(bits(col), bits(accum / f32(4)))


@pytest.mark.gpu
def test_render_denoised_rejects_shards_and_bad_arguments(pta, gpu_scene_cache):
    g = gpu_scene_cache("cube")
    lib = pta.gpu_lib()
    w, h = 33, 17
    prof = pta.Profile.make(w, h, 2, 2)
    good = pta.DenoiseParams.default()
    before = g.render(prof)
    rgb, col = np.empty((w * h, 3), np.uint8), np.empty((w * h, 3), f32)
    with pytest.raises(pta.PtError) as e:
        g.render_denoised(prof, good, pta.Opts.make(shard_rank=0, shard_count=2, tile_w=16, tile_h=16))
    assert e.value.code == pta.PT_ERR_UNSUPPORTED
    bad = [dict(iterations=9), dict(flags=2), dict(normal_power_log2=11), dict(tonemap=3), dict(tonemap=-1),
           dict(sigma_depth=0.0), dict(sigma_depth=-1.0), dict(sigma_depth=float("inf")), dict(sigma_depth=float("nan")),
           dict(sigma_color=-0.5), dict(sigma_color=float("inf")), dict(sigma_color=float("nan"))]
    samples, accum, guides = dm.synthetic_inputs(w, h, 3)
    for change in bad:
        p = pta.DenoiseParams.default(**change)
        assert lib.pt_render_denoised(g.handle, C.byref(prof), None, C.byref(p), rgb.ctypes.data, col.ctypes.data) == pta.PT_ERR_INVALID, change
        assert lib.pt_denoise(0, w, h, samples, C.byref(p), accum.ctypes.data, guides.ctypes.data, col.ctypes.data, rgb.ctypes.data) == pta.PT_ERR_INVALID, change
        assert lib.pt_last_error()
    gp, a, gd = C.byref(good), accum.ctypes.data, guides.ctypes.data
    assert lib.pt_render_denoised(None, C.byref(prof), None, gp, rgb.ctypes.data, None) == pta.PT_ERR_INVALID
    assert lib.pt_render_denoised(g.handle, None, None, gp, rgb.ctypes.data, None) == pta.PT_ERR_INVALID
    assert lib.pt_render_denoised(g.handle, C.byref(prof), None, None, rgb.ctypes.data, None) == pta.PT_ERR_INVALID
    assert lib.pt_render_denoised(g.handle, C.byref(pta.Profile.make(w, h, 0, 2)), None, gp, rgb.ctypes.data, None) == pta.PT_ERR_INVALID
    assert lib.pt_render_denoised(g.handle, C.byref(pta.Profile.make(0, h, 2, 2)), None, gp, rgb.ctypes.data, None) == pta.PT_ERR_INVALID
    assert lib.pt_denoise(0, w, h, samples, None, a, gd, col.ctypes.data, None) == pta.PT_ERR_INVALID
    assert lib.pt_denoise(0, w, h, samples, gp, None, gd, col.ctypes.data, None) == pta.PT_ERR_INVALID
    assert lib.pt_denoise(0, w, h, samples, gp, a, None, col.ctypes.data, None) == pta.PT_ERR_INVALID
    assert lib.pt_denoise(0, 0, h, samples, gp, a, gd, col.ctypes.data, None) == pta.PT_ERR_INVALID
    assert lib.pt_denoise(0, w, 0, samples, gp, a, gd, col.ctypes.data, None) == pta.PT_ERR_INVALID
    assert lib.pt_denoise(0, w, h, 0, gp, a, gd, col.ctypes.data, None) == pta.PT_ERR_INVALID
    assert lib.pt_denoise_device(0, w, h, samples, gp, None, None, None, None, None, None) == pta.PT_ERR_INVALID
    assert lib.pt_render_guides(None, w, h, gd) == pta.PT_ERR_INVALID
    assert lib.pt_render_guides(g.handle, w, h, None) == pta.PT_ERR_INVALID
    assert lib.pt_render_guides(g.handle, 0, h, gd) == pta.PT_ERR_INVALID
    assert lib.pt_render_guides_device(g.handle, w, h, None, None) == pta.PT_ERR_INVALID
    assert pta.denoise_scratch_bytes(0, 5) == 0 and pta.denoise_scratch_bytes(w, h) >= 68 * w * h
    # both outputs are optional
    assert lib.pt_denoise(0, w, h, samples, gp, a, gd, None, None) == pta.PT_OK
    after = g.render(prof)
    assert np.array_equal(after[0], before[0]) and np.array_equal(bits(after[1]), bits(before[1]))


# ------------------------------------------------------------------------------------------------ CLI and ABI
@pytest.mark.gpu
def test_cli_denoise_writes_the_filtered_frame(tmp_path, pta, gpu_scene_cache):
    from PIL import Image
    prof = tmp_path / "p.yml"
    prof.write_text("resolution: {width: 64, height: 48}\nsamples: 4\nbounces: 2\n")
    scene = str(SCENES / "cube" / "scene.isf")
    g = gpu_scene_cache("cube")
    p = pta.Profile.make(64, 48, 4, 2)
    for extra, params in (((), pta.DenoiseParams.default()), (("--denoise-iterations", "3"), pta.DenoiseParams.default(iterations=3))):
        out = tmp_path / f"d{len(extra)}.png"
        r = subprocess.run([str(EXE), "render", scene, "-q", "-p", str(prof), "-o", str(out), "--denoise", *extra],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        want, _ = g.render_denoised(p, params)
        assert np.array_equal(np.asarray(Image.open(out)).reshape(-1, 3), want), extra
    assert not np.array_equal(want, g.render(p)[0])
    out = tmp_path / "two.png"
    r = subprocess.run([str(EXE), "render", scene, "-q", "-p", str(prof), "-o", str(out), "--devices", "0,0", "--denoise"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--denoise" in r.stderr and not out.exists()


def test_cli_help_lists_the_denoise_flags_and_rejects_bad_values():
    r = subprocess.run([str(EXE), "render", "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--denoise " in r.stdout and "--denoise-iterations <N>" in r.stdout
    for args in (("--denoise", "--denoise-iterations", "9"), ("--denoise", "--denoise-iterations", "x"), ("--denoise-iterations", "2"),
                 ("--denoise", "--devices", "0,1")):
        r = subprocess.run([str(EXE), "render", str(SCENES / "cube" / "scene.isf"), "-q", *args], capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and "denoise" in r.stderr, args


def test_denoise_params_size_matches_the_header(pta, tmp_path):
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "ptgpu.h"
int main(){ printf("%zu %zu %zu %d %d %d\n", sizeof(pt_denoise_params), offsetof(pt_denoise_params, tonemap),
  offsetof(pt_denoise_params, sigma_depth), (int)PT_GUIDE_FLOATS, (int)PT_DENOISE_NO_DEMODULATE, (int)PT_DENOISE_STAGES); return 0; }'''
    exe = tmp_path / "dn_sizes"
    subprocess.run(["gcc", "-x", "c", "-", "-I", str(ROOT / "include"), "-o", str(exe)], input=src.encode(), check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, check=True).stdout.split()]
    assert got == [C.sizeof(pta.DenoiseParams), pta.DenoiseParams.tonemap.offset, pta.DenoiseParams.sigma_depth.offset,
                   pta.PT_GUIDE_FLOATS, pta.PT_DENOISE_NO_DEMODULATE, pta.PT_DENOISE_STAGES]
