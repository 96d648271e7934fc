"""The variance-guided a-trous filter on the GPU: k_dnv_prep / k_dnv_pass against tests/denoise_var_model.py bit for bit,
pt_render_denoised_var against its three steps, argument errors, the CLI flag and the ABI."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import denoise_model as dm
import denoise_var_model as dvm
from conftest import ROOT, SCENES

f32 = np.float32
EXE = ROOT / "path-tracer_amd" / "path-tracer"
SIZES = ((1, 1), (2, 3), (5, 4), (33, 9), (64, 48), (70, 33), (130, 67))
ITERATIONS = (0, 1, 3, 5)
NEW_SYMBOLS = ("pt_render_moments", "pt_render_moments_device", "pt_render_samples", "pt_denoise_var_params_default",
               "pt_denoise_var_scratch_bytes", "pt_denoise_var", "pt_denoise_var_device", "pt_render_denoised_var",
               "pt_denoise_var_stage_times")


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def denoise_var_on_device(pta, w, h, samples, params, accum, moments, guides):
    """pt_denoise_var_device on torch tensors and torch's current stream."""
    import torch
    n = w * h
    d_acc, d_mom, d_g = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (accum, moments, guides))
    d_col = torch.empty((n, 3), dtype=torch.float32, device="cuda")
    d_rgb = torch.empty((n, 3), dtype=torch.uint8, device="cuda")
    d_scratch = torch.empty(max(1, pta.denoise_var_scratch_bytes(w, h)), dtype=torch.uint8, device="cuda")
    assert d_scratch.data_ptr() % 256 == 0 and d_g.data_ptr() % 16 == 0 and d_mom.data_ptr() % 8 == 0
    pta.check_gpu(pta.gpu_lib().pt_denoise_var_device(0, w, h, samples, C.byref(params), d_acc.data_ptr(), d_mom.data_ptr(),
                                                      d_g.data_ptr(), d_col.data_ptr(), d_rgb.data_ptr(), d_scratch.data_ptr(),
                                                      torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return d_col.cpu().numpy(), d_rgb.cpu().numpy()


# ------------------------------------------------------------------------------------------------ the filter
@pytest.mark.gpu
@pytest.mark.parametrize("w,h", SIZES)
def test_filter_equals_the_model_bit_for_bit(pta, oracle, w, h):
    samples, accum, guides = dm.synthetic_inputs(w, h, 200 + w)
    moments = dvm.synthetic_moments(samples, accum, 300 + w)
    N = f32(samples)
    if w * h >= 300:   # the special populations are there: zero variance, the clamp, fireflies
        raw = moments[:, 1] / N - (moments[:, 0] / N) * (moments[:, 0] / N)
        assert (raw == 0).any() and (raw < 0).any() and (accum.max(axis=1) > 40).any()
    combos = [(it, fl) for it in ITERATIONS for fl in (0, pta.PT_DENOISE_NO_DEMODULATE)]
    for k, (it, fl) in enumerate(combos):
        params = pta.DenoiseParams.default_var(iterations=it, flags=fl, sigma_color=(4.0, 0.75, 16.0)[k % 3],
                                               sigma_depth=(0.5, 2.0)[k % 2], normal_power_log2=(0, 3, 10)[(k // 2) % 3], tonemap=k % 3)
        want = dvm.denoise_var_with(params, w, h, samples, accum, moments, guides)
        want_rgb = oracle.post_process(pta.Profile.make(w, h, 1, 1, int(params.tonemap)), want)
        for form, (col, rgb) in (("host", pta.denoise_var(w, h, samples, params, accum, moments, guides)),
                                 ("device", denoise_var_on_device(pta, w, h, samples, params, accum, moments, guides))):
            same = (bits(col) == bits(want)) | (np.isnan(col) & np.isnan(want))
            assert same.all(), (form, w, h, it, fl, int((~same).any(axis=1).sum()), np.argwhere(~same)[0].tolist())
            assert np.array_equal(rgb, want_rgb), (form, w, h, it, fl)
        if it and w * h >= 297:
            assert not np.array_equal(bits(want), bits(accum / N)), (w, h, it, fl)


@pytest.mark.gpu
def test_the_variance_steers_the_filter(pta):
    """The same frame with other moments is another picture; the plain filter's parameters mean something else here."""
    w, h = 33, 9
    samples, accum, guides = dm.synthetic_inputs(w, h, 11)
    moments = dvm.synthetic_moments(samples, accum, 12)
    params = pta.DenoiseParams.default_var()
    a, _ = pta.denoise_var(w, h, samples, params, accum, moments, guides)
    louder = moments.copy()
    louder[:, 1] *= f32(3.0)
    b, _ = pta.denoise_var(w, h, samples, params, accum, louder, guides)
    plain, _ = pta.denoise(w, h, samples, params, accum, guides)
    assert not np.array_equal(bits(a), bits(b)) and not np.array_equal(bits(a), bits(plain))


# ------------------------------------------------------------------------------------------------ pt_render_denoised_var
@pytest.mark.gpu
def test_render_denoised_var_equals_its_three_steps(pta, gpu_scene_cache):
    g = gpu_scene_cache("cube")
    w, h = 64, 48
    prof = pta.Profile.make(w, h, 4, 3, "ACES")
    raw_rgb, accum, moments = g.render_moments(prof)
    guides = g.render_guides(w, h)
    for params in (pta.DenoiseParams.default_var(tonemap="ACES"),
                   pta.DenoiseParams.default_var(iterations=4, sigma_color=2.0, flags=0, tonemap="ACES")):
        rgb, col = g.render_denoised_var(prof, params)
        want_col, want_rgb = pta.denoise_var(w, h, 4, params, accum, moments, guides)
        assert np.array_equal(bits(col), bits(want_col)) and np.array_equal(rgb, want_rgb)
        assert np.array_equal(bits(col), bits(dvm.denoise_var_with(params, w, h, 4, accum, moments, guides)))
        assert not np.array_equal(bits(col), bits(accum / f32(4)))
    rgb, col = g.render_denoised_var(prof, pta.DenoiseParams.default_var(iterations=0, tonemap="ACES"))
    assert np.array_equal(rgb, raw_rgb) and np.array_equal(bits(col), bits(accum / f32(4)))
    plain_rgb, plain_acc = g.render(prof)
    assert np.array_equal(plain_rgb, raw_rgb) and np.array_equal(bits(plain_acc), bits(accum))


@pytest.mark.gpu
def test_bad_arguments_and_shards_are_rejected_and_leave_the_scene_alone(pta, gpu_scene_cache):
    g = gpu_scene_cache("cube")
    lib = pta.gpu_lib()
    w, h = 33, 17
    prof = pta.Profile.make(w, h, 2, 2)
    good = pta.DenoiseParams.default_var()
    before = g.render(prof)
    rgb, col = np.empty((w * h, 3), np.uint8), np.empty((w * h, 3), f32)
    samples, accum, guides = dm.synthetic_inputs(w, h, 3)
    moments = dvm.synthetic_moments(samples, accum, 4)
    gp, a, m, gd = C.byref(good), accum.ctypes.data, moments.ctypes.data, guides.ctypes.data

    def unchanged():
        after = g.render(prof)
        assert np.array_equal(after[0], before[0]) and np.array_equal(bits(after[1]), bits(before[1]))

    with pytest.raises(pta.PtError) as e:
        g.render_denoised_var(prof, good, pta.Opts.make(shard_rank=0, shard_count=2, tile_w=16, tile_h=16))
    assert e.value.code == pta.PT_ERR_UNSUPPORTED
    unchanged()
    # samples = 1: no sample variance
    assert lib.pt_render_denoised_var(g.handle, C.byref(pta.Profile.make(w, h, 1, 2)), None, gp, rgb.ctypes.data, None) == pta.PT_ERR_INVALID
    assert lib.pt_render_denoised_var(g.handle, C.byref(pta.Profile.make(w, h, 0, 2)), None, gp, rgb.ctypes.data, None) == pta.PT_ERR_INVALID
    assert lib.pt_denoise_var(0, w, h, 1, gp, a, m, gd, col.ctypes.data, None) == pta.PT_ERR_INVALID
    assert lib.pt_denoise_var(0, w, h, 0, gp, a, m, gd, col.ctypes.data, None) == pta.PT_ERR_INVALID
    assert lib.pt_denoise_var_device(0, w, h, 1, gp, a, m, gd, None, None, a, None) == pta.PT_ERR_INVALID
    unchanged()
    bad = [dict(sigma_color=0.0), dict(sigma_color=-0.5), dict(sigma_color=float("inf")), dict(sigma_color=float("nan")),
           dict(iterations=9), dict(flags=2), dict(normal_power_log2=11), dict(tonemap=3), dict(sigma_depth=0.0),
           dict(sigma_depth=float("nan"))]
    for change in bad:
        p = pta.DenoiseParams.default_var(**change)
        assert lib.pt_render_denoised_var(g.handle, C.byref(prof), None, C.byref(p), rgb.ctypes.data, col.ctypes.data) == pta.PT_ERR_INVALID, change
        assert lib.pt_denoise_var(0, w, h, samples, C.byref(p), a, m, gd, col.ctypes.data, rgb.ctypes.data) == pta.PT_ERR_INVALID, change
        assert lib.pt_last_error()
    unchanged()
    assert lib.pt_render_denoised_var(None, C.byref(prof), None, gp, rgb.ctypes.data, None) == pta.PT_ERR_INVALID
    assert lib.pt_render_denoised_var(g.handle, None, None, gp, rgb.ctypes.data, None) == pta.PT_ERR_INVALID
    assert lib.pt_render_denoised_var(g.handle, C.byref(prof), None, None, rgb.ctypes.data, None) == pta.PT_ERR_INVALID
    assert lib.pt_denoise_var(0, w, h, samples, None, a, m, gd, col.ctypes.data, None) == pta.PT_ERR_INVALID
    assert lib.pt_denoise_var(0, w, h, samples, gp, None, m, gd, col.ctypes.data, None) == pta.PT_ERR_INVALID
    assert lib.pt_denoise_var(0, w, h, samples, gp, a, None, gd, col.ctypes.data, None) == pta.PT_ERR_INVALID
    assert lib.pt_denoise_var(0, w, h, samples, gp, a, m, None, col.ctypes.data, None) == pta.PT_ERR_INVALID
    assert lib.pt_denoise_var(0, 0, h, samples, gp, a, m, gd, col.ctypes.data, None) == pta.PT_ERR_INVALID
    assert lib.pt_denoise_var_device(0, w, h, samples, gp, None, None, None, None, None, None, None) == pta.PT_ERR_INVALID
    ms = (C.c_float * pta.PT_DENOISE_STAGES)()
    assert lib.pt_denoise_var_stage_times(0, w, h, samples, gp, None, None, None, None, None, None, ms) == pta.PT_ERR_INVALID
    assert pta.denoise_var_scratch_bytes(0, 5) == 0 and pta.denoise_var_scratch_bytes(w, h) >= 68 * w * h
    # both outputs are optional
    assert lib.pt_denoise_var(0, w, h, samples, gp, a, m, gd, None, None) == pta.PT_OK
    unchanged()


@pytest.mark.gpu
def test_stage_times_report_prep_passes_and_finish(pta):
    import torch
    w, h = 70, 33
    samples, accum, guides = dm.synthetic_inputs(w, h, 5)
    moments = dvm.synthetic_moments(samples, accum, 6)
    params = pta.DenoiseParams.default_var(iterations=3)
    d_acc, d_mom, d_g = (torch.from_numpy(a).cuda() for a in (accum, moments, guides))
    d_col = torch.empty((w * h, 3), dtype=torch.float32, device="cuda")
    d_scratch = torch.empty(pta.denoise_var_scratch_bytes(w, h), dtype=torch.uint8, device="cuda")
    ms = (C.c_float * pta.PT_DENOISE_STAGES)()
    pta.check_gpu(pta.gpu_lib().pt_denoise_var_stage_times(0, w, h, samples, C.byref(params), d_acc.data_ptr(), d_mom.data_ptr(),
                                                           d_g.data_ptr(), d_col.data_ptr(), None, d_scratch.data_ptr(), ms))
    t = list(ms)
    assert all(v > 0 for v in t[0:4] + [t[9]]) and all(v == 0 for v in t[4:9])
    assert np.array_equal(bits(d_col.cpu().numpy()), bits(dvm.denoise_var_with(params, w, h, samples, accum, moments, guides)))


# ------------------------------------------------------------------------------------------------ CLI and ABI
@pytest.mark.gpu
def test_cli_denoise_variance_writes_the_filtered_frame(tmp_path, pta, gpu_scene_cache):
    from PIL import Image
    prof = tmp_path / "p.yml"
    prof.write_text("resolution: {width: 64, height: 48}\nsamples: 4\nbounces: 2\n")
    scene = str(SCENES / "cube" / "scene.isf")
    g = gpu_scene_cache("cube")
    p = pta.Profile.make(64, 48, 4, 2)
    for extra, params in (((), pta.DenoiseParams.default_var()), (("--denoise-iterations", "3"), pta.DenoiseParams.default_var(iterations=3))):
        out = tmp_path / f"v{len(extra)}.png"
        r = subprocess.run([str(EXE), "render", scene, "-q", "-p", str(prof), "-o", str(out), "--denoise", "--denoise-variance", *extra],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        want, _ = g.render_denoised_var(p, params)
        assert np.array_equal(np.asarray(Image.open(out)).reshape(-1, 3), want), extra
    assert not np.array_equal(want, g.render(p)[0])
    assert not np.array_equal(want, g.render_denoised(p, pta.DenoiseParams.default(iterations=3))[0])


def test_cli_rejects_denoise_variance_without_denoise_or_with_one_sample(tmp_path):
    r = subprocess.run([str(EXE), "render", "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--denoise-variance" in r.stdout
    scene = str(SCENES / "cube" / "scene.isf")
    out = tmp_path / "o.png"
    r = subprocess.run([str(EXE), "render", scene, "-q", "-o", str(out), "--denoise-variance"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--denoise" in r.stderr and not out.exists()
    prof = tmp_path / "one.yml"
    prof.write_text("resolution: {width: 16, height: 16}\nsamples: 1\nbounces: 1\n")
    r = subprocess.run([str(EXE), "render", scene, "-q", "-p", str(prof), "-o", str(out), "--denoise", "--denoise-variance"],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "samples" in r.stderr and not out.exists()


def test_new_functions_are_declared_and_exported(pta):
    text = (ROOT / "include" / "ptgpu.h").read_text()
    lib = pta.gpu_lib()
    for name in NEW_SYMBOLS:
        assert name + "(" in text and name in pta.GPU_SYMBOLS, name
        getattr(lib, name)
    for name in ("render_moments", "render_samples", "render_denoised_var"):
        assert callable(getattr(pta.GpuScene, name))
    assert callable(pta.denoise_var) and callable(pta.denoise_var_scratch_bytes) and callable(pta.DenoiseParams.default_var)
