"""pt_render_samples and pt_render_moments on the GPU: the sample planes against the oracle's partial sums, the moments against
the numpy restatement over those planes (tests/denoise_var_model.py), both bit for bit; batches, shards, flags, the cull
branch of k_accumulate_moments and the frame plan."""
import ctypes as C

import numpy as np
import pytest

import denoise_var_model as dvm
from conftest import SCENES

pytestmark = pytest.mark.gpu
f32 = np.float32
SAMPLES, BOUNCES = 4, 4
CASES = {"cube": (40, 24), "head": (33, 20)}   # head: translucent (the ALPHA kernels)


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


@pytest.fixture(scope="module")
def frames(pta, oracle, scene_cache, gpu_scene_cache):
    """Per scene: the profile, the sample planes, the frame of render() and the restated moments - computed once."""
    out = {}
    for name, (w, h) in CASES.items():
        g = gpu_scene_cache(name)
        prof = pta.Profile.make(w, h, SAMPLES, BOUNCES)
        planes = g.render_samples(prof)
        rgb, acc = g.render(prof)
        want_acc, want_mom = dvm.moments_of(planes)
        for a in (planes, rgb, acc, want_acc, want_mom):
            a.setflags(write=False)
        out[name] = dict(g=g, prof=prof, planes=planes, rgb=rgb, acc=acc, want_acc=want_acc, want_mom=want_mom)
    return out


@pytest.mark.parametrize("name", CASES)
def test_running_sums_of_the_sample_planes_are_the_oracles_partial_frames(pta, oracle, scene_cache, frames, name):
    fr = frames[name]
    assert fr["planes"].shape == (SAMPLES, fr["prof"].width * fr["prof"].height, 3)
    osc = oracle.OracleScene(scene_cache(name).desc, oracle.PTO_BVH)
    run = np.zeros_like(fr["planes"][0])
    for k in range(1, SAMPLES + 1):
        run = run + fr["planes"][k - 1]
        _, want, _ = osc.render(fr["prof"], sample_count=k)
        assert np.array_equal(bits(run), bits(want)), (name, k)


@pytest.mark.parametrize("name", CASES)
def test_moments_equal_the_restatement_and_the_frame_is_renders(frames, name):
    fr = frames[name]
    rgb, acc, mom = fr["g"].render_moments(fr["prof"])
    assert mom.shape == (len(acc), 2)
    assert np.array_equal(bits(mom), bits(fr["want_mom"]))
    assert np.array_equal(bits(acc), bits(fr["acc"])) and np.array_equal(rgb, fr["rgb"])
    assert np.array_equal(bits(fr["want_acc"]), bits(fr["acc"]))
    # the samples of a pixel differ somewhere: the second moment says more than the first
    N = f32(SAMPLES)
    assert (mom[:, 1] > (mom[:, 0] * mom[:, 0]) / N * f32(1.001)).any()


@pytest.mark.parametrize("name", CASES)
def test_sample_batches_give_the_same_bits(pta, frames, name):
    fr = frames[name]
    for batch in (1, 3, 0):
        opts = pta.Opts.make(sample_batch=batch)
        rgb, acc, mom = fr["g"].render_moments(fr["prof"], opts)
        assert np.array_equal(bits(mom), bits(fr["want_mom"])), batch
        assert np.array_equal(bits(acc), bits(fr["acc"])) and np.array_equal(rgb, fr["rgb"]), batch
        assert np.array_equal(bits(fr["g"].render_samples(fr["prof"], opts)), bits(fr["planes"])), batch


@pytest.mark.parametrize("tile_w,tile_h", [(16, 16), (8, 32), (32, 8)])
@pytest.mark.parametrize("name", CASES)
def test_three_shards_equal_the_unsharded_planes(pta, frames, name, tile_w, tile_h):
    """The smallest tiles pt_opts accepts (sides multiples of 8, tile_w * tile_h a multiple of 256; 8 x 8 is PT_ERR_INVALID):
    several tiles per rank, tiles clipped at the right and bottom borders."""
    fr = frames[name]
    n = fr["prof"].width * fr["prof"].height
    mom_all, acc_all = np.full((n, 2), np.nan, f32), np.full((n, 3), np.nan, f32)
    planes_all = np.full((SAMPLES, n, 3), np.nan, f32)
    for rank in range(3):
        opts = pta.Opts.make(shard_rank=rank, shard_count=3, tile_w=tile_w, tile_h=tile_h)
        where = pta.local_pixel_map(fr["prof"], opts)
        rgb, acc, mom = fr["g"].render_moments(fr["prof"], opts)
        assert len(mom) == len(where)
        mom_all[where], acc_all[where] = mom, acc
        assert np.array_equal(rgb, fr["rgb"][where])
        planes_all[:, where] = fr["g"].render_samples(fr["prof"], opts)
    assert np.array_equal(bits(mom_all), bits(fr["want_mom"]))
    assert np.array_equal(bits(acc_all), bits(fr["acc"]))
    assert np.array_equal(bits(planes_all), bits(fr["planes"]))


@pytest.mark.parametrize("name", CASES)
def test_no_grids_gives_the_same_bits_and_the_megakernel_is_unsupported(pta, frames, name):
    fr = frames[name]
    g, prof = fr["g"], fr["prof"]
    rgb, acc, mom = g.render_moments(prof, pta.Opts.make(flags=pta.PT_FLAG_NO_GRIDS))
    assert np.array_equal(bits(mom), bits(fr["want_mom"])) and np.array_equal(bits(acc), bits(fr["acc"])) and np.array_equal(rgb, fr["rgb"])
    assert np.array_equal(bits(g.render_samples(prof, pta.Opts.make(flags=pta.PT_FLAG_NO_GRIDS))), bits(fr["planes"]))
    mega = pta.Opts.make(flags=pta.PT_FLAG_MEGAKERNEL)
    for call in (lambda: g.render_moments(prof, mega), lambda: g.render_samples(prof, mega),
                 lambda: g.render_denoised_var(prof, pta.DenoiseParams.default_var(), mega)):
        with pytest.raises(pta.PtError) as e:
            call()
        assert e.value.code == pta.PT_ERR_UNSUPPORTED
    rgb2, acc2 = g.render(prof)
    assert np.array_equal(rgb2, fr["rgb"]) and np.array_equal(bits(acc2), bits(fr["acc"]))


def test_argument_errors_leave_the_scene_alone(pta, frames):
    fr = frames["cube"]
    g, prof, lib = fr["g"], fr["prof"], pta.gpu_lib()
    n = prof.width * prof.height
    mom, acc = np.empty((n, 2), f32), np.empty((n, 3), f32)
    assert lib.pt_render_moments(g.handle, C.byref(prof), None, None, acc.ctypes.data, None) == pta.PT_ERR_INVALID
    assert lib.pt_render_moments(None, C.byref(prof), None, None, None, mom.ctypes.data) == pta.PT_ERR_INVALID
    assert lib.pt_render_moments(g.handle, None, None, None, None, mom.ctypes.data) == pta.PT_ERR_INVALID
    assert lib.pt_render_moments_device(g.handle, C.byref(prof), None, None, None, None, None) == pta.PT_ERR_INVALID
    assert lib.pt_render_samples(g.handle, C.byref(prof), None, None) == pta.PT_ERR_INVALID
    # 1024 x 1024 x 12 B = 12 MiB per plane: 22 planes exceed 256 MiB, 21 do not (not rendered here)
    big = pta.Profile.make(1024, 1024, 22, 1)
    assert lib.pt_render_samples(g.handle, C.byref(big), None, mom.ctypes.data) == pta.PT_ERR_INVALID
    assert "256 MiB" in lib.pt_last_error().decode()
    # rgb8 and accum are optional
    assert lib.pt_render_moments(g.handle, C.byref(prof), None, None, None, mom.ctypes.data) == pta.PT_OK
    assert np.array_equal(bits(mom), bits(fr["want_mom"]))
    rgb2, acc2 = g.render(prof)
    assert np.array_equal(rgb2, fr["rgb"]) and np.array_equal(bits(acc2), bits(fr["acc"]))


def test_device_entry_point_on_torch_tensors(pta, frames):
    import torch
    fr = frames["head"]
    n = fr["prof"].width * fr["prof"].height
    d_rgb = torch.empty((n, 3), dtype=torch.uint8, device="cuda")
    d_acc = torch.empty((n, 3), dtype=torch.float32, device="cuda")
    d_mom = torch.full((n, 2), float("nan"), dtype=torch.float32, device="cuda")
    fr["g"].render_moments_device(fr["prof"], pta.Opts.make(sample_batch=3), d_rgb.data_ptr(), d_acc.data_ptr(), d_mom.data_ptr(),
                                  torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert np.array_equal(bits(d_mom.cpu().numpy()), bits(fr["want_mom"]))
    assert np.array_equal(bits(d_acc.cpu().numpy()), bits(fr["acc"])) and np.array_equal(d_rgb.cpu().numpy(), fr["rgb"])


def test_culled_blocks_take_the_background_once_per_sample(pta, oracle):
    """The camera pulled back until whole 8x8 blocks see nothing: k_accumulate_moments' cull branch (and the fill of
    pt_render_samples), against the oracle and the restatement."""
    host = pta.HostScene.load_isf(SCENES / "cube" / "scene.isf")
    cam = pta.make_camera(host.camera)
    for k in range(3):   # away from the scene along the camera's own z axis (it looks down -z)
        cam.transform[12 + k] += f32(8.0) * cam.transform[8 + k]
    host.set_camera(cam)
    g = pta.GpuScene(pta.HostScene.load_isf(SCENES / "cube" / "scene.isf"))
    g.set_camera(cam)
    prof = pta.Profile.make(40, 24, SAMPLES, BOUNCES)
    for batch in (0, 3):
        opts = pta.Opts.make(sample_batch=batch)
        rgb, acc, mom = g.render_moments(prof, opts)
        blocks, empty = g.cull_stats()
        assert blocks > 0 and 0 < empty < blocks, (blocks, empty)
        planes = g.render_samples(prof, opts)
        assert 0 < g.cull_stats()[1] < blocks
        want_acc, want_mom = dvm.moments_of(planes)
        assert np.array_equal(bits(mom), bits(want_mom)) and np.array_equal(bits(acc), bits(want_acc)), batch
        _, o_acc, _ = oracle.OracleScene(host.desc, oracle.PTO_BVH).render(prof)
        assert np.array_equal(bits(acc), bits(o_acc)), batch
        rgb2, acc2 = g.render(prof, opts)
        assert np.array_equal(rgb2, rgb) and np.array_equal(bits(acc2), bits(acc)), batch
    # the object is still in the picture: some pixel's samples differ
    assert (mom[:, 1] > (mom[:, 0] * mom[:, 0]) / f32(SAMPLES) * f32(1.001)).any()
    g.close()


def test_a_moments_frame_leaves_the_frame_plan_valid(pta, scene_cache):
    g = pta.GpuScene(scene_cache("cube"))
    prof = pta.Profile.make(40, 24, SAMPLES, BOUNCES)
    first = g.render(prof)
    for _ in range(2):
        g.render(prof)
    assert g.info().frame_planned == 1
    planes = g.render_samples(prof)
    rgb, acc, mom = g.render_moments(prof)
    assert g.info().frame_planned == 1
    assert np.array_equal(bits(mom), bits(dvm.moments_of(planes)[1]))
    assert np.array_equal(rgb, first[0]) and np.array_equal(bits(acc), bits(first[1]))
    after = g.render(prof)
    assert g.info().frame_planned == 1
    assert np.array_equal(after[0], first[0]) and np.array_equal(bits(after[1]), bits(first[1]))
    g.close()
