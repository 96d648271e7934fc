"""Window frames (pt_render_window) on the GPU: chains of windows against pt_render_moments of the whole
enumeration bit for bit, every chain boundary against the running sums of pt_render_samples' planes and the oracle's
post-processing, sample batches, shards, PT_FLAG_NO_GRIDS, the megakernel, the cull branch, tile-list windows, the device
form, every refusal with the outputs untouched, and what a chain of windows leaves behind in its scene: nothing.

pt_opts refuses 8 x 8 tiles (tile_w * tile_h must be a multiple of 256), so the smallest tiles it accepts stand in for them:
8 x 32 for the shards (five tiles, the last 1 pixel wide) and 16 x 16 for the lists (3 x 2 tiles, a last column 1 wide, a last
row 1 high)."""
import ctypes as C

import numpy as np
import pytest

import denoise_var_model as dvm
import film_adaptive_model as am
from conftest import SCENES

pytestmark = pytest.mark.gpu

f32 = np.float32
W, H, N, BOUNCES = 33, 17, 12, 3
CHAIN = ((0, 1), (1, 4), (4, 5), (5, 12))
NAMES = ("cube", "alpha_transparency")
TILE = 16
TILING = am.Tiling(W, H, TILE, TILE)
PT_FLAG_NO_GRIDS, PT_FLAG_MEGAKERNEL = 4, 8


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def same_bits(a, b):
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    return a.shape == b.shape and bool((bits(a) == bits(b)).all())


def host(pta, name):
    return pta.HostScene.load_isf(SCENES / name / "scene.isf")


def profile(pta, samples=N):
    return pta.Profile.make(W, H, samples, BOUNCES)


@pytest.fixture(scope="module")
def refs(pta):
    """Per scene, rendered once by a scene of its own and left unchanged: the frame of pt_render_moments(N) and the N sample
    planes."""
    out = {}
    for name in NAMES:
        g = pta.GpuScene(host(pta, name))
        frame = g.render_moments(profile(pta))
        planes = g.render_samples(profile(pta))
        g.close()
        for a in frame + (planes,):
            a.setflags(write=False)
        assert np.abs(frame[1]).max() > 0
        out[name] = {"frame": frame, "planes": planes}
    return out


def run_chain(g, prof, chain, opts=None, tiles=None, want_moments=True):
    """The windows of `chain` on the same buffers; yields (s1, rgb8, accum, moments) after each."""
    acc = mom = None
    for s0, s1 in chain:
        rgb, acc, mom = g.render_window(prof, s0, s1, acc, mom, opts, tiles, want_moments)
        yield s1, rgb, acc, mom


@pytest.mark.parametrize("name", NAMES)
def test_chains_end_as_the_whole_frame_and_every_boundary_is_a_prefix(pta, oracle, refs, name):
    want, planes = refs[name]["frame"], refs[name]["planes"]
    g = pta.GpuScene(host(pta, name))
    prof = profile(pta)
    for chain in (CHAIN, ((0, 12),), ((0, 7), (7, 12))):
        for k, rgb, acc, mom in run_chain(g, prof, chain):
            w_acc, w_mom = dvm.moments_of(planes[:k])
            assert same_bits(acc, w_acc) and same_bits(mom, w_mom), (name, chain, k)
            assert np.array_equal(rgb, oracle.post_process(profile(pta, k), acc)), (name, chain, k)
        assert k == N
        assert np.array_equal(rgb, want[0]) and same_bits(acc, want[1]) and same_bits(mom, want[2]), (name, chain)
    # the running sums really differ from boundary to boundary, and a window that starts at 0 ignores what the buffers hold
    assert not same_bits(dvm.moments_of(planes[:4])[0], dvm.moments_of(planes[:5])[0])
    junk = np.full((W * H, 3), 1e6, f32), np.full((W * H, 2), 1e6, f32)
    rgb, acc, mom = g.render_window(prof, 0, N, junk[0], junk[1])
    assert same_bits(acc, want[1]) and same_bits(mom, want[2]) and np.array_equal(rgb, want[0])
    g.close()


@pytest.mark.parametrize("name", NAMES)
def test_batches_flags_and_shards_change_no_bit(pta, refs, name):
    want, planes = refs[name]["frame"], refs[name]["planes"]
    g = pta.GpuScene(host(pta, name))
    prof = profile(pta)
    for flags in (0, PT_FLAG_NO_GRIDS):
        for batch in (1, 3, 0):
            o = pta.Opts.make(flags=flags, sample_batch=batch)
            for k, rgb, acc, mom in run_chain(g, prof, CHAIN, o):
                w_acc, w_mom = dvm.moments_of(planes[:k])
                assert same_bits(acc, w_acc) and same_bits(mom, w_mom), (name, flags, batch, k)
            assert np.array_equal(rgb, want[0]), (name, flags, batch)
    # rank 1 of 3 shards: the packed local order of pt_render
    o = pta.Opts.make(shard_rank=1, shard_count=3, tile_w=8, tile_h=32)
    where = pta.local_pixel_map(prof, o)
    assert 0 < len(where) < W * H
    for k, rgb, acc, mom in run_chain(g, prof, CHAIN, o):
        w_acc, w_mom = dvm.moments_of(planes[:k, where])
        assert same_bits(acc, w_acc) and same_bits(mom, w_mom), (name, "shard", k)
    assert np.array_equal(rgb, want[0][where])
    # the megakernel carries accum the same way; it stages no samples, so it has no moments
    mega = pta.Opts.make(flags=PT_FLAG_MEGAKERNEL)
    for k, rgb, acc, mom in run_chain(g, prof, CHAIN, mega, want_moments=False):
        assert same_bits(acc, dvm.moments_of(planes[:k])[0]), (name, "megakernel", k)
    assert np.array_equal(rgb, want[0]) and mom is None
    acc, mom = np.full((W * H, 3), -7.0, f32), np.full((W * H, 2), -7.0, f32)
    assert g.lib.pt_render_window(g.handle, C.byref(prof), C.byref(mega), 0, 4, None, 0, None, acc.ctypes.data,
                                  mom.ctypes.data) == pta.PT_ERR_UNSUPPORTED
    assert (acc == f32(-7.0)).all() and (mom == f32(-7.0)).all()
    g.close()


def test_culled_blocks_carry_the_background(pta):
    """The pulled-back camera of tests/test_moments_gpu.py: whole 8 x 8 blocks see nothing, and k_accumulate's cull branch adds
    the background once per sample of the window."""
    cam_host = host(pta, "cube")
    cam = pta.make_camera(cam_host.camera)
    for k in range(3):
        cam.transform[12 + k] += f32(8.0) * cam.transform[8 + k]
    g, ref = pta.GpuScene(host(pta, "cube")), pta.GpuScene(host(pta, "cube"))
    g.set_camera(cam)
    ref.set_camera(cam)
    prof = pta.Profile.make(40, 24, N, BOUNCES)
    want = ref.render_moments(prof)
    planes = ref.render_samples(prof)
    for batch in (0, 3):
        for k, rgb, acc, mom in run_chain(g, prof, CHAIN, pta.Opts.make(sample_batch=batch)):
            blocks, n_empty = g.cull_stats()
            assert blocks > 0 and 0 < n_empty < blocks, (blocks, n_empty)
            w_acc, w_mom = dvm.moments_of(planes[:k])
            assert same_bits(acc, w_acc) and same_bits(mom, w_mom), (batch, k)
        assert np.array_equal(rgb, want[0]) and same_bits(acc, want[1]) and same_bits(mom, want[2])
    g.close()
    ref.close()


@pytest.mark.parametrize("name", NAMES)
def test_tile_list_windows_are_the_whole_frame_windows_pixels(pta, refs, name):
    planes = refs[name]["planes"]
    g = pta.GpuScene(host(pta, name))
    prof = profile(pta)
    o = pta.Opts.make(tile_w=TILE, tile_h=TILE)
    whole = {k: (rgb, acc, mom) for k, rgb, acc, mom in run_chain(g, prof, ((0, 5), (5, 12)), o)}
    for tiles in ([0, 4], [1, 2, 5]):      # tiles 2 and 5: a column 1 pixel wide; 4 and 5: a row 1 pixel high
        where = TILING.pixel_map(tiles)
        for flags in (0, PT_FLAG_NO_GRIDS):
            for k, rgb, acc, mom in run_chain(g, prof, ((0, 5), (5, 12)), pta.Opts.make(flags=flags, tile_w=TILE, tile_h=TILE), tiles):
                assert len(acc) == len(where)
                assert same_bits(acc, whole[k][1][where]) and same_bits(mom, whole[k][2][where]), (name, tiles, flags, k)
                assert np.array_equal(rgb, whole[k][0][where]), (name, tiles, flags, k)
                assert same_bits(acc, dvm.moments_of(planes[:k, where])[0])
    assert same_bits(whole[12][1], refs[name]["frame"][1])
    g.close()


def test_the_device_form_on_torch_tensors(pta, refs):
    import torch
    want, planes = refs["alpha_transparency"]["frame"], refs["alpha_transparency"]["planes"]
    g = pta.GpuScene(host(pta, "alpha_transparency"))
    prof = profile(pta)
    stream = torch.cuda.current_stream().cuda_stream
    n, guard = W * H, 64
    d_rgb = torch.full((n * 3 + guard,), 0xA5, dtype=torch.uint8, device="cuda")
    d_acc = torch.full((n * 3 + guard,), -7.0, dtype=torch.float32, device="cuda")
    d_mom = torch.full((n * 2 + guard,), -7.0, dtype=torch.float32, device="cuda")
    for s0, s1 in CHAIN:
        g.render_window_device(prof, pta.Opts.make(sample_batch=2), s0, s1, d_rgb.data_ptr(), d_acc.data_ptr(), d_mom.data_ptr(),
                               stream=stream)
        torch.cuda.synchronize()
        w_acc, w_mom = dvm.moments_of(planes[:s1])
        assert same_bits(d_acc.cpu().numpy()[:n * 3].reshape(-1, 3), w_acc), s1
        assert same_bits(d_mom.cpu().numpy()[:n * 2].reshape(-1, 2), w_mom), s1
    rgb, acc, mom = d_rgb.cpu().numpy(), d_acc.cpu().numpy(), d_mom.cpu().numpy()
    assert (rgb[n * 3:] == 0xA5).all() and (acc[n * 3:] == f32(-7.0)).all() and (mom[n * 2:] == f32(-7.0)).all()
    assert np.array_equal(rgb[:n * 3].reshape(-1, 3), want[0]) and same_bits(acc[:n * 3].reshape(-1, 3), want[1])
    # a tile list, accum alone
    tiles = [1, 5]
    where = am.Tiling(W, H, TILE, TILE).pixel_map(tiles)
    d_t = torch.full((len(where) * 3 + guard,), -7.0, dtype=torch.float32, device="cuda")
    o = pta.Opts.make(tile_w=TILE, tile_h=TILE)
    for s0, s1 in ((0, 5), (5, 12)):
        g.render_window_device(prof, o, s0, s1, None, d_t.data_ptr(), None, tiles=tiles, stream=stream)
    torch.cuda.synchronize()
    t = d_t.cpu().numpy()
    assert (t[len(where) * 3:] == f32(-7.0)).all() and same_bits(t[:len(where) * 3].reshape(-1, 3), want[1][where])
    g.close()


def test_a_chain_of_windows_leaves_the_scene_undisturbed(pta, refs):
    """The pattern of tests/test_render_tiles_gpu.py: the N-sample frame is rendered until it is planned and its caches are
    keyed; a chain of windows in between moves no counter, and the frame behind it follows its predecessor."""
    name = "cube"
    want = refs[name]["frame"]
    g = pta.GpuScene(host(pta, name))
    prof = profile(pta)
    o = pta.Opts.make()

    def counters():
        return g.rng_cache_stats(), g.hit_cache_stats(), g.hit1_cache_stats()
    for warm in (0, 4):
        for _ in range(warm):
            g.render(prof, o)
        before = g.render(prof, o)
        planned = g.info().frame_planned
        chunk, queue_bytes = g.info().queue_chunk_items, g.info().queue_bytes
        c0 = counters()
        if warm:
            assert planned == 1 and c0[0][2] > 0 and c0[1][2] > 0    # (words and camera hits are cached by now)
        for flags in (0, PT_FLAG_NO_GRIDS):
            for k, rgb, acc, mom in run_chain(g, prof, CHAIN, pta.Opts.make(flags=flags)):
                pass
            assert np.array_equal(rgb, want[0]) and same_bits(acc, want[1]) and same_bits(mom, want[2]), (warm, flags)
        for k, rgb, acc, mom in run_chain(g, prof, ((0, 5), (5, 12)), pta.Opts.make(tile_w=TILE, tile_h=TILE), [0, 5]):
            pass
        assert same_bits(acc, want[1][TILING.pixel_map([0, 5])])
        assert counters() == c0, warm                                # nothing keyed, released, zeroed or counted
        info = g.info()
        assert (info.frame_planned, info.queue_chunk_items, info.queue_bytes) == (planned, chunk, queue_bytes)
        after = g.render(prof, o)
        assert np.array_equal(before[0], after[0]) and same_bits(before[1], after[1]), warm
        if warm:
            c1 = counters()
            assert g.info().frame_planned == 1
            # the whole frame behind the windows loads what was cached and fills nothing again
            assert c1[0][3] == c0[0][3] and c1[1][3] == c0[1][3] and c1[1][4] > c0[1][4] and c1[2][3] == c0[2][3]
    assert np.array_equal(before[0], want[0]) and same_bits(before[1], want[1])
    g.close()


def test_every_refusal_leaves_the_outputs_untouched(pta, refs):
    import torch
    INVALID = pta.PT_ERR_INVALID
    g = pta.GpuScene(host(pta, "cube"))
    lib = g.lib
    n = W * H
    rgb = np.full((n, 3), 0xA5, np.uint8)
    acc, mom = np.full((n, 3), -7.0, f32), np.full((n, 2), -7.0, f32)
    good_prof, good_opts = profile(pta), pta.Opts.make(tile_w=TILE, tile_h=TILE)

    def call(s0=0, s1=4, prof=good_prof, o=good_opts, tiles=None, n_tiles=None, scene=g.handle, outs=(rgb, acc, mom)):
        ptrs = [x.ctypes.data if x is not None else None for x in outs]
        return lib.pt_render_window(scene, C.byref(prof) if prof is not None else None, C.byref(o) if o is not None else None,
                                    s0, s1, tiles.ctypes.data if tiles is not None else None,
                                    (len(tiles) if tiles is not None else 0) if n_tiles is None else n_tiles, *ptrs)

    def prof_with(**kw):
        p = profile(pta)
        for k, v in kw.items():
            setattr(p, k, v)
        return p
    u32 = lambda *v: np.asarray(v, np.uint32)   # noqa: E731
    # the window
    assert call(4, 4) == INVALID and call(5, 4) == INVALID and call(0, 13) == INVALID and call(12, 13) == INVALID
    assert call(0, 0) == INVALID and call(0xFFFFFFFF, 2) == INVALID
    assert call(outs=(rgb, None, mom)) == INVALID and call(outs=(None, None, None)) == INVALID      # a null accum
    # what pt_render refuses
    assert call(prof=prof_with(samples=0)) == INVALID and call(prof=prof_with(tonemap=7)) == INVALID
    assert call(prof=prof_with(brdf=5)) == INVALID and call(prof=prof_with(bounces=5000)) == INVALID
    assert call(prof=prof_with(width=0)) == INVALID
    assert call(o=pta.Opts.make(tile_w=12, tile_h=16)) == INVALID and call(o=pta.Opts.make(tile_w=8, tile_h=8)) == INVALID
    assert call(o=pta.Opts.make(shard_count=2, shard_rank=2)) == INVALID
    assert call(prof=None) == INVALID and call(scene=None) == INVALID
    # what pt_render_tiles refuses
    assert call(tiles=u32(0), n_tiles=0) == INVALID
    assert call(tiles=u32(3, 3)) == INVALID and call(tiles=u32(4, 3)) == INVALID and call(tiles=u32(6)) == INVALID
    assert call(tiles=u32(0, 1), o=pta.Opts.make(tile_w=TILE, tile_h=TILE, shard_count=2)) == INVALID
    assert (rgb == 0xA5).all() and (acc == f32(-7.0)).all() and (mom == f32(-7.0)).all()
    # the device form refuses the same, and writes nothing
    d_acc = torch.full((n * 3,), -7.0, dtype=torch.float32, device="cuda")
    dev = lambda s0, s1, tiles=None, accum=d_acc.data_ptr(): lib.pt_render_window_device(   # noqa: E731
        g.handle, C.byref(good_prof), C.byref(good_opts), s0, s1, tiles.ctypes.data if tiles is not None else None,
        len(tiles) if tiles is not None else 0, None, accum, None, None)
    assert dev(3, 3) == INVALID and dev(0, 13) == INVALID and dev(0, 4, u32(3, 3)) == INVALID and dev(0, 4, accum=None) == INVALID
    torch.cuda.synchronize()
    assert (d_acc.cpu().numpy() == f32(-7.0)).all()
    # and the next pt_render is what it would have been
    got = g.render(good_prof)
    assert np.array_equal(got[0], refs["cube"]["frame"][0]) and same_bits(got[1], refs["cube"]["frame"][1])
    assert call() == pta.PT_OK and not (acc == f32(-7.0)).any()
    g.close()
