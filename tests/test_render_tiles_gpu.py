"""Tile-list frames (pt_render_tiles) on the GPU: every packed pixel against the same pixel of the whole frame bit for
bit - lists, pipelines, sample batches, several chunks -, every refusal with the outputs untouched, and what a run of tile
frames leaves behind in its scene: nothing."""
import ctypes as C
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import film_adaptive_model as am
from conftest import SCENES

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
f32 = np.float32
W, H, TILE, BOUNCES, SAMPLES = 72, 40, 16, 2, 8   # 5 x 3 tiles, a last column 8 wide, a last row 8 high
TILING = am.Tiling(W, H, TILE, TILE)
LISTS = ([0], [14], list(range(0, 15, 2)), list(range(15)))
PT_FLAG_NO_GRIDS, PT_FLAG_MEGAKERNEL = 4, 8
NAMES = ("cube", "spheres", "alpha_transparency")


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def same_bits(a, b):
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    return a.shape == b.shape and bool((bits(a) == bits(b)).all())


def host(pta, name):
    return pta.HostScene.load_isf(SCENES / name / "scene.isf")


def opts(pta, flags=0, batch=0, **more):
    return pta.Opts.make(flags=flags, tile_w=TILE, tile_h=TILE, sample_batch=batch, **more)


_whole = {}


def whole(pta, name, flags=0, batch=0, samples=SAMPLES):
    """(rgb8, accum, moments or None) of the whole frame, rendered once by a scene of its own."""
    key = (name, flags, batch, samples)
    if key not in _whole:
        g = pta.GpuScene(host(pta, name))
        prof = pta.Profile.make(W, H, samples, BOUNCES)
        if flags & PT_FLAG_MEGAKERNEL:
            _whole[key] = g.render(prof, opts(pta, flags, batch)) + (None,)
        else:
            _whole[key] = g.render_moments(prof, opts(pta, flags, batch))
        g.close()
    return _whole[key]


def check_tiles(got, want, tiles, label):
    where = TILING.pixel_map(tiles)
    rgb, acc, mom = got
    assert len(rgb) == len(acc) == len(where), label
    assert np.array_equal(rgb, want[0][where]), label
    assert same_bits(acc, want[1][where]), label
    if want[2] is not None:
        assert same_bits(mom, want[2][where]), label
    assert np.abs(want[1]).max() > 0


@pytest.mark.parametrize("name", NAMES)
def test_every_packed_pixel_is_the_whole_frames_pixel(pta, name):
    g = pta.GpuScene(host(pta, name))
    prof = pta.Profile.make(W, H, SAMPLES, BOUNCES)
    for flags, batch in ((0, 0), (PT_FLAG_NO_GRIDS, 0), (PT_FLAG_MEGAKERNEL, 0), (0, 3), (PT_FLAG_NO_GRIDS, 3)):
        want = whole(pta, name, flags, batch)
        mega = bool(flags & PT_FLAG_MEGAKERNEL)
        for tiles in LISTS:
            assert pta.tiles_pixel_count(prof, tiles, opts(pta)) == len(TILING.pixel_map(tiles))
            got = g.render_tiles(prof, tiles, opts(pta, flags, batch), want_moments=not mega)
            check_tiles(got, want, tiles, (name, flags, batch, tiles))
        if mega:   # the megakernel stages no samples
            t = np.asarray([0], np.uint32)
            mom = np.full((256, 2), -3.0, f32)
            o = opts(pta, flags)
            assert g.lib.pt_render_tiles(g.handle, C.byref(prof), C.byref(o), t.ctypes.data, 1, None, None,
                                         mom.ctypes.data) == pta.PT_ERR_UNSUPPORTED
            assert (mom == f32(-3.0)).all()
    # batches agree with one another (the whole frames do: the references above are not one and the same render by accident)
    assert same_bits(whole(pta, name, 0, 0)[1], whole(pta, name, 0, 3)[1])
    # each output alone
    tiles = LISTS[2]
    want = whole(pta, name)
    where = TILING.pixel_map(tiles)
    t = np.asarray(tiles, np.uint32)
    o = opts(pta)
    rgb, acc, mom = np.empty((len(where), 3), np.uint8), np.empty((len(where), 3), f32), np.empty((len(where), 2), f32)
    for out in ((rgb, None, None), (None, acc, None), (None, None, mom)):
        ptrs = [x.ctypes.data if x is not None else None for x in out]
        pta.check_gpu(g.lib.pt_render_tiles(g.handle, C.byref(prof), C.byref(o), t.ctypes.data, len(t), *ptrs))
    check_tiles((rgb, acc, mom), want, tiles, (name, "one output at a time"))
    g.close()


def test_the_device_form_and_another_tiling(pta):
    """pt_render_tiles_device on the caller's stream with guard bytes behind every output; 70 x 50 in 32 x 8 tiles."""
    import torch
    g = pta.GpuScene(host(pta, "spheres"))
    w, h = 70, 50
    tiling = am.Tiling(w, h, 32, 8)     # 3 x 7 tiles: a last column 6 wide, a last row 2 high
    prof = pta.Profile.make(w, h, 4, BOUNCES)
    o = pta.Opts.make(tile_w=32, tile_h=8)
    ref = pta.GpuScene(host(pta, "spheres"))
    want = ref.render_moments(prof, o)
    for tiles in ([2], [20], [0, 5, 6, 19, 20], list(range(21))):
        where = tiling.pixel_map(tiles)
        n, guard = len(where), 64
        d_rgb = torch.full((n * 3 + guard,), 0xA5, dtype=torch.uint8, device="cuda")
        d_acc = torch.full((n * 3 + guard,), -7.0, dtype=torch.float32, device="cuda")
        d_mom = torch.full((n * 2 + guard,), -7.0, dtype=torch.float32, device="cuda")
        g.render_tiles_device(prof, o, tiles, d_rgb.data_ptr(), d_acc.data_ptr(), d_mom.data_ptr(),
                              torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        rgb, acc, mom = d_rgb.cpu().numpy(), d_acc.cpu().numpy(), d_mom.cpu().numpy()
        assert (rgb[n * 3:] == 0xA5).all() and (acc[n * 3:] == f32(-7.0)).all() and (mom[n * 2:] == f32(-7.0)).all()
        assert np.array_equal(rgb[:n * 3].reshape(-1, 3), want[0][where]), tiles
        assert same_bits(acc[:n * 3].reshape(-1, 3), want[1][where]), tiles
        assert same_bits(mom[:n * 2].reshape(-1, 2), want[2][where]), tiles
    g.close()
    ref.close()


CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
import __graft_entry__ as e
import film_adaptive_model as am
pta = e.load_package()
W, H, TILE = 72, 40, 16
tiling = am.Tiling(W, H, TILE, TILE)
prof = pta.Profile.make(W, H, 8, 2)
opts = pta.Opts.make(tile_w=TILE, tile_h=TILE)
for name in ("cube", "alpha_transparency"):
    sc = pta.HostScene.load_isf(%(scenes)r + "/" + name + "/scene.isf")
    g, ref = pta.GpuScene(sc, device=0), pta.GpuScene(sc, device=0)
    want = ref.render_moments(prof, opts)
    for tiles in ([14], list(range(0, 15, 2)), list(range(15))):
        where = tiling.pixel_map(tiles)
        rgb, acc, mom = g.render_tiles(prof, tiles, opts)
        ok = (np.array_equal(rgb, want[0][where]) and np.array_equal(acc.view(np.uint32), want[1][where].view(np.uint32))
              and np.array_equal(mom.view(np.uint32), want[2][where].view(np.uint32)))
        if not ok:
            print("MISMATCH", name, tiles)
            sys.exit(1)
print("OK")
"""


@pytest.mark.parametrize("extra", ({"PT_WF_CHUNK": "4096"}, {"PT_TILE_ORDER": "morton"}, {"PT_OG_FUSE_RNG": "0", "PT_WF_CHUNK": "4096"}),
                         ids=("chunks", "morton", "staged-words-in-chunks"))
def test_a_list_that_spans_several_chunks(extra):
    """The process-static knobs (tests/test_gpu_options.py): with PT_WF_CHUNK=4096 the every-other-tile list of 8 samples is
    8 tiles x 256 pixels x 8 samples = 16384 work items, four chunks; Morton order visits the listed tiles along a Z curve."""
    env = dict(os.environ)
    for k in list(env):
        if k.startswith(("PT_WF_", "PT_OG", "PT_SHADE_", "PT_TILE_", "PT_KD_", "PT_CAM_")):
            del env[k]
    env.update(extra)
    code = CHILD % {"root": str(ROOT), "tests": str(ROOT / "tests"), "scenes": str(SCENES)}
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith("OK"), (extra, out.stdout[-500:], out.stderr[-2000:])


def test_every_refusal_leaves_the_outputs_untouched(pta):
    import torch
    INVALID = pta.PT_ERR_INVALID
    g = pta.GpuScene(host(pta, "cube"))
    lib = g.lib
    n = W * H
    rgb = np.full((n, 3), 0xA5, np.uint8)
    acc, mom = np.full((n, 3), -7.0, f32), np.full((n, 2), -7.0, f32)
    good_prof, good_opts = pta.Profile.make(W, H, 4, BOUNCES), opts(pta)
    good = np.asarray([1, 3, 14], np.uint32)

    def call(prof=good_prof, o=good_opts, tiles=good, n_tiles=None, scene=g.handle, outs=(rgb, acc, mom)):
        ptrs = [x.ctypes.data if x is not None else None for x in outs]
        return lib.pt_render_tiles(scene, C.byref(prof) if prof is not None else None, C.byref(o) if o is not None else None,
                                   tiles.ctypes.data if tiles is not None else None,
                                   len(tiles) if n_tiles is None else n_tiles, *ptrs)

    def prof_with(**kw):
        p = pta.Profile.make(W, H, 4, BOUNCES)
        for k, v in kw.items():
            setattr(p, k, v)
        return p
    u32 = lambda *v: np.asarray(v, np.uint32)   # noqa: E731
    assert call(tiles=None, n_tiles=3) == INVALID                    # a null list
    assert call(n_tiles=0) == INVALID                                # an empty one
    assert call(tiles=u32(3, 3)) == INVALID and call(tiles=u32(4, 3)) == INVALID and call(tiles=u32(0, 5, 2)) == INVALID
    assert call(tiles=u32(15)) == INVALID and call(tiles=u32(0, 0xFFFFFFFF)) == INVALID
    assert call(o=opts(pta, shard_count=2)) == INVALID and call(o=opts(pta, shard_count=3, shard_rank=1)) == INVALID
    # what pt_render refuses
    assert call(prof=prof_with(samples=0)) == INVALID and call(prof=prof_with(tonemap=7)) == INVALID
    assert call(prof=prof_with(brdf=5)) == INVALID and call(prof=prof_with(bounces=5000)) == INVALID
    assert call(prof=prof_with(width=0)) == INVALID
    assert call(o=pta.Opts.make(tile_w=12, tile_h=16)) == INVALID and call(o=pta.Opts.make(tile_w=8, tile_h=8)) == INVALID
    assert call(o=opts(pta, shard_count=2, shard_rank=2)) == INVALID
    assert call(prof=None) == INVALID and call(scene=None) == INVALID and call(outs=(None, None, None)) == INVALID
    # the default tiling (32 x 32: 3 x 2 tiles) has no tile 6
    assert call(o=pta.Opts.make(), tiles=u32(6)) == INVALID
    assert (rgb == 0xA5).all() and (acc == f32(-7.0)).all() and (mom == f32(-7.0)).all()
    assert pta.tiles_pixel_count(good_prof, [3, 3], good_opts) == 0
    # the device form refuses the same, and writes nothing
    d_acc = torch.full((n * 3,), -7.0, dtype=torch.float32, device="cuda")
    for tiles, o in ((u32(3, 3), good_opts), (u32(15), good_opts), (good, opts(pta, shard_count=2))):
        assert lib.pt_render_tiles_device(g.handle, C.byref(good_prof), C.byref(o), tiles.ctypes.data, len(tiles), None,
                                          d_acc.data_ptr(), None, None) == INVALID
    assert lib.pt_render_tiles_device(g.handle, C.byref(good_prof), C.byref(good_opts), None, 2, None, d_acc.data_ptr(), None, None) == INVALID
    assert lib.pt_render_tiles_device(g.handle, C.byref(good_prof), C.byref(good_opts), good.ctypes.data, 3, None, None, None, None) == INVALID
    torch.cuda.synchronize()
    assert (d_acc.cpu().numpy() == f32(-7.0)).all()
    # and the scene still renders
    assert call() == pta.PT_OK and not (acc[:256 * 2 + 64] == f32(-7.0)).any() and (acc[256 * 2 + 64:] == f32(-7.0)).all()
    g.close()


def test_tile_frames_leave_the_scene_undisturbed(pta):
    import torch
    h = host(pta, "spheres")
    prof = pta.Profile.make(W, H, 4, BOUNCES)
    o = opts(pta)
    want = whole(pta, "spheres", samples=4)
    g = pta.GpuScene(h)

    def counters():
        return g.rng_cache_stats(), g.hit_cache_stats(), g.hit1_cache_stats()
    for warm in (0, 4):   # a fresh scene, then one that has rendered four frames of the view (planned, caches keyed)
        for _ in range(warm):
            g.render(prof, o)
        before = g.render(prof, o)
        planned = g.info().frame_planned
        chunk, queue_bytes = g.info().queue_chunk_items, g.info().queue_bytes
        c0 = counters()
        if warm:
            assert planned == 1 and c0[0][2] > 0 and c0[1][2] > 0    # (words and camera hits are cached by now)
        for tiles in LISTS + ([3], [7, 8]):
            for flags in (0, PT_FLAG_NO_GRIDS):
                got = g.render_tiles(prof, tiles, opts(pta, flags))
                check_tiles(got, want, tiles, (warm, tiles, flags))
        other = pta.Profile.make(W, H, 8, BOUNCES)                   # ... and frames of another configuration
        check_tiles(g.render_tiles(other, [2, 14], o), whole(pta, "spheres"), [2, 14], (warm, "8 samples"))
        assert counters() == c0, warm                                # nothing keyed, released, zeroed or counted
        info = g.info()
        assert (info.frame_planned, info.queue_chunk_items, info.queue_bytes) == (planned, chunk, queue_bytes)
        after = g.render(prof, o)
        assert np.array_equal(before[0], after[0]) and same_bits(before[1], after[1]), warm
        if warm:
            c1 = counters()
            assert g.info().frame_planned == 1
            # the whole frame behind the tile frames follows its predecessor: it loads what was cached, it fills nothing again
            assert c1[0][3] == c0[0][3] and c1[1][3] == c0[1][3] and c1[1][4] > c0[1][4] and c1[2][3] == c0[2][3]
    assert np.array_equal(before[0], want[0]) and same_bits(before[1], want[1])
    g.close()
    torch.cuda.synchronize()   # no HIP error is pending on the device the scene renders on
    assert float(torch.ones(4, device="cuda").sum().item()) == 4.0
