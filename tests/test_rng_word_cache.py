"""The scene's cache of ChaCha words (csrc/pt_gpu.hip RngCache, csrc/pt_wavefront.h k_wf_shade<..., GRID 3 + 8>): words 0-7 of
block 0 of every work item depend on the item enumeration alone - image size, samples, shard, tiling, sample batch - so a
frame that directly follows another of the same enumeration keys the cache to it, fills it chunk by chunk, and the fused
bounce-0 kernel of the later frames reads the words instead of deriving them.

What could go wrong: stale words after the enumeration changed (every seed changes with the sample count), something that
depends on the camera cached with them (the jittered screen position), a chunk that reads above the filled prefix or beyond
the budget, a shard reading another shard's words, a frame on another stream reading before the fill has finished.  Every
frame here is compared bit for bit - f32 accumulator and rgb8 - with the CPU oracle or with a render that has the cache
switched off, and every test reads the cache's own numbers (GpuScene.rng_cache_stats): without them it would prove nothing."""
import numpy as np
import pytest

import scene_builder as sb
import test_kernel_resources as kr
from test_prestaged_misses import COUNTERS, assert_same, open_scene, oracle_frame

gpu = pytest.mark.gpu

W, H, SPP, BOUNCES = 160, 96, 4, 5
ITEMS = W * H * SPP   # 61 440: 160 x 96 is whole 32 x 32 tiles


def stats(g):
    return dict(zip(("bytes", "items", "cached", "fills"), g.rng_cache_stats()))


def uncached(pta, monkeypatch, scene, prof, opts=None):
    """The frame of a fresh scene with the cache switched off."""
    monkeypatch.setenv("PT_RNG_CACHE", "0")
    g = pta.GpuScene(scene)
    out = g.render(prof, opts)
    assert stats(g) == dict(bytes=0, items=0, cached=0, fills=0)
    g.close()
    monkeypatch.delenv("PT_RNG_CACHE")
    return out


@gpu
@pytest.mark.parametrize("name", ["point", "alpha-five"])
def test_consecutive_frames_read_the_cache_and_equal_the_oracle(pta, oracle, monkeypatch, name):
    """Four frames and an instrumented one, both pipelines: the oracle's bits and an uncached render's; the fused pipeline
    has every item cached from its second frame on (one fill), the KD-tree pipeline and the counters frame leave the cache
    alone."""
    case, scene = open_scene(name, BOUNCES)
    prof = sb.profile(case, W, H, SPP)
    want = oracle_frame(oracle, scene, prof, walk=True)
    for flags in (0, 4):
        opts = pta.Opts.make(flags=flags)
        assert_same(uncached(pta, monkeypatch, scene, prof, opts), want, (name, flags, "uncached"))
        g = pta.GpuScene(scene)
        for frame in range(4):
            assert_same(g.render(prof, opts), want, (name, flags, frame))
            st = stats(g)
            if flags == 0 and frame >= 1:
                assert st == dict(bytes=ITEMS * 32, items=ITEMS, cached=ITEMS, fills=1), (name, frame, st)
            else:   # (a first frame; the KD-tree pipeline stages its words per frame)
                assert st["cached"] == 0 and st["fills"] == 0, (name, flags, frame, st)
        before = stats(g)
        got = g.render(prof, pta.Opts.make(flags=flags | pta.PT_FLAG_COUNTERS))
        assert_same(got, want, (name, flags, "counters"))
        c = g.counters().as_dict()
        assert {k: c[k] for k in COUNTERS} == {k: want[2][k] for k in COUNTERS}, (name, flags)
        assert stats(g) == before
        assert_same(g.render(prof, opts), want, (name, flags, "after counters"))
        assert stats(g) == before
        g.close()


@gpu
def test_edits_between_cached_frames(pta, oracle):
    """A camera move, a light edit and a material edit between cached frames: each frame is a fresh scene's in the new
    state and the oracle's, and nothing is filled again - the words are the enumeration's, not the camera's."""
    case, scene = open_scene("point", BOUNCES)
    prof = sb.profile(case, W, H, SPP)
    cam2 = sb.make_camera(pta, eye=(-0.9, 2.1, 2.9), target=(0.3, 0.3, -0.4), fov=0.8)
    lights2 = sb.make_lights(pta, "point_dir")
    mats2 = sb.case_materials(case._replace(factor_set="glow"), pta)
    g = pta.GpuScene(scene)
    for frame in range(2):
        assert_same(g.render(prof), oracle_frame(oracle, scene, prof), ("start", frame))
    filled = stats(g)
    assert filled == dict(bytes=ITEMS * 32, items=ITEMS, cached=ITEMS, fills=1)
    states = [("camera", lambda: g.set_camera(cam2), dict(camera=cam2)),
              ("lights", lambda: g.set_lights(lights2), dict(camera=cam2, lights=lights2)),
              ("materials", lambda: g.set_materials(mats2), dict(camera=cam2, lights=lights2, materials=mats2))]
    seen = [g.render(prof)]
    for what, edit, state in states:
        edit()
        fresh_scene = sb.build(case, pta=pta, **state)
        want = oracle_frame(oracle, fresh_scene, prof, walk=True)
        fresh = pta.GpuScene(fresh_scene)
        assert_same(fresh.render(prof), want, (what, "fresh"))
        fresh.close()
        for frame in range(2):
            got = g.render(prof)
            assert_same(got, want, (what, frame))
        assert not np.array_equal(got[1], seen[-1][1]), what   # (the edit changed the image)
        seen.append(got)
        assert stats(g) == filled, (what, stats(g))
    g.close()


@gpu
def test_change_of_enumeration(pta, oracle):
    """A A B B A A C C (B: twice the samples - every seed differs; C: the image transposed): the cache follows an enumeration
    at its second consecutive frame, and every frame is its own oracle frame.  A B A B A B: never keyed, same bits."""
    case, scene = open_scene("point", BOUNCES)
    profs = {"A": sb.profile(case, W, H, SPP), "B": sb.profile(case, W, H, 2 * SPP), "C": sb.profile(case, H, W, SPP)}
    want = {k: oracle_frame(oracle, scene, p) for k, p in profs.items()}
    items = {"A": ITEMS, "B": 2 * ITEMS, "C": ITEMS}
    g = pta.GpuScene(scene)
    keyed, fills = None, 0
    for n, k in enumerate("AABBAACC"):
        assert_same(g.render(profs[k]), want[k], (n, k))
        if n % 2 == 1:
            keyed, fills = k, fills + 1
        st = stats(g)
        if keyed is None:
            assert st == dict(bytes=0, items=0, cached=0, fills=0), (n, k, st)
        else:
            assert (st["items"], st["cached"], st["fills"]) == (items[keyed], items[keyed], fills), (n, k, st)
    g.close()
    g = pta.GpuScene(scene)
    for n, k in enumerate("ABABAB"):
        assert_same(g.render(profs[k]), want[k], (n, k))
        assert stats(g) == dict(bytes=0, items=0, cached=0, fills=0), (n, k)
    g.close()


@gpu
@pytest.mark.parametrize("name", ["point", "alpha-five"])
def test_chunks_sample_batches_and_a_partial_budget(pta, monkeypatch, name):
    """Small queues: the frame runs in two chunks of one pass over all eight samples (sample_batch 0), and - sample batches
    of two, asked for through pt_opts.sample_batch: the staging budget is read once per process and cannot be switched
    here - in four passes of one chunk each; the cache fills as a prefix over them.  With room for half of the items the
    rest derives its words as before.  Same bits as an uncached frame in one pass."""
    case, scene = open_scene(name, BOUNCES)
    w, h, spp = 640, 360, 8
    items = 640 * 384 * spp   # 1 966 080 (32 x 32 tiles): 62.9 MB of words
    prof = sb.profile(case, w, h, spp)
    one_pass = uncached(pta, monkeypatch, scene, prof)
    monkeypatch.setenv("PT_QUEUE_GIB", "0.01")
    monkeypatch.setenv("PT_QUEUE_STEADY_GIB", "0.02")
    monkeypatch.setenv("PT_QUEUE_ONE_PASS_GIB", "0.02")
    for budget, batch in ((None, 0), (None, 2), ("0.03", 2)):
        if budget:
            monkeypatch.setenv("PT_RNG_CACHE_GIB", budget)   # room for 1 006 592 items: two of the four batches
        g = pta.GpuScene(scene)
        for frame in range(4):
            assert_same(g.render(prof, pta.Opts.make(sample_batch=batch)), one_pass, (name, budget, batch, frame))
            assert g.info().as_dict()["queue_chunk_items"] < items
            st = stats(g)
            if frame == 0:
                assert st["cached"] == 0, st
            elif budget is None:
                assert st["items"] == items and st["cached"] == items and st["bytes"] == items * 32, (batch, frame, st)
            else:
                assert st["items"] == items and 0 < st["cached"] < items and st["bytes"] <= 0.03 * 2 ** 30, (frame, st)
        g.close()


@gpu
def test_shards(pta, oracle):
    """Ranks 0 and 1 of 2 with 32 x 32 tiles, a scene each, three frames: each rank's pixels are the unsharded frame's, from
    its own words."""
    case, scene = open_scene("point", BOUNCES)
    prof = sb.profile(case, W, H, SPP)
    want = oracle_frame(oracle, scene, prof)
    cached = 0
    for r in range(2):
        o = pta.Opts.make(shard_rank=r, shard_count=2, tile_w=32, tile_h=32)
        m = pta.local_pixel_map(prof, o)
        g = pta.GpuScene(scene)
        for frame in range(3):
            rgb, acc = g.render(prof, o)
            assert_same((rgb, acc), (want[0][m], want[1][m]), (r, frame))
        st = stats(g)
        assert st["items"] == len(m) * SPP and st["cached"] == st["items"] and st["fills"] == 1, (r, st)
        cached += st["cached"]
        g.close()
    assert cached == ITEMS


@gpu
def test_frames_in_flight_on_two_streams(pta, oracle):
    """Six frames enqueued without a host wait, alternating between two streams: the second fills the cache on its stream,
    the third reads it on the other.  Each stream waits on the device for the frame before it (wait_stream) - it has to,
    the scene's queues are one frame's at a time - so that wait already orders the read behind the fill: this test shows
    that frames in flight on two streams get the right words, NOT that the library's own wait for the fill event is
    needed (it passes without it)."""
    import torch
    case, scene = open_scene("point", BOUNCES)
    prof = sb.profile(case, W, H, SPP)
    want = oracle_frame(oracle, scene, prof)
    n = W * H
    outs = [(torch.empty(n * 3, dtype=torch.uint8, device="cuda"), torch.empty(n * 3, dtype=torch.float32, device="cuda")) for _ in range(6)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    g = pta.GpuScene(scene)
    for k, (rgb, acc) in enumerate(outs):
        st = streams[k & 1]
        st.wait_stream(streams[(k & 1) ^ 1])
        g.render_device(prof, pta.Opts.make(), rgb.data_ptr(), acc.data_ptr(), st.cuda_stream)
    for st in streams:
        st.synchronize()
    for k, (rgb, acc) in enumerate(outs):
        assert_same((rgb.cpu().numpy().reshape(-1, 3), acc.cpu().numpy().reshape(-1, 3)), want, k)
    assert stats(g) == dict(bytes=ITEMS * 32, items=ITEMS, cached=ITEMS, fills=1)
    g.close()


def test_cached_variant_stays_within_the_budget_of_its_occupancy(tmp_path):
    """The cached bounce-0 kernels as the built library has them: the waves per SIMD follow from the registers the code
    object allocates (512 per SIMD lane, in granules of 8); the opaque variant (config 3) ships at 3 waves like the kernel it
    stands in for, with the scratch measured for it (8 B) plus a little - at 4 waves it keeps 180 B there and is slower."""
    t = kr.kernel_table(tmp_path)
    b0 = kr.find(t, "k_wf_shadeILb0ELb0ELb1ELi11EE")
    waves = 512 // (-(-b0["vgpr_count"] // 8) * 8)
    assert waves >= 3 and b0["private_segment_fixed_size"] <= 16, (waves, b0)
    # translucent scenes (measured 84 B; the variant that derives its words 92 B)
    b0a = kr.find(t, "k_wf_shadeILb1ELb0ELb1ELi11EE")
    assert 512 // (-(-b0a["vgpr_count"] // 8) * 8) >= 3 and b0a["private_segment_fixed_size"] <= 96, b0a
