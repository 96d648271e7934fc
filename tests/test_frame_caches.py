"""What the scene's three frame caches do to each other (csrc/pt_gpu.hip FrameCache: the ChaCha words, the camera hits, the
bounce-0 shadow visibility).  Each has a test file of its own; here one of them is switched off or given another budget
under a live scene while the other two go on.  The hit cache is eligible only in a frame that uses the word cache, the
visibility cache only in a frame that uses the hit cache - but an ineligible frame leaves a cache's contents, key and
allocation alone, and still updates the key "of the last frame", so the caches come back without storing or zeroing again.

The expected tuples follow from the caches' rules, not from a run: a cache is keyed in a frame whose key equals that of the
frame before (also when that frame was switched off or ineligible) and whose stride - min(items, budget / bytes per item)
& ~63 - differs from the keyed one; keying keeps an allocation that is large enough and at most 64 MiB too large and
restarts the prefix; a chunk [g0, g1) of frame-global items fills / stores when g1 <= stride and g0 <= mark < g1, reads /
loads when g1 <= mark, and runs the visibility variant when it loads and g1 <= the visibility plane's stride.  Every frame
is compared bit for bit with a fresh scene rendered with all three switches at 0."""
import pytest

import scene_builder as sb
from test_prestaged_misses import assert_same, open_scene

gpu = pytest.mark.gpu

W, H, SPP, BOUNCES = 160, 96, 4, 5
N = W * H * SPP   # 61 440 work items: 160 x 96 is whole 32 x 32 tiles
SWITCHES = ("PT_RNG_CACHE", "PT_HIT_CACHE", "PT_VIS_CACHE")


def stats(g):
    """(bytes, items, cached, fills), (bytes, items, cached, stores, loads), (bytes, items, resets, launches)"""
    return g.rng_cache_stats(), g.hit_cache_stats(), g.vis_cache_stats()


def all_off(pta, monkeypatch, scene, prof, opts=None):
    """The frame of a fresh scene with the three caches switched off (the second frame of the view: the one that would key)."""
    for name in SWITCHES:
        monkeypatch.setenv(name, "0")
    g = pta.GpuScene(scene)
    g.render(prof, opts)
    out = g.render(prof, opts)
    assert stats(g) == ((0, 0, 0, 0), (0, 0, 0, 0, 0), (0, 0, 0, 0))
    g.close()
    for name in SWITCHES:
        monkeypatch.delenv(name)
    return out


def frame(g, prof, opts, want, what, expect):
    assert_same(g.render(prof, opts), want, what)
    got = stats(g)
    print(what, got)
    assert got == expect, (what, got, expect)


@gpu
def test_word_cache_switched_off_and_on_under_the_other_two(pta, monkeypatch):
    """One chunk per frame.  Frames 0-3 as in the caches' own tests: nothing, then fill + store + zeroed plane, then loads
    with the visibility variant.  A frame with PT_RNG_CACHE=0 gives the words' planes back and - no word cache in use - is
    ineligible for the other two: their numbers and allocations stay.  Switched on again, the words are keyed in the first
    frame (its key follows itself: the key of the last frame is kept through the switched-off one) and filled by its only
    chunk; that chunk's words are cached again, so it loads the hits that were kept - no new store - and runs the
    visibility variant on the plane that was kept - no new reset."""
    case, scene = open_scene("point", BOUNCES)
    prof = sb.profile(case, W, H, SPP)
    want = all_off(pta, monkeypatch, scene, prof)
    g = pta.GpuScene(scene)
    frame(g, prof, None, want, "first", ((0, 0, 0, 0), (0, 0, 0, 0, 0), (0, 0, 0, 0)))
    frame(g, prof, None, want, "keyed", ((32 * N, N, N, 1), (16 * N, N, N, 1, 0), (N, N, 1, 0)))
    frame(g, prof, None, want, "serving 1", ((32 * N, N, N, 1), (16 * N, N, N, 1, 1), (N, N, 1, 1)))
    frame(g, prof, None, want, "serving 2", ((32 * N, N, N, 1), (16 * N, N, N, 1, 2), (N, N, 1, 2)))
    monkeypatch.setenv("PT_RNG_CACHE", "0")
    frame(g, prof, None, want, "words off", ((0, 0, 0, 1), (16 * N, N, N, 1, 2), (N, N, 1, 2)))
    frame(g, prof, None, want, "words off 2", ((0, 0, 0, 1), (16 * N, N, N, 1, 2), (N, N, 1, 2)))
    monkeypatch.delenv("PT_RNG_CACHE")
    frame(g, prof, None, want, "words on", ((32 * N, N, N, 2), (16 * N, N, N, 1, 3), (N, N, 1, 3)))
    frame(g, prof, None, want, "words on 2", ((32 * N, N, N, 2), (16 * N, N, N, 1, 4), (N, N, 1, 4)))
    g.close()


@gpu
def test_hit_budget_changed_under_the_other_two(pta, monkeypatch):
    """Sample batches of two: two chunks per frame, g in [0, N/2) and [N/2, N).  With PT_HIT_CACHE_GIB at exactly N/2 records
    the hit cache is keyed again in the first frame of that budget (same key as the frame before, another stride): the
    allocation - large enough, less than 64 MiB too large - stays, the mark restarts, the first chunk stores and the
    second, above the stride, casts.  From the next frame the first chunk loads and runs the visibility variant (the plane
    was not zeroed: its key and stride are as before), the second does neither.  The words never change.  Back at the
    default budget: keyed again at stride N, both chunks store, then both load."""
    case, scene = open_scene("point", BOUNCES)
    prof = sb.profile(case, W, H, SPP)
    opts = pta.Opts.make(sample_batch=2)
    want = all_off(pta, monkeypatch, scene, prof, opts)
    half = N // 2
    assert half % 64 == 0
    words = (32 * N, N, N, 2)
    g = pta.GpuScene(scene)
    frame(g, prof, opts, want, "first", ((0, 0, 0, 0), (0, 0, 0, 0, 0), (0, 0, 0, 0)))
    frame(g, prof, opts, want, "keyed", (words, (16 * N, N, N, 2, 0), (N, N, 1, 0)))
    frame(g, prof, opts, want, "serving 1", (words, (16 * N, N, N, 2, 2), (N, N, 1, 2)))
    frame(g, prof, opts, want, "serving 2", (words, (16 * N, N, N, 2, 4), (N, N, 1, 4)))
    monkeypatch.setenv("PT_HIT_CACHE_GIB", repr(half * 16 / 2.0 ** 30))   # (exact: 15 x 2^-15)
    assert int(float(repr(half * 16 / 2.0 ** 30)) * 2.0 ** 30) // 16 == half
    frame(g, prof, opts, want, "half: keyed", (words, (16 * N, N, half, 3, 4), (N, N, 1, 4)))
    frame(g, prof, opts, want, "half: serving 1", (words, (16 * N, N, half, 3, 5), (N, N, 1, 5)))
    frame(g, prof, opts, want, "half: serving 2", (words, (16 * N, N, half, 3, 6), (N, N, 1, 6)))
    monkeypatch.delenv("PT_HIT_CACHE_GIB")
    frame(g, prof, opts, want, "default: keyed", (words, (16 * N, N, N, 5, 6), (N, N, 1, 6)))
    frame(g, prof, opts, want, "default: serving", (words, (16 * N, N, N, 5, 8), (N, N, 1, 8)))
    g.close()
