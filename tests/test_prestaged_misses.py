"""Pre-staged misses (csrc/pt_wavefront.h, wf_prestage_miss): the kernel that makes the colour of a path's record final also
stages `colour + throughput x background` (renderer/mod.rs:184-186) for the case that the record's cast finds nothing, and
the shade pass of the next bounce does nothing at all for a miss.  A path that does hit has its slot overwritten by the
kernel that ends it, which is ordered behind the one that staged.

What could go wrong: a miss whose result nobody staged (a kernel that finishes a colour and was forgotten), a staged value
that survives although the path went on (overwrite order), a slot that still holds an earlier chunk's or sample batch's
value.  Every frame here is compared bit for bit - f32 accumulator, rgb8, counters - with the CPU oracle; the scenes have a
non-black background and let most secondary rays leave."""
import numpy as np
import pytest

import scene_builder as sb
import shading_model as sm

pytestmark = pytest.mark.gpu

COUNTERS = ("samples", "segments", "shadow_rays", "shaded_hits", "rng_draws")
PIPELINES = (0, 4)   # the fused grid pipeline (k_og_shadow patches the colours), PT_FLAG_NO_GRIDS (k_wf_shadow, side stream)

# open geometry (floor, wall, panel, ball under the sky): name -> (light set, factor set)
#   point  one point light: every lit surface goes through the shadow queue, the shadow kernels patch and stage
#   none   no light: k_wf_shade's survivors are final at every bounce
#   five   point + directional lights, two of them moot on most surfaces: records with a moot light next to a live one
#   alpha  translucent materials (the ALPHA kernels; a cast whose hits are all skipped shades the last one: a hit)
SCENES = {"point": ("point", "opaque"), "none": ("none", "opaque"), "five": ("five", "opaque"), "alpha": ("point", "alpha"),
          "alpha-five": ("five", "alpha")}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# from above: three of five camera rays meet the floor, the wall, the panel or the ball, and most rays that leave those leave the scene
CAMERA = dict(eye=(0.3, 3.2, 2.4), target=(0.1, 0.0, -0.3), fov=0.93)


def open_scene(name, bounces):
    light_set, factor_set = SCENES[name]
    case = sb.Case(f"prestage-{name}", "open", "none", light_set, factor_set, bounces, "FILMIC", 0, False)
    pta = sb.entry.load_package()
    return case, sb.build(case, camera=sb.make_camera(pta, **CAMERA))


def oracle_frame(oracle, scene, prof, walk=False, **kw):
    """The oracle's frame; walk: every ray of every path checked finite first (what lets a new scene onto a GPU)."""
    o = oracle.OracleScene(scene.desc, oracle.PTO_BRUTE_FORCE)
    assert not walk or sm.rays_finite(o, prof)
    rgb, acc, stats = o.render(prof, **kw)
    assert stats["numeric_errors"] == 0
    return rgb, acc, stats


def assert_same(got, want, what):
    assert np.array_equal(got[0], want[0]), (what, "rgb8", int((got[0] != want[0]).any(axis=1).sum()))
    same = bits(got[1]) == bits(want[1])
    assert same.all(), (what, "accum", int((~same).any(axis=1).sum()), "first", np.argwhere(~same)[0].tolist())


def secondary_miss_share(oracle, scene, case, w, h, spp, bounces):
    """Share of the casts of bounces >= 1 that find nothing, from the oracle's counts (opaque scenes: one shaded hit per
    cast that hits; the camera rays' part is the frame at depth 0)."""
    deep = oracle_frame(oracle, scene, sb.profile(case, w, h, spp, bounces=bounces))[2]
    flat = oracle_frame(oracle, scene, sb.profile(case, w, h, spp, bounces=0))[2]
    casts = deep["segments"] - flat["segments"]
    hits = deep["shaded_hits"] - flat["shaded_hits"]
    return 1.0 - hits / max(1, casts)


@pytest.mark.parametrize("bounces", [1, 2, 5, 8])
@pytest.mark.parametrize("name", list(SCENES))
def test_accumulator_and_counters_equal_the_oracle(pta, oracle, name, bounces):
    """Bounce counts 1, 2, 5 and 8 (Russian roulette from bounce 4 on), both pipelines, opaque and translucent scenes."""
    case, scene = open_scene(name, bounces)
    assert scene.translucent == name.startswith("alpha")
    w, h, spp = 160, 96, 4
    prof = sb.profile(case, w, h, spp)
    want = oracle_frame(oracle, scene, prof, walk=True)
    if not scene.translucent:
        share = secondary_miss_share(oracle, scene, case, w, h, spp, bounces)
        print(f"{name}, {bounces} bounces: {share:.3f} of the casts of bounces >= 1 leave the scene")
        assert share > 0.6, (name, bounces, share)
    g = pta.GpuScene(scene)
    for flags in PIPELINES:
        for frame in range(2):   # counted, then planned (queues of the counted lengths, launches behind the last ray left out)
            assert_same(g.render(prof, pta.Opts.make(flags=flags)), want, (name, bounces, flags, frame))
        got = g.render(prof, pta.Opts.make(flags=flags | pta.PT_FLAG_COUNTERS))
        assert_same(got, want, (name, bounces, flags, "counters"))
        c = g.counters().as_dict()
        assert {k: c[k] for k in COUNTERS} == {k: want[2][k] for k in COUNTERS}, (name, bounces, flags)
    g.close()


@pytest.mark.parametrize("flags", PIPELINES)
@pytest.mark.parametrize("name", ["point", "alpha-five"])
def test_staging_slots_reused_across_chunks_and_sample_batches(pta, oracle, monkeypatch, name, flags):
    """The same frame in one pass, in chunks of 1 Mi work items and sample batches of two (small PT_QUEUE_GIB /
    PT_STAGING_GIB) and with a preview after every batch of three: a slot is written again by every batch, and within a batch
    a pre-staged value is overwritten by the path's later kernels.  Same bits every time, and the oracle's."""
    case, scene = open_scene(name, 5)
    w, h, spp = 640, 360, 8                       # 1.97 M work items (32 x 32 tiles): two chunks
    prof = sb.profile(case, w, h, spp)
    want = oracle_frame(oracle, scene, prof)
    one_pass = pta.GpuScene(scene).render(prof, pta.Opts.make(flags=flags))
    assert_same(one_pass, want, (name, flags, "one pass"))
    monkeypatch.setenv("PT_QUEUE_GIB", "0.01")
    monkeypatch.setenv("PT_QUEUE_STEADY_GIB", "0.02")
    monkeypatch.setenv("PT_QUEUE_ONE_PASS_GIB", "0.02")
    monkeypatch.setenv("PT_STAGING_GIB", "0.006")   # 6.4 MB: two samples of 640 x 360 x 12 B
    g = pta.GpuScene(scene)
    for frame in range(3):
        assert_same(g.render(prof, pta.Opts.make(flags=flags)), one_pass, (name, flags, "chunks", frame))
        info = g.info().as_dict()
        assert info["queue_chunk_items"] < 640 * 384 * spp, info
    seen = []

    def preview(rgb8, n_pixels, done, total, user):
        seen.append((done, np.ctypeslib.as_array(rgb8, (n_pixels, 3)).copy()))

    monkeypatch.delenv("PT_STAGING_GIB")
    got = g.render(prof, pta.Opts.make(flags=flags, sample_batch=3, preview=preview))
    assert_same(got, one_pass, (name, flags, "preview"))
    assert [d for d, _ in seen] == [3, 6, 8]
    for done, rgb8 in seen:
        assert np.array_equal(rgb8, oracle_frame(oracle, scene, prof, sample_count=done)[0]), (name, flags, done)
    g.close()


@pytest.mark.parametrize("name", ["point", "five", "none"])
def test_a_path_that_goes_on_overwrites_what_was_staged_for_it(pta, oracle, name):
    """Paths whose miss result was staged at bounce b, that hit at b + 1 and end at b + 2: the frames at depth b + 1 and b + 2
    differ (some path was still going at b + 1 and its sample changed at b + 2), and each equals the oracle's - a staged value
    that outlived its path, or a later value written under it, would show at one of the depths.  `five`: two lights that are
    moot on most surfaces next to live ones, so k_og_shadow (and k_wf_shadow) retire records with a moot light."""
    w, h, spp = 128, 80, 6
    frames = {}
    for depth in (1, 2, 3, 4):
        case, scene = open_scene(name, depth)
        prof = sb.profile(case, w, h, spp)
        frames[depth] = want = oracle_frame(oracle, scene, prof, walk=True)
        g = pta.GpuScene(scene)
        for flags in PIPELINES:
            for frame in range(2):
                assert_same(g.render(prof, pta.Opts.make(flags=flags)), want, (name, depth, flags, frame))
        g.close()
    for depth in (1, 2, 3):
        changed = int((bits(frames[depth][1]) != bits(frames[depth + 1][1])).any(axis=1).sum())
        print(f"{name}: {changed} pixels change between depth {depth} and {depth + 1}")
        assert changed >= 100, (name, depth, changed)   # (such paths exist, in more than a stray pixel)
