"""The lean variant of the fused shade pass of bounces 1 and 2 (csrc/pt_wf_shade_body.h LEAN1 and HAND, k_wf_shade_fused<256 | 8192>
and <256 | 16384>; csrc/pt_gpu.hip lean_frame, frame_plan, render_chunk, shade_stage).  A steady frame writes next to no
shadow record at these bounces - every visibility byte is known, the pass adds the lights itself - so a bounce whose last
counted frame sent fewer than 1/64 of its shaded records to the shadow queue launches a variant of the kernel without the
shadow-record, sorting, exact-list, roulette and ChaCha code: 96 registers, no scratch, five waves per SIMD.  A queue entry
that needs the missing code - a light of unknown visibility, a normal too long for the light grids - is written nothing for
and appended to a list; the general body runs over that list right behind the lean launch and shades the record whole.

What could go wrong: an entry shaded twice or not at all, a record handed over in part (some lights added), a colour read
from another thread's LDS slot or a stale step's, counts the frame plan reads that differ between the two ways, a list pass
behind the shadow kernel or the next bounce's loads, a bounce that stays lean across an edit.  Every frame of every sequence
is compared bit for bit - rgb8 and the f32 accumulator - with the same sequence under PT_B1_LEAN=0, together with the queue
bytes, the plan flag and the fused statistics of bounces 1 and 2, and every test reads the launch counts that make it mean
something (GpuScene.b1_lean_stats).

The scene and the helpers are tests/test_bounce0_lean.py's: 404 triangles and a sphere, 70 x 38 pixels, 4 spp, 3 bounces;
wall=True adds the slab whose vertex normals have lengths 4 and 0.5 - surfaces that take the shadow queue in every frame."""
import numpy as np
import pytest

import scene_builder as sb
from test_bounce0_lean import SPP, lean_lights, lean_scene
from test_masked_sequences import schedule
from test_prestaged_misses import assert_same, oracle_frame

gpu = pytest.mark.gpu

NAMES = ("lean1", "lean2", "general", "handed")
FUSED = ("launches", "inlined", "deferred", "next_written", "next_elided", "next_unknown")
SHARE = 64   # (pt_gpu.hip PT_B1_LEAN_SHARE)


def stats(g):
    d = dict(zip(NAMES, g.b1_lean_stats()))
    for b in (1, 2):
        for name, v in zip(FUSED, g.bounce_fused_stats(b)):
            d[f"{name}{b}"] = v
    return d


def sequence(pta, monkeypatch, scene, prof, frames, lean, edits=None, opts=None):
    """`frames` frames of a fresh GpuScene with PT_B1_LEAN=lean; edits: {frame: function(g)} applied before that frame.
    Returns per frame (rgb8, accum) and what that frame alone added to every count, with the plan flag and the queue bytes."""
    monkeypatch.setenv("PT_B1_LEAN", lean)
    g = pta.GpuScene(scene)
    out, seen, before = [], [], stats(g)
    for k in range(frames):
        if edits and k in edits:
            edits[k](g)
        out.append(g.render(prof, opts) if opts is not None else g.render(prof))
        now = stats(g)
        d = {key: now[key] - before[key] for key in now}
        d["planned"], d["queue_bytes"] = int(g.info().frame_planned), int(g.info().queue_bytes)
        seen.append(d)
        before = now
    g.close()
    return out, seen


def brief(seen):
    return [(s["lean1"], s["lean2"], s["general"], s["handed"], s["planned"], s["deferred1"], s["deferred2"]) for s in seen]


def both(pta, monkeypatch, scene, prof, frames, what, edits=None, opts=None, forced=False):
    """The sequence with the switch off and on: the same frames bit for bit, the same plan, queues and fused statistics;
    what the lean launches handed over is what the general pass sent to the shadow queue there.  Returns both per-frame lists."""
    monkeypatch.delenv("PT_B1_LEAN_TEST_FORCE", raising=False)
    ref, off = sequence(pta, monkeypatch, scene, prof, frames, "0", edits, opts)
    if forced:
        monkeypatch.setenv("PT_B1_LEAN_TEST_FORCE", "1")
    got, on = sequence(pta, monkeypatch, scene, prof, frames, "1", edits, opts)
    monkeypatch.delenv("PT_B1_LEAN_TEST_FORCE", raising=False)
    print(what, "off:", brief(off))
    print(what, "on: ", brief(on))
    for k in range(frames):
        assert_same(got[k], ref[k], (what, k))
        a, b = on[k], off[k]
        assert b["lean1"] == b["lean2"] == b["handed"] == 0, (what, k, b)
        assert a["lean1"] + a["lean2"] + a["general"] == b["general"], (what, k, a, b)
        assert a["planned"] == b["planned"] and a["queue_bytes"] == b["queue_bytes"], (what, k, a, b)
        for bounce in (1, 2):
            for name in FUSED:
                assert a[f"{name}{bounce}"] == b[f"{name}{bounce}"], (what, k, name, bounce, a, b)
        # a lean launch hands over exactly the records the general pass defers; a general launch hands over nothing
        want = sum(b[f"deferred{bounce}"] for bounce in (1, 2) if a[f"lean{bounce}"])
        assert a["handed"] == want, (what, k, a, b)
        if not forced and (a["lean1"] or a["lean2"]):   # behind a planned, counted frame only
            assert a["planned"] == 1 and k > 0 and on[k - 1]["planned"] == 1, (what, k, brief(on))
    return on, off, got


def first_lean(seen, start=0, key="lean1"):
    return next((k for k in range(start, len(seen)) if seen[k][key]), None)


def test_the_library_has_the_getter(pta):
    """No GPU: the symbol is there."""
    assert "pt_get_b1_lean_stats" in pta.GPU_SYMBOLS and len(pta.gpu_lib().pt_get_b1_lean_stats.argtypes) == 5


def test_the_lean_variant_fits_its_waves_without_scratch(tmp_path):
    """From the built library: the lean instantiation (GRIDX 256 | 8192) ships at five waves per SIMD - no scratch, at most
    512 / 5 registers in the allocation's granules of 8, and LDS that allows five workgroups of four waves on a CU's 160 KiB;
    the list pass (256 | 16384) is the general body; k_wf_shade_fused<256> stays at 128 registers, 84 B and 6 456 B."""
    from test_kernel_resources import find, kernel_table
    waves = 5
    t = kernel_table(tmp_path)
    lean = find(t, "k_wf_shade_fusedILi8448EE")
    print(lean)
    assert lean["private_segment_fixed_size"] == 0 and lean["vgpr_count"] <= (512 // waves) // 8 * 8, lean
    assert lean["group_segment_fixed_size"] <= 160 * 1024 // waves, lean
    general = find(t, "k_wf_shade_fusedILi256EE")
    assert (general["vgpr_count"], general["private_segment_fixed_size"], general["group_segment_fixed_size"]) == (128, 84, 6456), general
    hand = find(t, "k_wf_shade_fusedILi16640EE")
    assert hand["vgpr_count"] <= 128 and hand["private_segment_fixed_size"] <= 84 and hand["group_segment_fixed_size"] <= 6456, hand


@gpu
def test_a_fresh_scene_goes_lean_behind_a_counted_frame(pta, oracle, monkeypatch):
    """Default schedule, eight frames, all of them the oracle's frame.  The bounces go lean behind a planned frame whose counts
    came home with (next to) no shadow record, stay lean, and hand nothing over: every byte is known, every normal short."""
    case, scene, prof = lean_scene(pta)
    want = oracle_frame(oracle, scene, prof, walk=True)
    schedule(monkeypatch, "default")
    on, off, got = both(pta, monkeypatch, scene, prof, 8, "fresh")
    first = [first_lean(on, key=key) for key in ("lean1", "lean2")]
    assert None not in first and all(3 <= k <= 6 for k in first), brief(on)
    assert all(s["lean1"] and s["lean2"] and s["general"] == 0 for s in on[max(first):]), brief(on)
    assert sum(s["handed"] for s in on) == 0, brief(on)
    for k in range(8):
        assert_same(got[k], want, ("oracle", k))


@gpu
def test_long_normals_are_handed_over_under_the_hook(pta, monkeypatch):
    """wall=True with PT_B1_LEAN_TEST_FORCE: every plain fused launch of bounces 1 and 2 is lean, counts or no counts, once the
    hits are loaded (the frame that stores them lists rays for k_wf_trace_exact in its shade passes: general) - and the list
    pass shades what the switched-off run defers: the slab's surfaces, in every frame."""
    case, scene, prof = lean_scene(pta, wall=True)
    schedule(monkeypatch, "default")
    on, off, _ = both(pta, monkeypatch, scene, prof, 8, "wall forced", forced=True)
    assert all(s["general"] == 0 for s in on[2:]) and sum(s["lean1"] for s in on) >= 4 and sum(s["lean2"] for s in on) >= 4, brief(on)
    assert on[2]["planned"] == 0 and on[2]["lean1"], brief(on)   # (an unplanned frame: the hook alone)
    assert on[-1]["handed"] > 0 and on[-1]["handed"] == off[-1]["deferred1"] + off[-1]["deferred2"], (on[-1], off[-1])


@gpu
def test_long_normals_and_the_share_rule(pta, monkeypatch):
    """wall=True without the hook: the 1/64 rule decides per bounce, from the counts of the frame before (steady frames: the
    same every frame) - asserted from the switched-off run's counts, whichever way it goes."""
    case, scene, prof = lean_scene(pta, wall=True)
    schedule(monkeypatch, "default")
    on, off, _ = both(pta, monkeypatch, scene, prof, 9, "wall")
    for k in (7, 8):
        for b in (1, 2):
            deferred, shaded = off[k - 1][f"deferred{b}"], off[k - 1][f"deferred{b}"] + off[k - 1][f"inlined{b}"]
            assert off[k - 1]["planned"] == 1 and off[k - 2] == off[k - 1], brief(off)
            assert bool(on[k][f"lean{b}"]) == (deferred * SHARE < shaded), (k, b, deferred, shaded, brief(on))


def edit_of(pta, case, edit):
    def apply(g):
        if edit == "light-move":
            g.set_lights(lean_lights(pta, first_at=(-0.8, 2.9, 0.4)))
        elif edit == "material":
            other = sb.case_materials(case, pta)
            for m in other:
                m.roughness = min(1.0, 0.37 + 0.5 * m.roughness)
            g.set_materials(other)
        else:
            g.set_camera(sb.make_camera(pta, eye=(-0.9, 2.1, 2.9), target=(0.3, 0.3, -0.4), fov=0.8))
    return apply


@gpu
def test_a_light_move_under_the_hook_hands_everything_over(pta, monkeypatch):
    """The first fused launches behind a moved light find a plane that was zeroed for the new key: every bit unknown, no
    light added here, every shaded entry handed over - and the frame is the frame of the switched-off run."""
    case, scene, prof = lean_scene(pta)
    schedule(monkeypatch, "default")
    on, off, got = both(pta, monkeypatch, scene, prof, 11, "light-move forced", edits={6: edit_of(pta, case, "light-move")}, forced=True)
    k = next(k for k in range(6, 11) if on[k]["lean1"])
    assert off[k]["inlined1"] == 0 and off[k]["deferred1"] > 0 and on[k]["handed"] == off[k]["deferred1"] + off[k]["deferred2"], (k, on[k], off[k])
    assert not np.array_equal(got[5][1], got[10][1])


@gpu
@pytest.mark.parametrize("edit", ["light-move", "material", "camera"])
def test_an_edit_ends_it_and_a_counted_frame_brings_it_back(pta, monkeypatch, edit):
    """Seven frames (lean by then), the edit, seven more: the frame behind the edit is a first frame and general, the bounces
    stay general until a planned frame has been counted under the new state, then they are lean again."""
    case, scene, prof = lean_scene(pta)
    schedule(monkeypatch, "default")
    on, off, got = both(pta, monkeypatch, scene, prof, 14, edit, edits={7: edit_of(pta, case, edit)})
    assert on[6]["lean1"] and on[6]["lean2"], brief(on)
    assert on[7]["lean1"] == on[7]["lean2"] == 0 and on[7]["planned"] == 0, brief(on)
    back = first_lean(on, 7)
    assert back is not None and back >= 9 and all(s["lean1"] and s["lean2"] for s in on[back + 1:]), (edit, back, brief(on))
    assert not np.array_equal(got[6][1], got[13][1]), edit


@gpu
def test_a_frame_in_several_chunks(pta, monkeypatch):
    """1056 x 768 x 4 items, two bounces, queue budgets that leave the planned frame in chunks of 1 Mi items: several lean
    launches and list passes a frame on one list, the last chunk partial."""
    case, scene, _ = lean_scene(pta, wall=True)
    prof = pta.Profile.make(1056, 768, SPP, 2, "FILMIC")
    schedule(monkeypatch, "after-0")
    monkeypatch.setenv("PT_QUEUE_GIB", "0.01")
    monkeypatch.setenv("PT_QUEUE_STEADY_GIB", "0.02")
    monkeypatch.setenv("PT_QUEUE_ONE_PASS_GIB", "0.02")
    on, off, _ = both(pta, monkeypatch, scene, prof, 6, "chunks", forced=True)
    assert on[-1]["lean1"] >= 3 and on[-1]["lean2"] >= 3 and on[-1]["handed"] > 0, brief(on)


@gpu
def test_two_shards(pta, monkeypatch):
    """shard_count = 2, 16 x 16 tiles: every rank a scene, a plan and an eligibility of its own."""
    case, scene, prof = lean_scene(pta)
    schedule(monkeypatch, "default")
    for rank in range(2):
        o = pta.Opts.make(shard_rank=rank, shard_count=2, tile_w=16, tile_h=16)
        on, _, _ = both(pta, monkeypatch, scene, prof, 8, ("rank", rank), opts=o)
        k = first_lean(on)
        assert k is not None and all(s["lean1"] for s in on[k:]), (rank, brief(on))


@gpu
@pytest.mark.parametrize("name", ["after-0", "after-1", "after-4", "no-masks"])
def test_masks_that_arrive_late_or_never(pta, monkeypatch, name):
    """PT_ESCAPE_AFTER = 0, 1, 4 and PT_ESCAPE=0: new masks change the signature - general until counted again - and the
    frames are the switched-off run's whenever they arrive."""
    case, scene, prof = lean_scene(pta)
    schedule(monkeypatch, name)
    on, _, _ = both(pta, monkeypatch, scene, prof, 10, name)
    assert all(s["lean1"] and s["lean2"] for s in on[-2:]), (name, brief(on))


@gpu
@pytest.mark.parametrize("b0, b1", [("0", "1"), ("1", "0")])
def test_the_two_lean_switches_are_independent(pta, monkeypatch, b0, b1):
    """PT_B0_LEAN=0 with PT_B1_LEAN=1 and the reverse: each variant follows its own switch."""
    case, scene, prof = lean_scene(pta)
    schedule(monkeypatch, "default")
    monkeypatch.setenv("PT_B0_LEAN", b0)
    monkeypatch.setenv("PT_B1_LEAN", b1)
    g = pta.GpuScene(scene)
    frames = [g.render(prof) for _ in range(8)]
    s, s0 = stats(g), g.b0_lean_stats()
    g.close()
    assert (s["lean1"] > 0 and s["lean2"] > 0) == (b1 == "1") and (s0[0] > 0) == (b0 == "1"), (s, s0)
    monkeypatch.setenv("PT_B0_LEAN", "0")
    monkeypatch.setenv("PT_B1_LEAN", "0")
    g = pta.GpuScene(scene)
    for k in range(8):
        assert_same(frames[k], g.render(prof), (b0, b1, k))
    g.close()


@gpu
@pytest.mark.parametrize("kind", ["translucent", "directional", "counting", "no-grids"])
def test_frames_that_never_go_lean(pta, monkeypatch, kind):
    """A translucent table keys no cache, a directional light compiles the orthographic branch in, a counting frame and a
    frame without grids take k_wf_shade: no lean launch even under the hook, and identical frames."""
    opts = None
    if kind == "directional":
        lights = lean_lights(pta)[:2] + [sb._light(pta, pta.PT_LIGHT_DIRECTIONAL, 10.0 * sb._unit([-0.3, -0.9, -0.25]), (0.5, 0.6, 0.7))]
        case, scene, prof = lean_scene(pta, lights=lights)
    elif kind == "translucent":
        case, scene, prof = lean_scene(pta, factor_set="alpha")
        assert scene.translucent
    else:
        case, scene, prof = lean_scene(pta)
    if kind == "counting":
        opts = pta.Opts.make(flags=pta.PT_FLAG_COUNTERS)
    elif kind == "no-grids":
        opts = pta.Opts.make(flags=pta.PT_FLAG_NO_GRIDS)
    schedule(monkeypatch, "default")
    on, _, _ = both(pta, monkeypatch, scene, prof, 7, kind, opts=opts, forced=True)
    assert sum(s["lean1"] + s["lean2"] for s in on) == 0, (kind, brief(on))


SORT_CHILD = r"""
import hashlib, json, sys
import numpy as np
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(root)r + "/tests")
import __graft_entry__ as e
pta = e.load_package()
from test_bounce0_lean import lean_scene
case, scene, prof = lean_scene(pta)
g = pta.GpuScene(scene)
shas = []
for frame in range(7):
    rgb, acc = g.render(prof)
    shas.append(hashlib.sha1(np.ascontiguousarray(rgb, np.uint8).tobytes() + np.ascontiguousarray(acc, np.float32).tobytes()).hexdigest())
print("RESULT", json.dumps({"shas": shas, "lean": list(map(int, g.b1_lean_stats()))}))
"""


@gpu
def test_a_sorting_frame_never_goes_lean(pta, monkeypatch):
    """PT_WF_SORT=1 (read once per process: a child), under the hook: a sorting frame takes k_wf_shade at every bounce, so no
    fused launch, lean or general; sorting changes no bit, so the frames are those of this process with the switch off."""
    import hashlib
    import json
    import os
    import subprocess
    import sys
    from pathlib import Path
    root = Path(__file__).resolve().parent.parent
    case, scene, prof = lean_scene(pta)
    schedule(monkeypatch, "default")
    ref, _ = sequence(pta, monkeypatch, scene, prof, 7, "0")
    want = [hashlib.sha1(np.ascontiguousarray(r[0], np.uint8).tobytes() + np.ascontiguousarray(r[1], np.float32).tobytes()).hexdigest() for r in ref]
    env = {k: v for k, v in os.environ.items() if not k.startswith(("PT_WF_", "PT_B1_", "PT_ESCAPE"))}
    env.update(PT_WF_SORT="1", PT_B1_LEAN="1", PT_B1_LEAN_TEST_FORCE="1")
    run = subprocess.run([sys.executable, "-c", SORT_CHILD % {"root": str(root)}], env=env, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    res = json.loads([ln for ln in run.stdout.splitlines() if ln.startswith("RESULT ")][0][7:])
    print(res)
    assert res["shas"] == want and res["lean"] == [0, 0, 0, 0], res
