"""Steady frames of textured and normal-mapped scenes.  A scene's fourth frame and every frame behind it run other kernels
than its first: the loading bounce-0 launch with its LDS parking (k_wf_shade_hits<2283>), its LEAN variant (<6379>), the
fused pass of bounces 1 and 2 (k_wf_shade_fused<256>), its LEAN1 variant (<8448>) with the list pass HAND (<16640>), the
fused tail bounces, and the continuation cache, which replays a STORED sampled direction and throughput.  All of their values
come out of material_sample, shading_normal and ct_init - and the feature matrix (tests/scene_builder.py cases()) renders
every (profile, opts) pair once before the key changes, while every test that does drive a scene into its steady state
builds it with tex_kind="none".  So no parked, late-record, cached-continuation, lean or handed-over code path was ever run
on a surface with an emissive, metalness, roughness or normal texture, and on an opaque scene that can go steady none on an
albedo texture either.

What could go wrong and stay unseen behind material constants: a lean variant that reads a material factor where the
textured sample belongs, a parking slot that brings back the geometric normal in place of the mapped one or drops a field
of the BRDF, a continuation stored before a texture-only edit and loaded behind it, a list pass that samples at a stale uv.

Two scenes, both under the factor set `mirror` (under `opaque` every mesh material has metalness 0 and a metalness texture -
a factor times a texel - changes no bit):
  lean  test_bounce0_lean's scene (404 triangles and the ball, every normal of length one, three point lights), 70 x 38 x 4,
        3 bounces: the scene that goes lean at bounce 0, 1 and 2;
  room  scene_builder's closed metal box (12 triangles and the ball) under the point light, 64 x 40 x 4, 6 bounces: paths that
        are alive at bounces 3-6 (6.7 segments a sample without a texture).
Six opaque kinds: each texture alone and `five` - tex_kind "all" without the opacity textures.  Every frame sent to a GPU is
walked on the CPU first (every ray finite, numeric_errors == 0) and every GPU frame equals the oracle's bit for bit, rgb8 and
f32 accumulator; what a sequence covered is asserted from the launch statistics of each of its frames, which it prints as a
table (profiles/steady_textured.txt)."""
import numpy as np
import pytest

import scene_builder as sb
from test_bounce0_lean import lean_scene
from test_masked_sequences import schedule, shared
from test_prestaged_misses import assert_same, bits, oracle_frame

gpu = pytest.mark.gpu

KINDS = ("albedo", "emissive", "metalness", "roughness", "normal", "five")
DEEP = KINDS[:4]   # room: the kinds whose paths live on (a random normal map turns half the normals below the horizon)
SCENES = ("lean", "room")
ROOM = sb.Case("steady-room", "room", "none", "point", "mirror", 6, "FILMIC", 0, False)
ROOM_SIZE = (64, 40, 4)
FRAMES = 10

HITS = ("resets", "stores", "loads", "unknown")
COLUMNS = (["planned", "b0_lean", "b0_general", "b0_guard", "lean1", "lean2", "b1_general", "handed", "hit_stores", "hit_loads",
            "vis_resets", "vis_launches", "cont_stores", "cont_loads", "cont_missing", "h1f_launches"]
           + [f"{n}{b}" for b in (1, 2, 3, 4) for n in ("fused", "inlined", "deferred")]
           + [f"{n}{b}" for b in (1, 2, 3, 4, 5) for n in ("stores", "loads", "unknown")])


# -------------------------------------------------------------------------------------------------------------------------
# tables, scenes, oracle frames
# -------------------------------------------------------------------------------------------------------------------------
def table(pta, kind, size_shift=0):
    """The material table of a kind under `mirror`: "none", one of the texture kinds, "five" (all but opacity), "all"."""
    tex_kind = "all" if kind == "five" else kind
    mats = sb.case_materials(ROOM._replace(tex_kind=tex_kind, factor_set="mirror", size_shift=size_shift), pta)
    if kind == "five":
        for m in mats:
            m.tex_opacity = -1
    return mats


def make(pta, name, kind, bounces=None, wall=False, size_shift=0):
    """(scene, profile) of `lean` / `room` with the table of `kind`."""
    mats = table(pta, kind, size_shift)
    if name == "lean":
        _, scene, prof = lean_scene(pta, materials=mats, wall=wall)
        if bounces is not None:
            prof = pta.Profile.make(prof.width, prof.height, prof.samples, bounces, "FILMIC")
        return scene, prof
    w, h, spp = ROOM_SIZE
    return sb.build(ROOM, pta=pta, materials=mats), sb.profile(ROOM, w, h, spp, bounces=bounces, pta=pta)


def want_of(pta, oracle, name, kind, bounces=None, walk=True, **kw):
    """The oracle's frame of (scene, kind), walked first; made once per session, shared and left unchanged."""
    def frame():
        scene, prof = make(pta, name, kind, bounces, **kw)
        return oracle_frame(oracle, scene, prof, walk=walk)
    return shared(("steady-textured", name, kind, bounces, walk, tuple(sorted(kw.items()))), frame)


def changed(a, b):
    """Share of the pixels whose accumulator differs bit-wise."""
    return float((bits(a[1]) != bits(b[1])).any(axis=1).mean())


# -------------------------------------------------------------------------------------------------------------------------
# statistics of a live scene
# -------------------------------------------------------------------------------------------------------------------------
def snapshot(g):
    d = dict(zip(("b0_lean", "b0_general", "b0_guard"), g.b0_lean_stats()))
    d.update(zip(("lean1", "lean2", "b1_general", "handed"), g.b1_lean_stats()))
    hit, vis, cont = g.hit_cache_stats(), g.vis_cache_stats(), g.cont_cache_stats()
    d.update(hit_stores=hit[3], hit_loads=hit[4], vis_resets=vis[2], vis_launches=vis[3],
             cont_stores=cont[4], cont_loads=cont[5], cont_missing=cont[6], h1f_launches=g.hit1_fused_stats()[0])
    for b in (1, 2, 3, 4):
        f = g.bounce_fused_stats(b)
        d[f"fused{b}"], d[f"inlined{b}"], d[f"deferred{b}"] = f[0], f[1], f[2]
    for b in (1, 2, 3, 4, 5):
        d.update(zip((f"{n}{b}" for n in HITS), g.bounce_hits_cache_stats(b)[3:7]))
    return d


def run(pta, monkeypatch, scene, prof, frames, edits=None, env=None, opts=None):
    """`frames` frames of a fresh GpuScene under the default schedule; edits: {frame: function(g)} applied before that frame;
    env: switches set before the scene is made.  Returns per frame (rgb8, accum) and what that frame alone added to every
    count, with its plan flag and has_translucent."""
    schedule(monkeypatch, "default")
    for k in ("PT_B0_LEAN", "PT_B1_LEAN", "PT_B0_LEAN_TEST_FORCE", "PT_B1_LEAN_TEST_FORCE"):
        monkeypatch.delenv(k, raising=False)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    g = pta.GpuScene(scene)
    out, seen, before = [], [], snapshot(g)
    for k in range(frames):
        if edits and k in edits:
            edits[k](g)
        out.append(g.render(prof, opts) if opts is not None else g.render(prof))
        now = snapshot(g)
        d = {key: now[key] - before[key] for key in now}
        info = g.info()
        d["planned"], d["translucent"] = int(info.frame_planned), int(info.has_translucent)
        seen.append(d)
        before = now
    g.close()
    return out, seen


def show(what, seen):
    """The per-frame table: one row per frame, the columns that are zero in every frame left out."""
    cols = [c for c in COLUMNS if any(s[c] for s in seen)]
    print(f"STEADY {what}")
    print("STEADY    frame " + " ".join(cols))
    for k, s in enumerate(seen):
        print(f"STEADY    {k:5d} " + " ".join(str(s[c]).rjust(len(c)) for c in cols))


_runs = {}


def steady(pta, oracle, monkeypatch, name, kind):
    """The ten-frame sequence of (scene, kind), rendered once per session: (frames, per-frame statistics, the oracle's frame)."""
    if (name, kind) not in _runs:
        want = want_of(pta, oracle, name, kind)
        scene, prof = make(pta, name, kind)
        assert not scene.translucent
        _runs[(name, kind)] = "the sequence was started and did not end"   # (a sequence that failed is not rendered again)
        try:
            out, seen = run(pta, monkeypatch, scene, prof, FRAMES)
        except Exception as err:
            _runs[(name, kind)] = f"the sequence failed: {err!r}"
            raise
        show(f"{name}/{kind}", seen)
        _runs[(name, kind)] = (out, seen, want)
    assert isinstance(_runs[(name, kind)], tuple), _runs[(name, kind)]
    return _runs[(name, kind)]


# -------------------------------------------------------------------------------------------------------------------------
# the same sequences with the shadow casts of bounces >= 1 kept out of the shade kernel
# -------------------------------------------------------------------------------------------------------------------------
# The frame plan puts a bounce's shadow casts inside k_wf_shade where it counted shadow records for 60 % of the bounce's
# queue (make_plan, PT_OG_INLINE_AUTO) - and then that bounce has no fused pass, general or lean.  An emissive surface's
# light term is never exactly 0, so every hit of it writes a record: in the closed `room` every kind but `normal` (whose
# turned normals make half the lights moot) is planned inline at every bounce, and so is `five` on `lean`, whose mapped
# normals send two of three bounce-1 rays back into the scene (1 620 of 2 467 hit, 136 of 169 at bounce 2; without a normal
# map 431 of 4 368 - the oracle's counts).  Their planned frames run k_wf_shade<grid 1> behind loaded
# hits; the fused passes on those tables are reached with PT_OG_INLINE_AUTO=0, which is read once per process: one child
# process renders all of these sequences, the list-pass pair of test 4 among them.
INLINED_BY_THE_PLAN = (("lean", "five"),) + tuple(("room", k) for k in KINDS if k != "normal")
FORCED = {"PT_B1_LEAN": "1", "PT_B1_LEAN_TEST_FORCE": "1"}
CHILD_JOBS = {f"{name}/{kind}": (name, kind, False, FRAMES, {}) for name, kind in INLINED_BY_THE_PLAN}
CHILD_JOBS["wall/off"] = ("lean", "five", True, 8, {"PT_B1_LEAN": "0"})
CHILD_JOBS["wall/forced"] = ("lean", "five", True, 8, FORCED)

CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(root)r + "/tests")
import __graft_entry__ as e
import test_steady_textured as t
pta = e.load_package()
out = {}
for key, (name, kind, wall, frames, env) in t.CHILD_JOBS.items():
    scene, prof = t.make(pta, name, kind, wall=wall)
    got, seen = t.run(pta, t.ProcessEnv(), scene, prof, frames, env=env)
    out[key + " seen"] = np.frombuffer(repr(seen).encode(), np.uint8)
    out[key + " rgb8"] = np.stack([f[0] for f in got])
    out[key + " accum"] = np.stack([f[1] for f in got])
np.savez(%(out)r, **out)
print("RESULT written")
"""


class ProcessEnv:
    """monkeypatch's two calls on the process's own environment (the child has no monkeypatch and ends with its changes)."""

    def setenv(self, k, v):
        import os
        os.environ[k] = v

    def delenv(self, k, raising=True):
        import os
        os.environ.pop(k, None)


def without_inline_casts(pta, oracle):
    """{job: {"frames": [(rgb8, accum)], "seen", "want"}} of CHILD_JOBS under PT_OG_INLINE_AUTO=0, rendered by one child
    process, once per session.  Every job's frame is walked on the CPU before the child starts, whichever test asks first;
    the child's outcome is kept, a failure too: a child that failed is not started again, every later caller fails from
    what the first one saw."""
    if "child" not in _runs:
        import ast
        import os
        import subprocess
        import sys
        import tempfile
        from pathlib import Path
        wants = {key: want_of(pta, oracle, name, kind, wall=wall) for key, (name, kind, wall, _, _) in CHILD_JOBS.items()}
        root = Path(__file__).resolve().parent.parent
        env = {k: v for k, v in os.environ.items() if not k.startswith(("PT_WF_", "PT_B0_", "PT_B1_", "PT_ESCAPE", "PT_OG_", "PT_TAIL_"))}
        env["PT_OG_INLINE_AUTO"] = "0"
        _runs["child"] = "the child process was started and did not come back"
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "frames.npz")
            try:
                res = subprocess.run([sys.executable, "-c", CHILD % {"root": str(root), "out": path}], env=env,
                                     capture_output=True, text=True, timeout=300)
            except subprocess.TimeoutExpired as err:
                _runs["child"] = f"the child process did not end in {err.timeout} s"
            else:
                if res.returncode != 0 or "RESULT written" not in res.stdout:
                    _runs["child"] = f"the child process ended with {res.returncode}: {res.stderr[-2000:]}"
                else:
                    with np.load(path) as z:
                        _runs["child"] = {key: {"frames": list(zip(z[key + " rgb8"], z[key + " accum"])), "want": wants[key],
                                                "seen": ast.literal_eval(z[key + " seen"].tobytes().decode())} for key in CHILD_JOBS}
                    for key, r in _runs["child"].items():
                        show(f"{key} PT_OG_INLINE_AUTO=0 {CHILD_JOBS[key][4]}", r["seen"])
    assert isinstance(_runs["child"], dict), _runs["child"]
    return _runs["child"]


def fused_runs(pta, oracle, monkeypatch, name, kind):
    """The statistics in which the fused passes of (scene, kind) are looked for: the default sequence's - which must then
    have none in a planned frame, or the reason above no longer holds - and the child's, or the default sequence's alone."""
    _, seen, _ = steady(pta, oracle, monkeypatch, name, kind)
    if (name, kind) not in INLINED_BY_THE_PLAN:
        return seen
    assert all(s["fused1"] == s["fused2"] == 0 for s in seen if s["planned"]), (name, kind, "no longer planned inline")
    return without_inline_casts(pta, oracle)[f"{name}/{kind}"]["seen"]


# -------------------------------------------------------------------------------------------------------------------------
# 1. the inputs can see what they test (CPU)
# -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", SCENES)
def test_the_inputs_can_see_what_they_test(pta, oracle, name, kind):
    """No GPU.  The table is opaque, the frame walks clean, the texture reaches the image - 0.35 of the pixels of `lean` (its
    hit pixels are 0.405-0.423 of the frame: the bound is that share less a margin), every pixel of the closed `room` - and
    the later bounces reach it too: some pixel of `lean` between depth 1 and 3, 0.9 of the pixels of `room` between depth 2
    and 6 for the four kinds with deep paths.  Conditions on the inputs: if a kind stops meeting one, the input changes."""
    scene, prof = make(pta, name, kind)
    assert not scene.translucent and not make(pta, name, "none")[0].translucent
    want = want_of(pta, oracle, name, kind)
    none = want_of(pta, oracle, name, "none")
    assert want[2]["numeric_errors"] == 0 and not np.isnan(want[1]).any()
    share = changed(want, none)
    per_sample = want[2]["segments"] / (prof.width * prof.height * prof.samples)
    print(f"STEADY input {name}/{kind}: {share:.3f} of the pixels differ from `none`, {per_sample:.2f} segments a sample")
    if name == "lean":
        assert share >= 0.35, (kind, share)
        shallow = want_of(pta, oracle, name, kind, bounces=1, walk=False)   # (its paths are prefixes of the walked ones)
        assert changed(want, shallow) > 0.0, kind
    else:
        assert share == 1.0, (kind, share)
        if kind in DEEP:
            shallow = want_of(pta, oracle, name, kind, bounces=2, walk=False)
            deep = changed(want, shallow)
            print(f"STEADY input {name}/{kind}: {deep:.3f} of the pixels differ between depth 2 and 6")
            assert deep >= 0.9, (kind, deep)
        # a ray at bounce 5, which test_room_reaches_the_tail_bounces wants loaded: every kind but `five`, whose last
        # seven paths end at bounce 4 (ROOM_HIT_BOUNCES)
        rays = [want_of(pta, oracle, name, kind, bounces=b, walk=False)[2]["segments"] for b in (4, 5)]
        print(f"STEADY input {name}/{kind}: {rays[1] - rays[0]} rays at bounce 5")
        assert (rays[1] > rays[0]) == (5 in ROOM_HIT_BOUNCES.get(kind, ROOM_HIT_BOUNCES["other"])), (kind, rays)


# -------------------------------------------------------------------------------------------------------------------------
# 2. steady sequences equal the oracle
# -------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", SCENES)
def test_ten_frames_equal_the_oracle(pta, oracle, monkeypatch, name, kind):
    """A fresh scene, the default schedule, ten frames of one profile: each the oracle's frame bit for bit."""
    out, seen, want = steady(pta, oracle, monkeypatch, name, kind)
    for k in range(FRAMES):
        assert_same(out[k], want, (name, kind, k))


@gpu
@pytest.mark.parametrize("name, kind", INLINED_BY_THE_PLAN)
def test_ten_frames_without_inline_casts_equal_the_oracle(pta, oracle, name, kind):
    """The sequences the plan takes the fused passes from, rendered with PT_OG_INLINE_AUTO=0 (a child process): each of
    the ten frames is the oracle's bit for bit."""
    r = without_inline_casts(pta, oracle)[f"{name}/{kind}"]
    assert len(r["frames"]) == FRAMES
    for k in range(FRAMES):
        assert_same(r["frames"][k], r["want"], (name, kind, "without inline casts", k))


# -------------------------------------------------------------------------------------------------------------------------
# 3. what the sequences covered, from their statistics
# -------------------------------------------------------------------------------------------------------------------------
def some(seen, test):
    return any(test(s) for s in seen)


@gpu
@pytest.mark.parametrize("kind", KINDS)
def test_lean_reaches_every_steady_variant(pta, oracle, monkeypatch, kind):
    """`lean`, per kind, in some frame of the ten: (a) a general loading bounce-0 launch, (b) a lean one, and the last two
    frames lean, (c) continuation-loading launches, (d) lights added by a general fused launch at bounce 1, (e) a lean launch
    at bounce 1 and one at bounce 2, (f) the guard silent throughout - the states test_bounce0_lean and test_bounce1_lean
    assert of the untextured scene.  (d) and (e) of `five`: in the sequence without inline casts."""
    _, seen, _ = steady(pta, oracle, monkeypatch, "lean", kind)
    assert some(seen, lambda s: s["hit_loads"] > 0 and s["b0_general"] > 0), (kind, "a")
    assert some(seen, lambda s: s["b0_lean"] > 0), (kind, "b")
    assert all(s["b0_lean"] > 0 and s["b0_general"] == 0 for s in seen[-2:]), (kind, "b, the last two frames")
    assert some(seen, lambda s: s["cont_loads"] > 0), (kind, "c")
    assert all(s["cont_missing"] == 0 and s["b0_guard"] == 0 for s in seen), (kind, "c, f")
    fused = fused_runs(pta, oracle, monkeypatch, "lean", kind)
    assert some(fused, lambda s: s["b1_general"] > 0 and s["inlined1"] > 0), (kind, "d")
    assert some(fused, lambda s: s["lean1"] > 0) and some(fused, lambda s: s["lean2"] > 0), (kind, "e")
    assert all(s["lean1"] > 0 and s["lean2"] > 0 and s["b1_general"] == 0 for s in fused[-2:]), (kind, "e, the last two frames")
    assert all(s["b0_guard"] == 0 and s["cont_missing"] == 0 for s in fused), (kind, "f")


@gpu
@pytest.mark.parametrize("kind", KINDS)
def test_room_reaches_the_tail_bounces(pta, oracle, monkeypatch, kind):
    """`room`, per kind: loading launches of the hit planes of the bounces that have a ray (ROOM_HIT_BOUNCES) in planned
    frames, a record for every cast, a lean bounce-0 launch - and, in the sequence without inline casts for every kind but
    `normal`: lights added by the fused pass at each of bounces 1-4, lean launches at bounces 1 and 2.  `normal` and `five`
    have 1.6 segments a sample where the others have 5.0-6.9, and still a few records at bounces 3 and 4 (`normal`: 8 and 2
    in this frame, `five`: 92 and 7): the fused passes are asked of them like of the others."""
    _, seen, _ = steady(pta, oracle, monkeypatch, "room", kind)
    fused = fused_runs(pta, oracle, monkeypatch, "room", kind)
    for stats in ((seen,) if fused is seen else (seen, fused)):
        for b in ROOM_HIT_BOUNCES.get(kind, ROOM_HIT_BOUNCES["other"]):
            assert some(stats, lambda s: s["planned"] and s[f"loads{b}"] > 0), (kind, "loads", b)
        for b in (1, 2, 3, 4, 5):
            assert all(s[f"unknown{b}"] == 0 for s in stats), (kind, "unknown", b)
        assert all(s["b0_lean"] > 0 for s in stats[-2:]), (kind, "b")
        assert all(s["b0_guard"] == 0 and s["cont_missing"] == 0 for s in stats), kind
    for b in (1, 2, 3, 4):
        assert some(fused, lambda s: s[f"fused{b}"] > 0 and s[f"inlined{b}"] > 0), (kind, "d", b)
    assert some(fused, lambda s: s["lean1"] > 0) and some(fused, lambda s: s["lean2"] > 0), (kind, "e")


# The bounces of `room` whose hit plane a planned frame loads.  `five` has no ray at bounce 5 (10 240, 5 445, 1 293, 92 and 7
# rays at bounces 0-4, all seven of the last end there; test_the_inputs_can_see_what_they_test holds the premise): its bounce-5
# plane is keyed and marked full without a storing launch, a planned frame leaves the bounces behind its last ray out, and
# the one loading launch the statistics show at bounce 5 is the unplanned frame 2's, which launches every bounce, on an empty
# queue.  `normal` has two rays there, the other kinds thousands.
ROOM_HIT_BOUNCES = {"five": (1, 2, 3, 4), "other": (1, 2, 3, 4, 5)}


# -------------------------------------------------------------------------------------------------------------------------
# 4. the list pass on textured, normal-mapped records
# -------------------------------------------------------------------------------------------------------------------------
@gpu
def test_the_list_pass_shades_textured_records(pta, oracle):
    """`lean` with terrace's slab (vertex normals of length 4 and 0.5: records the lean pass hands over in every frame) and
    the table `five`, under PT_B1_LEAN_TEST_FORCE, eight frames (in the child without inline casts: `five` on `lean` is
    planned inline): entries are handed over in lean frames, every frame is the oracle's and the frame of the same sequence
    under PT_B1_LEAN=0, with the same fused statistics - the one run of HAND on a normal-mapped, textured record."""
    scene, _ = make(pta, "lean", "five", wall=True)
    assert not scene.translucent and scene.n_triangles == 406
    child = without_inline_casts(pta, oracle)
    off, on = child["wall/off"]["seen"], child["wall/forced"]["seen"]
    assert len(child["wall/forced"]["frames"]) == len(child["wall/off"]["frames"]) == 8
    for k in range(8):
        assert_same(child["wall/forced"]["frames"][k], child["wall/forced"]["want"], ("oracle", k))
        assert_same(child["wall/forced"]["frames"][k], child["wall/off"]["frames"][k], ("switched off", k))
        a, b = on[k], off[k]
        assert b["lean1"] == b["lean2"] == b["handed"] == 0, (k, b)
        assert a["lean1"] + a["lean2"] + a["b1_general"] == b["b1_general"] and a["planned"] == b["planned"], (k, a, b)
        for bounce in (1, 2):
            for n in ("fused", "inlined", "deferred"):
                assert a[f"{n}{bounce}"] == b[f"{n}{bounce}"], (k, n, bounce, a, b)
        # a lean launch hands over exactly the records the general pass defers; a general launch hands over nothing
        assert a["handed"] == sum(b[f"deferred{bounce}"] for bounce in (1, 2) if a[f"lean{bounce}"]), (k, a, b)
    assert all(s["b1_general"] == 0 for s in on[2:]) and sum(s["lean1"] for s in on) >= 4 and sum(s["lean2"] for s in on) >= 4, on
    # steady frames: the visibility is known, what is handed over is the slab's long normals - and lights are added beside it
    assert all(s["lean1"] and s["lean2"] and s["handed"] > 0 and s["inlined1"] > 0 for s in on[-2:]), on[-2:]


# -------------------------------------------------------------------------------------------------------------------------
# 5. edits that change textures only, while lean
# -------------------------------------------------------------------------------------------------------------------------
# name -> the tables in order: (kind, size_shift, frames).  Six frames, the edit, seven more; `five-all-five`: four frames
# translucent, then seven more, so that the opaque table has the frames to go lean again.
EDITS = {"roughness-moved": (("roughness", 0, 6), ("roughness", 1, 7)),
         "none-normal": (("none", 0, 6), ("normal", 0, 7)),
         "normal-none": (("normal", 0, 6), ("none", 0, 7)),
         "five-all-five": (("five", 0, 6), ("all", 0, 4), ("five", 0, 7))}


@gpu
@pytest.mark.parametrize("edit", list(EDITS))
def test_a_texture_only_edit_while_lean(pta, oracle, monkeypatch, edit):
    """set_materials with tables that differ in texture indices alone - the roughness textures moved to other textures of
    the same channel count, a normal map arriving and leaving, the opacity textures arriving (the scene turns translucent:
    the caches go, the ALPHA variants take over) and leaving.  Every frame is the oracle's frame of the scene as edited at
    that moment; the frame behind an edit is not planned and has no lean launch; the lean launches are there before the edit
    and back by the end of every opaque stretch, and there is none while translucent; the image changed across the edit."""
    steps = EDITS[edit]
    scene, prof = make(pta, "lean", steps[0][0], size_shift=steps[0][1])
    wants, edits, first = [], {}, 0
    for kind, shift, n in steps:
        want = want_of(pta, oracle, "lean", kind, size_shift=shift)
        if first:
            edits[first] = lambda g, kind=kind, shift=shift: g.set_materials(table(pta, kind, shift))
        wants += [want] * n
        first += n
    out, seen = run(pta, monkeypatch, scene, prof, first, edits=edits)
    show(f"edit {edit}", seen)
    for k in range(first):
        assert_same(out[k], wants[k], (edit, k))
    # (`five` on `lean` is planned inline at bounces 1 and 2 - INLINED_BY_THE_PLAN: its lean launches are bounce 0's)
    lean = lambda s, kind: s["b0_lean"] > 0 and (kind == "five" or (s["lean1"] > 0 and s["lean2"] > 0))
    any_lean = lambda s: s["b0_lean"] + s["lean1"] + s["lean2"] > 0
    assert all(s["b0_guard"] == 0 and s["cont_missing"] == 0 for s in seen), edit
    at = 0
    for i, (kind, shift, n) in enumerate(steps):
        stretch = seen[at:at + n]
        assert all(s["translucent"] == (kind == "all") for s in stretch), (edit, i, [s["translucent"] for s in stretch])
        if i:
            assert stretch[0]["planned"] == 0 and not any_lean(stretch[0]), (edit, i, stretch[0])
            assert changed(out[at - 1], out[at]) > 0.0, (edit, i)
        if kind == "all":
            assert not any(any_lean(s) for s in stretch), (edit, i)
            assert all(s["hit_loads"] == s["cont_loads"] == s["loads1"] == 0 for s in stretch), (edit, i)
        else:
            assert lean(stretch[-1], kind), (edit, i, stretch[-1])
        at += n


# -------------------------------------------------------------------------------------------------------------------------
# 6. the other two pipelines
# -------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name, kind", [("lean", "five"), ("room", "roughness")])
def test_the_kd_pipeline_and_the_megakernel_render_the_same_frames(pta, oracle, name, kind):
    """PT_FLAG_NO_GRIDS and PT_FLAG_MEGAKERNEL have no steady variants: one frame each against the oracle frames of the
    sequences above - the three-pipeline convention of the matrix, on these scenes."""
    want = want_of(pta, oracle, name, kind)
    scene, prof = make(pta, name, kind)
    g = pta.GpuScene(scene)
    for flags in (pta.PT_FLAG_NO_GRIDS, pta.PT_FLAG_MEGAKERNEL):
        assert_same(g.render(prof, pta.Opts.make(flags=flags)), want, (name, kind, flags))
    g.close()
