"""The KD-tree walkers on deep and on tiny trees.

The bit-exact cast tests of tests/test_geometry_model.py run on two scenes whose rays never hold more than 11 pending far
children, so the halves of stack_push / stack_get behind WF_LDS_STACK (csrc/pt_wavefront.h), the ov_* arrays of
k_wf_trace_exact behind WF_EXACT_LDS_STACK, a trav_enter that pushes across that limit and the trees smaller than the
WF_LDS_NODES slots staged in LDS were executed by no test that compares results.  Here:

  * tests/kd_shape_scenes.py makes a NEST whose tree is a chain of ~59 levels (and 25 under the default builder settings), in
    two orientations, nested boxes whose entry lists reach 53 entries, and TINY scenes;
  * tests/kd_walk_model.py certifies on the CPU what the rays REACH (stack heights, the height an accepted hit's leaf is
    popped from, entry-list lengths), every condition against constants read from the headers with a margin of 2;
  * expected values come from tests/geometry_model.py (brute force, f32) and the oracle, never from a walk.

Measured (CPU, the model's walk; deep build = PT_KD_MAX_LEAF=1 PT_KD_MAX_DEPTH=62; per orientation, 5 classes of 2 048 rays):
  nest, deep build     depth 59, 713 nodes; 4 357 rays reach >= 18 and 3 067 reach >= 40 (the outward rays hold 39 - 47); 945
                       accepted hits (941 at the maximum corner) lie in a leaf popped from >= 16; 1 273 near-axis rays reach
                       >= 18; all 32 alternating blocks hold heights <= 12 and >= 16
  nest, default build  depth 25, 111 nodes; 1 729 rays (1 739) reach 16 - 18
  entry lists          the nest: 0 - 14 entries, 8 and 9 among them.  Nested boxes (dolls_scene, 244 primitives, deep build:
                       depth 62): 142 primitives with lists above 16 entries, 38 above 40, the longest 53
  escape masks         built on the nest shrunk to a box of 4 (same tree); in the box of 2^30 the builder declines every primitive
"""
import os

import numpy as np
import pytest

import geometry_model as gm
import kd_shape_scenes as ks
import kd_walk_model as kw
from test_geometry_model import bits, same_records

MAX_HITS = 16
CORNERS = ("min", "max")
BUILDS = {"default": {}, "deep": ks.DEEP_ENV}
NEST_KEYS = [(c, b) for c in CORNERS for b in BUILDS]
SLOT_LABELS = {"below": kw.WF_LDS_NODES - 2, "at": kw.WF_LDS_NODES, "above": kw.WF_LDS_NODES + 2}   # device node slots
TINY_NAMES = ("one-triangle", "one-sphere", "root-is-a-leaf", "max-leaf-plus-one", "empty", "slots-below", "slots-at", "slots-above")
TINY_RAYS = 4096
COUNTERS = ("samples", "segments", "shadow_rays", "shaded_hits", "rng_draws")
REFUSAL_ENV = {"PT_KD_MAX_LEAF": "1", "PT_KD_MAX_DEPTH": "70"}


def n_prims_of(scene):
    return gm.flatten(scene["models"])[5] if scene["models"] else 0


def cast_reference(scene, rays):
    if not scene["models"]:
        hits = np.zeros((len(rays), MAX_HITS), gm.HIT_DTYPE)
        hits["prim"] = -1
        return hits, np.zeros(len(rays), np.uint32), np.zeros(len(rays), bool)
    return gm.ray_cast(rays, scene["models"], MAX_HITS)


def origins_strictly_inside(tree, rays):
    o = np.asarray(rays, np.float32)[:, :3]
    return bool(((o > tree.bmin) & (o < tree.bmax)).all())


# ---------------------------------------------------------------------------------------------------------------------
# the scenes, their trees, rays and brute-force answers: made once
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def nests(pta):
    """(corner, build) -> everything about one build of one orientation of the nest.  The builder's variables are set
    around the CPU build only and restored; the GPU tests set them again around the creation of their scene."""
    cache, shared = {}, {}

    def get(corner, build):
        if corner not in shared:
            scene = ks.nest_scene(corner)
            rays, starts, classes = ks.nest_rays(scene)
            hits, counts, aside = cast_reference(scene, rays)
            shared[corner] = dict(scene=scene, rays=rays, starts=starts, classes=classes, hits=hits, counts=counts, keep=~aside)
        if (corner, build) not in cache:
            c = dict(shared[corner])
            c["built"] = ks.built(pta, c["scene"])
            before = dict(os.environ)
            with ks.kd_env(BUILDS[build]):
                c["tree"] = kw.Tree(pta, c["built"])
            assert dict(os.environ) == before
            c["n_prims"] = n_prims_of(c["scene"])
            first = c["hits"][:, 0]
            c["walk"] = kw.walk(c["tree"], c["rays"], c["n_prims"], first["prim"], kw.stop_parameters(c["rays"], first, gm))
            c["home"] = kw.home_depths(c["tree"], c["scene"]["models"], c["scene"]["camera"][0])
            cache[(corner, build)] = c
        return cache[(corner, build)]
    return get


@pytest.fixture(scope="module")
def dolls(pta):
    """build -> the nested boxes (kd_shape_scenes.dolls_scene) under that build, as `nests` gives the nest."""
    cache, shared = {}, {}

    def get(build):
        if not shared:
            scene = ks.dolls_scene()
            rays, starts = ks.dolls_rays(scene)
            hits, counts, aside = cast_reference(scene, rays)
            shared.update(scene=scene, rays=rays, starts=starts, hits=hits, counts=counts, keep=~aside)
        if build not in cache:
            c = dict(shared)
            c["built"] = ks.built(pta, c["scene"])
            with ks.kd_env(BUILDS[build]):
                c["tree"] = kw.Tree(pta, c["built"])
            c["n_prims"] = n_prims_of(c["scene"])
            first = c["hits"][:, 0]
            c["walk"] = kw.walk(c["tree"], c["rays"], c["n_prims"], first["prim"], kw.stop_parameters(c["rays"], first, gm))
            c["home"] = kw.home_depths(c["tree"], c["scene"]["models"], c["scene"]["camera"][0])
            cache[build] = c
        return cache[build]
    return get


def _slot_counts(pta):
    """The primitive counts of the scattered scene whose trees have WF_LDS_NODES - 2, WF_LDS_NODES and WF_LDS_NODES + 2 device
    node slots.  A tree of n nodes takes n + 1 slots (slot 1 pads the root: prep_treelets, csrc/pt_gpu.hip) and n is odd, so
    these are the nearest counts on either side of the limit, and the limit itself."""
    want = {v - 1: k for k, v in SLOT_LABELS.items()}   # builder nodes -> label
    found = {}
    for seed in range(3, 40):
        for n in range(100, 180):
            t = kw.Tree(pta, ks.built(pta, ks.scattered_scene(n, seed)))
            if t.n_nodes in want and want[t.n_nodes] not in found:
                found[want[t.n_nodes]] = (n, seed)
            if t.n_nodes > max(want):
                break
        if len(found) == len(want):
            break
    assert len(found) == len(want), ("no scattered scene with the wanted node counts", found)
    return {k: found[k] for k in SLOT_LABELS}


@pytest.fixture(scope="module")
def tinies(pta):
    cache = {}

    def get(name):
        if not cache:
            for scene in ks.tiny_scenes(_slot_counts(pta)):
                rays = ks.generic_rays(scene, TINY_RAYS)
                hits, counts, aside = cast_reference(scene, rays)
                built = ks.built(pta, scene)
                cache[scene["name"]] = dict(scene=scene, rays=rays, hits=hits, counts=counts, keep=~aside, built=built,
                                            tree=kw.Tree(pta, built), n_prims=n_prims_of(scene))
            assert sorted(cache) == sorted(TINY_NAMES)
        return cache[name]
    return get


def describe(name, c):
    t = c["tree"]
    line = f"{name}: prims {c['n_prims']} depth {t.depth} nodes {t.n_nodes} leaves {t.n_leaves} set-aside share {(~c['keep']).mean():.5f}"
    if "walk" in c:
        line += f" longest entry list {int(c['home'].max())} stack heights (height: rays) " + \
                str({int(h): int(n) for h, n in enumerate(np.bincount(c["walk"]["height"])) if n})
    print(line)


# ---------------------------------------------------------------------------------------------------------------------
# CPU: reach
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("corner", CORNERS)
def test_deep_build_reaches_the_overflow_stacks(nests, corner):
    """Deep build: at least 500 rays with a model height >= WF_EXACT_LDS_STACK + 2, 200 with >= 40, 200 whose accepted hit lies
    in a leaf popped from >= WF_LDS_STACK + 2 (a value stored in the overflow part decides a result), 100 near-axis rays with
    >= WF_EXACT_LDS_STACK + 2, and 20 blocks of 64 that hold heights on both sides of WF_LDS_STACK."""
    c = nests(corner, "deep")
    describe(f"nest-{corner} deep", c)
    h, hh, cls = c["walk"]["height"], c["walk"]["hit_height"], c["classes"]
    figures = dict(exact_limit=int((h >= kw.WF_EXACT_LDS_STACK + 2).sum()), forty=int((h >= 40).sum()),
                   hit_from_overflow=int(((hh >= kw.WF_LDS_STACK + 2) & c["keep"]).sum()),
                   near_axis=int((h[cls == 3] >= kw.WF_EXACT_LDS_STACK + 2).sum()))
    blocks = h[cls == 4].reshape(-1, 64)
    figures["mixed_blocks"] = int(((blocks <= kw.WF_LDS_STACK - 2).any(axis=1) & (blocks >= kw.WF_LDS_STACK + 2).any(axis=1)).sum())
    print(figures)
    assert c["tree"].depth <= 62
    assert figures["exact_limit"] >= 500 and figures["forty"] >= 200 and figures["hit_from_overflow"] >= 200
    assert figures["near_axis"] >= 100 and figures["mixed_blocks"] >= 20
    near = c["rays"][cls == 3, 3:]
    assert (np.abs(near).min(axis=1) < ks.AXIS_SLACK).all() and (near == 0).any(axis=1).sum() > 100
    # blocks of 64 that are all deep: the outward class
    assert (h[cls == 0].reshape(-1, 64) >= kw.WF_LDS_STACK + 2).all(axis=1).sum() >= 20
    leaving = c["starts"] >= 0
    assert leaving.sum() == ks.RAYS_PER_CLASS and (c["starts"][leaving] < c["n_prims"]).all()


@pytest.mark.parametrize("corner", CORNERS)
def test_default_build_reaches_the_overflow_stack(nests, corner):
    """Default builder settings (depth cap 16 + 1.3 log2 n = 25): at least 200 rays with a model height >= WF_LDS_STACK + 2."""
    c = nests(corner, "default")
    describe(f"nest-{corner} default", c)
    n = int((c["walk"]["height"] >= kw.WF_LDS_STACK + 2).sum())
    print("rays at or above", kw.WF_LDS_STACK + 2, ":", n)
    assert n >= 200


@pytest.mark.parametrize("corner,build", NEST_KEYS)
def test_generated_sets_keep_their_conditions(nests, corner, build):
    """The set-aside share within gm.SET_ASIDE_CAP (asserted for the model alone), every origin strictly inside the scene's
    box, hits of both kinds, and rays that leave a primitive."""
    c = nests(corner, build)
    assert (~c["keep"]).mean() <= gm.SET_ASIDE_CAP
    assert origins_strictly_inside(c["tree"], c["rays"])
    first = c["hits"][:, 0]
    hit = first["prim"] >= 0
    assert (hit & ((first["flags"] & gm.FLAG_SPHERE) != 0)).sum() > 100 and (hit & ((first["flags"] & gm.FLAG_SPHERE) == 0)).sum() > 2000
    assert (first["flags"][hit] & gm.FLAG_BACKFACE).any() and (~hit).sum() > 100
    assert c["n_prims"] <= 400


@pytest.mark.parametrize("corner", CORNERS)
def test_entry_lists_cover_the_batch_boundaries(nests, corner):
    """Home depths (= entry-list lengths) 0, exactly WF_ENTRY_BATCH and WF_ENTRY_BATCH + 1 occur, in both builds."""
    for build in BUILDS:
        home = nests(corner, build)["home"]
        print(corner, build, "home depths (depth: primitives)", {int(d): int(n) for d, n in enumerate(np.bincount(home)) if n})
        assert (home == 0).any() and (home == kw.WF_ENTRY_BATCH).any() and (home == kw.WF_ENTRY_BATCH + 1).any()
        assert home.max() <= kw.ENTRY_LIST_CAP


def test_entry_lists_reach_the_long_lists(dolls):
    """At least 100 primitives with a home depth above 2 * WF_ENTRY_BATCH and at least one above 40, on the nested boxes under
    the deep build; lists of 0, WF_ENTRY_BATCH and WF_ENTRY_BATCH + 1 entries too, and rays that leave primitives of each.

    The corner nest cannot give these: its longest list has 14 entries (prep_entry_lists pads a primitive's box by 2.5e-7 of
    the scene's largest coordinate, which leaves 22 octaves, and the builder spends about one level per octave on a corner
    nest: it cuts several octaves off at once).  The nested boxes make it peel one face per level (kd_shape_scenes.dolls_scene)."""
    c = dolls("deep")
    describe("dolls deep", c)
    home = c["home"]
    print("home depths (depth: primitives)", {int(d): int(n) for d, n in enumerate(np.bincount(home)) if n})
    figures = dict(above_two_batches=int((home > 2 * kw.WF_ENTRY_BATCH).sum()), above_40=int((home > 40).sum()), longest=int(home.max()))
    lists = home[c["starts"][c["starts"] >= 0]]           # the list each leaving ray reads
    figures.update(rays_above_two_batches=int((lists > 2 * kw.WF_ENTRY_BATCH).sum()), rays_above_40=int((lists > 40).sum()))
    print(figures)
    assert figures["above_two_batches"] >= 100 and figures["above_40"] >= 1
    assert (home == 0).any() and (home == kw.WF_ENTRY_BATCH).any() and (home == kw.WF_ENTRY_BATCH + 1).any()
    assert home.max() <= kw.ENTRY_LIST_CAP and c["tree"].depth <= 62
    assert figures["rays_above_two_batches"] >= 500 and figures["rays_above_40"] >= 100
    assert (~c["keep"]).mean() <= gm.SET_ASIDE_CAP and origins_strictly_inside(c["tree"], c["rays"]) and c["n_prims"] <= 400


# ---------------------------------------------------------------------------------------------------------------------
# CPU: the builder, the oracle
# ---------------------------------------------------------------------------------------------------------------------
def check_tree(c):
    """The structure checks of test_kd_tree_structure_and_coverage, and its coverage check against the brute-force model:
    every hit lies in a leaf the traversal visits."""
    import test_abi_and_kd as tak
    t = c["tree"]
    if t.n_nodes == 0:
        assert c["n_prims"] == 0 and t.depth == 0
        return
    kw.check_structure(t, c["n_prims"])
    rng = np.random.default_rng(11)
    for r in rng.choice(np.nonzero(c["keep"])[0], 60, replace=False):
        vis = tak.visited_prims(t.nodes, t.refs, t.info, c["rays"][r, :3], c["rays"][r, 3:])
        for j in range(min(int(c["counts"][r]), MAX_HITS)):
            assert int(c["hits"]["prim"][r, j]) in vis, (r, j)


@pytest.mark.parametrize("corner,build", NEST_KEYS)
def test_nest_trees_are_well_formed(nests, corner, build):
    c = nests(corner, build)
    check_tree(c)
    assert c["tree"].depth <= 62


@pytest.mark.parametrize("build", sorted(BUILDS))
def test_dolls_trees_are_well_formed(dolls, build):
    c = dolls(build)
    check_tree(c)
    assert c["tree"].depth <= 62


@pytest.mark.parametrize("mode", ["PTO_BRUTE_FORCE", "PTO_BVH"])
def test_oracle_casts_match_the_model_on_the_dolls(pta, oracle, dolls, mode):
    c = dolls("default")
    hits, counts = oracle.OracleScene(c["built"].desc, getattr(oracle, mode)).trace_all(c["rays"], MAX_HITS)
    assert np.array_equal(counts[c["keep"]], c["counts"][c["keep"]])
    same_records(hits, c["hits"], c["keep"], ("dolls", mode))


@pytest.mark.parametrize("name", TINY_NAMES)
def test_tiny_trees_are_well_formed(tinies, name):
    c = tinies(name)
    describe(name, c)
    check_tree(c)
    assert (~c["keep"]).mean() <= gm.SET_ASIDE_CAP
    assert c["n_prims"] == 0 or origins_strictly_inside(c["tree"], c["rays"])
    t = c["tree"]
    if name in ("one-triangle", "one-sphere", "root-is-a-leaf"):
        assert t.n_nodes == 1 and t.depth == 0 and c["n_prims"] == {"root-is-a-leaf": kw.PT_KD_MAX_LEAF}.get(name, 1)
    if name == "max-leaf-plus-one":
        assert c["n_prims"] == kw.PT_KD_MAX_LEAF + 1
    if name.startswith("slots-"):
        assert t.n_nodes + 1 == SLOT_LABELS[name[6:]]
    if c["n_prims"]:
        assert (c["counts"] > 0).sum() > 200 and (c["counts"] == 0).sum() > 200


@pytest.mark.parametrize("mode", ["PTO_BRUTE_FORCE", "PTO_BVH"])
@pytest.mark.parametrize("corner", CORNERS)
def test_oracle_casts_match_the_model_on_the_nest(pta, oracle, nests, corner, mode):
    c = nests(corner, "default")
    hits, counts = oracle.OracleScene(c["built"].desc, getattr(oracle, mode)).trace_all(c["rays"], MAX_HITS)
    assert np.array_equal(counts[c["keep"]], c["counts"][c["keep"]])
    same_records(hits, c["hits"], c["keep"], (corner, mode))


@pytest.mark.parametrize("mode", ["PTO_BRUTE_FORCE", "PTO_BVH"])
@pytest.mark.parametrize("name", TINY_NAMES)
def test_oracle_casts_match_the_model_on_tiny_scenes(pta, oracle, tinies, name, mode):
    c = tinies(name)
    hits, counts = oracle.OracleScene(c["built"].desc, getattr(oracle, mode)).trace_all(c["rays"], MAX_HITS)
    assert np.array_equal(counts[c["keep"]], c["counts"][c["keep"]])
    same_records(hits, c["hits"], c["keep"], (name, mode))


def frame_profile(pta):
    return pta.Profile.make(48, 32, 2, 6)


@pytest.mark.parametrize("corner", CORNERS)
def test_the_frames_own_rays_reach_the_overflow_stack(pta, oracle, nests, corner):
    """The rays of the 48 x 32 frame itself (OracleScene.path_rays of 300 paths: camera, shadow and bounce rays) through the
    model's walk of the deep tree: at least 100 of them reach WF_LDS_STACK + 2.  The camera sits inside the corner."""
    c = nests(corner, "deep")
    prof = frame_profile(pta)
    osc = oracle.OracleScene(c["built"].desc, oracle.PTO_BVH)
    rng = np.random.default_rng(5)
    rays = np.concatenate([osc.path_rays(prof, int(p), int(s)) for p, s in zip(rng.integers(0, 48 * 32, 300), rng.integers(1, 3, 300))])
    h = kw.walk(c["tree"], rays, c["n_prims"])["height"]
    print(corner, "frame rays", len(rays), "reaching", kw.WF_LDS_STACK + 2, ":", int((h >= kw.WF_LDS_STACK + 2).sum()), "highest", int(h.max()))
    assert (h >= kw.WF_LDS_STACK + 2).sum() >= 100


def refusal_scene(pta):
    """The shortest nest, by octaves, whose tree under PT_KD_MAX_DEPTH=70 is deeper than the walkers' stacks allow
    (depth >= PT_KD_STACK), or None when no nest of up to 100 octaves gets there.  -> (scene, CPU depth, octaves)."""
    deepest = (None, 0, 0)
    for octaves in range(ks.NEST_OCTAVES + 4, 101, 4):
        scene = ks.nest_scene("min", octaves)
        with ks.kd_env(REFUSAL_ENV):
            depth = kw.Tree(pta, ks.built(pta, scene)).depth
        if depth > deepest[1]:
            deepest = (scene, depth, octaves)
        if depth >= kw.PT_KD_STACK:
            return scene, depth, octaves
    return deepest


def test_a_longer_nest_passes_the_depth_the_walkers_allow(pta):
    """PT_KD_MAX_DEPTH is read after the builder's clamp to 62, so the variable can make a tree the walkers' stacks do not
    hold; prep_create is the guard (the GPU test below asserts its refusal).  Here: the builder really gets there."""
    scene, depth, octaves = refusal_scene(pta)
    print("octaves", octaves, "primitives", n_prims_of(scene), "depth under PT_KD_MAX_DEPTH=70:", depth)
    assert depth >= kw.PT_KD_STACK and n_prims_of(scene) <= 400
    with ks.kd_env(ks.DEEP_ENV):
        assert kw.Tree(pta, ks.built(pta, scene)).depth <= 62


# ---------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------
def gpu_scene(pta, c, env, translucent=False):
    """A GpuScene of the scene under the builder's variables `env`; its tree is the one the CPU tests measured."""
    built = ks.built(pta, c["scene"], translucent)
    before = dict(os.environ)
    with ks.kd_env(env):
        g = pta.GpuScene(built)
    assert dict(os.environ) == before
    info = g.info()
    assert info.kd_depth == c["tree"].depth and info.n_kd_nodes == c["tree"].n_nodes, (info.kd_depth, c["tree"].depth)
    return g, built


def check_casts(pta, g, c, what, modes=(0, 2)):
    keep, ref, rays = c["keep"], c["hits"], c["rays"]
    hits, counts = g.trace_all(rays, MAX_HITS)                           # the scalar walker, whole lists
    assert np.array_equal(counts[keep], c["counts"][keep]), what
    same_records(hits, ref, keep, (what, "trace_all"))
    same_records(g.trace(rays), ref[:, 0], keep, (what, "trace"))
    for mode in modes:                                                   # k_wf_trace, k_wf_trace_wide, k_wf_trace_exact
        same_records(g.trace_wavefront(rays, None, mode), ref[:, 0], keep, (what, "wavefront", mode))


@pytest.mark.gpu
def test_wavefront_trace_on_the_default_nest(pta, nests):
    """The narrowest of the device tests: trace_wavefront mode 0 on the default-build nest."""
    c = nests("min", "default")
    g, _ = gpu_scene(pta, c, BUILDS["default"])
    same_records(g.trace_wavefront(c["rays"], None, 0), c["hits"][:, 0], c["keep"], ("nest-min default", "wavefront", 0))
    g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("corner,build", NEST_KEYS)
def test_device_casts_match_the_model_on_the_nest(pta, nests, corner, build):
    """Every cast path on every build and orientation, all fields bit for bit on the kept rows: GpuScene.trace_all (whole
    lists and counts), GpuScene.trace, trace_wavefront modes 0 and 2, and modes 1 and 3 with start_prims on the rays that
    leave a primitive."""
    c = nests(corner, build)
    what = f"nest-{corner} {build}"
    g, _ = gpu_scene(pta, c, BUILDS[build])
    check_casts(pta, g, c, what)
    leaving = c["starts"] >= 0
    for mode in (1, 3):
        w = g.trace_wavefront(c["rays"][leaving], c["starts"][leaving].astype(np.uint32), mode)
        same_records(w, c["hits"][leaving, 0], c["keep"][leaving], (what, "wavefront", mode))
    g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("build", sorted(BUILDS))
def test_device_casts_match_the_model_on_the_dolls(pta, dolls, build):
    """The nested boxes: every cast path, and trace_wavefront modes 1 and 3 with start_prims on the rays that leave a face -
    under the deep build trav_enter reads lists of up to 53 entries, seven batches."""
    c = dolls(build)
    g, _ = gpu_scene(pta, c, BUILDS[build])
    check_casts(pta, g, c, f"dolls {build}")
    leaving = c["starts"] >= 0
    for mode in (1, 3):
        w = g.trace_wavefront(c["rays"][leaving], c["starts"][leaving].astype(np.uint32), mode)
        same_records(w, c["hits"][leaving, 0], c["keep"][leaving], ("dolls", build, "wavefront", mode))
    g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", TINY_NAMES)
def test_device_casts_match_the_model_on_tiny_scenes(pta, tinies, name):
    c = tinies(name)
    g, _ = gpu_scene(pta, c, {})
    check_casts(pta, g, c, name)
    if c["n_prims"]:     # entry lists of a root that is a leaf: none; of a small tree: short
        starts = (np.arange(len(c["rays"])) % c["n_prims"]).astype(np.uint32)
        for mode in (1, 3):
            same_records(g.trace_wavefront(c["rays"], starts, mode), c["hits"][:, 0], c["keep"], (name, "wavefront", mode))
    else:
        assert (c["counts"] == 0).all()
    g.close()


def check_frames(pta, oracle, c, env, translucent, what):
    prof = frame_profile(pta)
    g, built = gpu_scene(pta, c, env, translucent)
    o_rgb, o_acc, stats = oracle.OracleScene(built.desc, oracle.PTO_BVH).render(prof)
    assert stats["numeric_errors"] == 0
    for flags in (0, pta.PT_FLAG_NO_GRIDS, pta.PT_FLAG_MEGAKERNEL):
        rgb, acc = g.render(prof, pta.Opts.make(flags=flags))
        assert np.array_equal(bits(acc), bits(o_acc)) and np.array_equal(rgb, o_rgb), (what, translucent, flags)
        g.render(prof, pta.Opts.make(flags=flags | pta.PT_FLAG_COUNTERS))
        counters = g.counters().as_dict()
        for k in COUNTERS:
            assert counters[k] == stats[k], (what, translucent, flags, k, counters[k], stats[k])
    assert g.info().has_translucent == int(translucent)
    g.close()
    return stats, o_acc


@pytest.mark.gpu
@pytest.mark.parametrize("translucent", [False, True])
@pytest.mark.parametrize("corner", CORNERS)
def test_device_frames_match_the_oracle_on_the_deep_nest(pta, oracle, nests, corner, translucent):
    """48 x 32, 2 spp, 6 bounces on the default path, the KD-tree pipeline and the megakernel: accumulator and image equal to
    the oracle's bit for bit, the path counters equal to the oracle's.  The translucent variant (opacity 0.5 on a third of the
    models) runs the ALPHA trace and the ordered shadow walk.  test_the_frames_own_rays_reach_the_overflow_stack shows that
    these frames' rays go where the deep stacks are."""
    stats, _ = check_frames(pta, oracle, nests(corner, "deep"), ks.DEEP_ENV, translucent, f"nest-{corner}")
    assert stats["segments"] > stats["samples"] and stats["shadow_rays"] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("name", TINY_NAMES)
def test_device_frames_match_the_oracle_on_tiny_scenes(pta, oracle, tinies, name):
    stats, o_acc = check_frames(pta, oracle, tinies(name), {}, False, name)
    if name == "empty":      # every cast misses: the frame is the background
        assert stats["shaded_hits"] == 0 and stats["segments"] == stats["samples"]
        assert (bits(o_acc) == bits(np.broadcast_to(o_acc[0], o_acc.shape))).all()


ESCAPE_EXTENT = 4.0     # k_escape_build declines a primitive whose rays reach further than H_LO / 2e-6 = 2.5: the nest, shrunk


@pytest.mark.gpu
@pytest.mark.parametrize("corner", CORNERS)
def test_escape_masks_prove_only_misses_on_the_deep_nest(pta, oracle, corner):
    """k_escape_build walks the same deep tree with a stack of its own (ESC_STACK).  The clear-bit proof of
    tests/test_escape_masks.py: a ray through a clear cell of a primitive's mask, from a height the kernel accepts, hits
    nothing - for the brute-force oracle and for the device's exact walker - and the kernels' own lookup (escape_query)
    proves nothing that brute force contradicts.  The scene is the nest shrunk to a box of ESCAPE_EXTENT (the same tree: depth
    59): in the box of 2^30 the mask builder declines every primitive, their rays reach too far for its height band."""
    from test_escape_masks import H_HI, H_LO, rays_through_clear_cells
    scene = ks.nest_scene(corner, scale=ESCAPE_EXTENT / ks.HI)
    c = dict(scene=scene, n_prims=n_prims_of(scene))
    with ks.kd_env(ks.DEEP_ENV):
        c["tree"] = kw.Tree(pta, ks.built(pta, scene))
    assert c["tree"].depth >= kw.WF_EXACT_LDS_STACK + 2
    g, built = gpu_scene(pta, c, ks.DEEP_ENV)
    masks = g.escape_masks()
    has = np.abs(masks[0]).sum(axis=1) > 0
    assert g.info().escape_prims == int(has.sum())
    rays, prims = rays_through_clear_cells(built, masks, 20000, seed=9)
    print(corner, "tree depth", c["tree"].depth, "primitives with a mask", int(has.sum()), "of", c["n_prims"])
    assert has.sum() >= 1 and rays is not None
    h = ((rays[:, :3] - masks[1][prims]) * masks[0][prims]).sum(axis=1)
    ok = (h >= H_LO) & (h <= H_HI) & np.isfinite(rays).all(axis=1)
    proven = g.escape_query(prims[ok], rays[ok])
    osc = oracle.OracleScene(built.desc, oracle.PTO_BRUTE_FORCE)
    _, o_counts = osc.trace_all(rays[ok], 2)
    hits, counts = g.trace_all(rays[ok], 2)
    print(corner, "queries", int(ok.sum()), "proven", int(proven.sum()), "brute-force hits among all", int((o_counts > 0).sum()))
    assert ok.sum() >= 1000 and proven.sum() >= 500
    assert (o_counts[proven] == 0).all() and (counts[proven] == 0).all(), (rays[ok][proven & (o_counts > 0)][:3])
    assert o_counts.sum() == 0 and counts.sum() == 0, (int(o_counts.sum()), int(counts.sum()))
    g.close()


@pytest.mark.gpu
def test_a_tree_deeper_than_the_stacks_is_refused(pta, nests):
    """Under PT_KD_MAX_DEPTH=70 the longer nest's tree has depth >= PT_KD_STACK: scene creation fails with PT_ERR_UNSUPPORTED
    and a message that names the depth, and a scene created afterwards without the variable works."""
    scene, depth, _ = refusal_scene(pta)
    assert depth >= kw.PT_KD_STACK
    built = ks.built(pta, scene)
    with ks.kd_env(REFUSAL_ENV):
        with pytest.raises(pta.PtError) as err:
            pta.GpuScene(built)
    assert err.value.code == pta.PT_ERR_UNSUPPORTED and str(depth) in str(err.value) and "depth" in str(err.value)
    assert "PT_KD_MAX_DEPTH" not in os.environ
    c = nests("min", "default")
    g, _ = gpu_scene(pta, c, {})
    same_records(g.trace(c["rays"][:2048]), c["hits"][:2048, 0], c["keep"][:2048], "after the refusal")
    g.close()
