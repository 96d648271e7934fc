"""The escape answers of continuation records that were stored before the scene's masks existed (csrc/pt_wavefront.h
k_cont_escape_fill, csrc/pt_gpu.hip render_chunk).  A fresh view stores its records in its second frame and gets its masks
before the third, so without a refill no record of it ever carries an answer and every loading launch runs the escape test
itself.  The first frame that finds masks the records were not stored under refills them, chunk by chunk, in front of the
launch that loads them; from then on the loading launches are told that the records have answers (PT_CONT_ESCAPE).

What could go wrong: an answer computed from other operands than the storing launch's (another item's hit, words or record),
a record above the marks written, a flag handed to a launch whose records were not refilled, stale answers after the masks
were dropped and rebuilt, a refill where none is due (no masks, records stored under the masks, a translucent scene).  Every
frame is compared bit for bit - rgb8 and the f32 accumulator - with the brute-force CPU oracle, the sequences are repeated
with PT_CONT_ESCAPE=0, and every test reads the numbers that make it mean something: the refill's own counters
(GpuScene.cont_escape_stats), the state words of the records (GpuScene.cont_states) and the caches' counters.

The geometry is `terrace` (tests/test_masked_sequences.py): its masks answer a third of the secondary misses, so the records
carry both answers."""
import numpy as np
import pytest

import scene_builder as sb
from test_masked_sequences import W, H, SPP, far_camera, schedule, shared, terrace, want_of
from test_prestaged_misses import CAMERA, assert_same, oracle_frame

gpu = pytest.mark.gpu

NAMES = ("fill_launches", "fill_items", "flagged", "fallback")
CONT = ("bytes", "items", "cached", "resets", "stores", "loads", "missing")
ITEMS = (W // 32) * ((H + 31) // 32) * 32 * 32 * SPP   # (32 x 32 tiles)


@pytest.fixture(autouse=True)
def escape_answers_on(monkeypatch):
    """The tests run the recorded answers whatever ships on; the switched-off sequences set it themselves."""
    monkeypatch.setenv("PT_CONT_ESCAPE", "1")
    for k in ("PT_QUEUE_GIB", "PT_QUEUE_STEADY_GIB", "PT_QUEUE_ONE_PASS_GIB", "PT_CONT_CACHE_GIB", "PT_CONT_CACHE"):
        monkeypatch.delenv(k, raising=False)


def esc(g):
    return dict(zip(NAMES, g.cont_escape_stats()))


def cont(g):
    return dict(zip(CONT, g.cont_cache_stats()))


def answers(words):
    """(records written, records with an answer, records whose answer is `proven`) of an array of state words."""
    assert not (words & ~np.uint32(7)).any() and not ((words & 6) != 0)[(words & 1) == 0].any(), np.unique(words)
    assert not ((words & 4) != 0)[(words & 2) == 0].any(), np.unique(words)
    return int((words & 1).astype(bool).sum()), int((words & 2).astype(bool).sum()), int((words & 4).astype(bool).sum())


_reference = {}


def stored_under_masks(pta, monkeypatch, key, scene, prof, want, frames=3, opts=None):
    """The state words of a scene whose records were stored under existing masks (PT_ESCAPE_AFTER=0): made once per key."""
    if key not in _reference:
        schedule(monkeypatch, "after-0")
        g = pta.GpuScene(scene)
        for k in range(frames):
            assert_same(g.render(prof, opts) if opts is not None else g.render(prof), want, (key, "reference", k))
        e, loads, words = esc(g), cont(g)["loads"], g.cont_states()
        g.close()
        assert e["fill_launches"] == 0 and e["fallback"] == 0 and e["flagged"] == loads > 0, (key, e, loads)
        words.setflags(write=False)
        _reference[key] = words
    return _reference[key]


def test_the_library_has_the_getters(pta):
    """No GPU: the symbols are there."""
    lib = pta.gpu_lib()
    assert "pt_get_cont_escape_stats" in pta.GPU_SYMBOLS and "pt_scene_cont_states_copy" in pta.GPU_SYMBOLS
    assert len(lib.pt_get_cont_escape_stats.argtypes) == 5 and len(lib.pt_scene_cont_states_copy.argtypes) == 3


def test_the_fill_kernel_is_in_the_library_and_small(tmp_path):
    """From the built library: k_cont_escape_fill is there, without scratch and without LDS."""
    from test_bounce0_four_waves import kernel_table
    k = [v for name, v in kernel_table(tmp_path).items() if "k_cont_escape_fill" in name]
    assert len(k) == 1, k
    assert k[0]["private_segment_fixed_size"] == 0 and k[0]["group_segment_fixed_size"] == 0 and k[0]["vgpr_count"] <= 128, k[0]


@gpu
@pytest.mark.parametrize("sched", ["default", "after-4", "after-0", "after-1"])
def test_the_records_get_their_answers_when_the_masks_arrive(pta, oracle, monkeypatch, sched):
    """Seven frames of a fresh terrace.  default / after-4: the records are stored in frame 1 without masks (no answer in any
    state word), the arrival frame refills them in ONE launch over every cached item and is flagged already, every later frame
    is flagged, no lane of a flagged launch runs the test itself, and the state words are those of a scene that stored under
    existing masks, word for word.  after-0 / after-1: stored under the masks - no refill, flagged from the first load on.
    Then the same sequence with PT_CONT_ESCAPE=0: the same frames, nothing refilled, nothing flagged."""
    case, scene, prof = terrace(pta, "point")
    want = want_of(oracle, scene, prof, "point", "opaque")
    ref = stored_under_masks(pta, monkeypatch, "A", scene, prof, want)
    n_written, n_known, n_proven = answers(ref)
    print("reference: written, with an answer, proven:", n_written, n_known, n_proven, "of", len(ref))
    assert len(ref) == ITEMS and 0 < n_proven < n_known <= n_written   # (both answers occur: the test can tell them apart)
    arrival = schedule(monkeypatch, sched)
    g = pta.GpuScene(scene)
    for k in range(7):
        assert_same(g.render(prof), want, (sched, k))
        e, c = esc(g), cont(g)
        print(sched, k, e, c)
        assert c["missing"] == 0 and e["fallback"] == 0, (sched, k, e, c)
        if k == 0:
            assert not any(e.values()) and not any(c.values()), (sched, k, e, c)
            continue
        assert (c["cached"], c["stores"], c["loads"]) == (ITEMS, 1, k - 1), (sched, k, c)
        words = g.cont_states()
        if arrival >= 2:
            late = k >= arrival
            assert (e["fill_launches"], e["fill_items"]) == ((1, ITEMS) if late else (0, 0)), (sched, k, e)
            assert e["flagged"] == (k - arrival + 1 if late else 0), (sched, k, e)
            assert np.array_equal(words, ref) if late else answers(words)[1:] == (0, 0), (sched, k, answers(words))
        else:
            assert (e["fill_launches"], e["fill_items"], e["flagged"]) == (0, 0, k - 1), (sched, k, e)
            assert np.array_equal(words, ref), (sched, k, answers(words))
    g.close()
    monkeypatch.setenv("PT_CONT_ESCAPE", "0")
    g = pta.GpuScene(scene)
    for k in range(7):
        assert_same(g.render(prof), want, (sched, "off", k))
        assert not any(esc(g).values()), (sched, "off", k, esc(g))
    assert cont(g)["loads"] == 5 and cont(g)["missing"] == 0
    if arrival >= 2:
        assert answers(g.cont_states())[1:] == (0, 0)
    g.close()


@gpu
def test_no_masks_no_refill(pta, oracle, monkeypatch):
    """PT_ESCAPE=0: no masks, no fill launch, no flag."""
    case, scene, prof = terrace(pta, "point")
    want = want_of(oracle, scene, prof, "point", "opaque")
    schedule(monkeypatch, "no-masks")
    g = pta.GpuScene(scene)
    for k in range(5):
        assert_same(g.render(prof), want, ("no masks", k))
        assert not any(esc(g).values()), (k, esc(g))
    assert cont(g)["loads"] == 3 and g.info().escape_prims == 0 and answers(g.cont_states())[1:] == (0, 0)
    g.close()


@gpu
@pytest.mark.parametrize("switch", ["1", "0"])
def test_masks_dropped_by_a_camera_move_and_rebuilt(pta, oracle, monkeypatch, switch):
    """Default schedule.  Four frames at A (refilled in frame 2); a move to a camera twice as far out drops the masks and starts
    an empty prefix: nothing, stored without masks, then the masks return and the records of THAT view are refilled - a second
    launch, the words of a scene that stored the far view under masks -, then loaded.  Back at A the masks stay: the records
    are stored under them, no third refill.  No flagged lane ever runs the test itself.  PT_CONT_ESCAPE=0: the same frames."""
    cams = {"A": sb.make_camera(pta, **CAMERA), "far": far_camera(pta)}
    state = {}
    for label, cam in cams.items():
        case, scene, prof = terrace(pta, "point", camera=cam)
        state[label] = (scene, want_of(oracle, scene, prof, "point", "opaque", label))
    ref_far = stored_under_masks(pta, monkeypatch, "far", state["far"][0], prof, state["far"][1])
    assert 0 < answers(ref_far)[2] < answers(ref_far)[1]
    monkeypatch.setenv("PT_CONT_ESCAPE", switch)
    on = switch == "1"
    schedule(monkeypatch, "default")
    g = pta.GpuScene(state["A"][0])
    for k in range(4):
        assert_same(g.render(prof), state["A"][1], ("A", k))
    e = esc(g)
    assert e == ({"fill_launches": 1, "fill_items": ITEMS, "flagged": 2, "fallback": 0} if on else dict.fromkeys(NAMES, 0)), e
    g.set_camera(cams["far"])
    assert g.info().escape_prims == 0
    for k in range(4):
        assert_same(g.render(prof), state["far"][1], ("far", k))
        e = esc(g)
        print("far", k, e, cont(g))
        assert (g.info().escape_prims > 0) == (k >= 2)
        if on:
            assert e == {"fill_launches": 1 + (k >= 2), "fill_items": ITEMS * (1 + (k >= 2)), "flagged": 2 + max(0, k - 1), "fallback": 0}, (k, e)
            if k >= 1:
                words = g.cont_states()
                assert np.array_equal(words, ref_far) if k >= 2 else answers(words)[1:] == (0, 0), (k, answers(words))
        else:
            assert not any(e.values()), (k, e)
    g.set_camera(cams["A"])
    assert g.info().escape_prims > 0   # (the masks of the larger delta_in stay)
    for k in range(3):
        assert_same(g.render(prof), state["A"][1], ("back at A", k))
        e = esc(g)
        print("back at A", k, e, cont(g))
        if on:
            assert e == {"fill_launches": 2, "fill_items": 2 * ITEMS, "flagged": 4 + (k >= 2), "fallback": 0}, (k, e)
        else:
            assert not any(e.values()), (k, e)
    if on:
        assert 0 < answers(g.cont_states())[2] < answers(g.cont_states())[1]   # (stored under the masks: answers present)
    assert cont(g)["missing"] == 0
    g.close()


@gpu
def test_a_material_edit_under_masks_stores_the_answers_itself(pta, oracle, monkeypatch):
    """Default schedule, four frames, then a table with other roughnesses: nothing, then zeroed and stored - under the masks, so
    with answers -, then loaded and flagged: no fill launch beyond the first view's, no flagged lane runs the test."""
    case, scene, prof = terrace(pta, "point")
    cam = sb.make_camera(pta, **CAMERA)
    other = sb.case_materials(case, pta)
    for m in other:
        m.roughness = min(1.0, 0.37 + 0.5 * m.roughness)
    first = want_of(oracle, scene, prof, "point", "opaque")
    want_other = want_of(oracle, sb.build(case, pta=pta, camera=cam, materials=other), prof, "point", "opaque", "other materials")
    assert not np.array_equal(first[1], want_other[1])
    schedule(monkeypatch, "default")
    g = pta.GpuScene(scene)
    for k in range(4):
        assert_same(g.render(prof), first, ("first", k))
    assert esc(g) == {"fill_launches": 1, "fill_items": ITEMS, "flagged": 2, "fallback": 0}, esc(g)
    g.set_materials(other)
    for k in range(4):
        assert_same(g.render(prof), want_other, ("other", k))
        e, c = esc(g), cont(g)
        print("other", k, e, c)
        assert e == {"fill_launches": 1, "fill_items": ITEMS, "flagged": 2 + max(0, k - 1), "fallback": 0}, (k, e)
        assert (c["resets"], c["stores"], c["loads"], c["missing"]) == (1 + (k >= 1), 1 + (k >= 1), 2 + max(0, k - 1), 0), (k, c)
    n_written, n_known, n_proven = answers(g.cont_states())
    assert 0 < n_proven < n_known <= n_written, (n_written, n_known, n_proven)
    g.close()


@gpu
def test_a_translucent_table_keys_no_records(pta, oracle, monkeypatch):
    """The translucent terrace never keys the continuation cache: no fill launch, no flag, nothing allocated."""
    case, scene, prof = terrace(pta, "point", "alpha")
    assert scene.translucent
    want = want_of(oracle, scene, prof, "point", "alpha")
    schedule(monkeypatch, "default")
    g = pta.GpuScene(scene)
    for k in range(5):
        assert_same(g.render(prof), want, ("alpha", k))
        assert not any(esc(g).values()) and not any(cont(g).values()), (k, esc(g), cont(g))
    assert g.info().escape_prims > 0
    g.close()


@gpu
def test_three_shards(pta, oracle, monkeypatch):
    """shard_count = 3, 16 x 16 tiles, a 70 x 33 frame: every rank a scene with masks and records of its own - one refill each,
    over that rank's items, the words of that rank's scene stored under masks, every frame the oracle's pixels of the rank."""
    case, scene, prof = terrace(pta, "point", size=(70, 33))
    want = want_of(oracle, scene, prof, "point", "opaque")
    for rank in range(3):
        o = pta.Opts.make(shard_rank=rank, shard_count=3, tile_w=16, tile_h=16)
        m = pta.local_pixel_map(prof, o)
        local = (want[0][m], want[1][m])
        ref = stored_under_masks(pta, monkeypatch, ("rank", rank), scene, prof, local, opts=o)
        schedule(monkeypatch, "default")
        g = pta.GpuScene(scene)
        for k in range(5):
            assert_same(g.render(prof, o), local, ("rank", rank, k))
        e, c = esc(g), cont(g)
        print("rank", rank, e, c)
        assert c["cached"] == c["items"] >= len(m) * SPP and c["missing"] == 0, (rank, c)
        assert e == {"fill_launches": 1, "fill_items": c["items"], "flagged": 3, "fallback": 0}, (rank, e)
        assert np.array_equal(g.cont_states(), ref) and answers(ref)[1] > 0, rank
        g.close()


@gpu
def test_a_chunk_only_partly_below_the_marks(pta, oracle, monkeypatch):
    """A 1024 x 768 x 4 frame (3 Mi items: the smallest chunk of a frame is 1 Mi), two bounces, room for 2.5 Mi records.  Frame 1
    is planned and runs in chunks of 1 Mi: two of them fit the budget, the mark stands at 2 Mi.  The arrival frame counts again - a first frame, whose chunk is PT_QUEUE_GIB /
    272 B, here about 1.5 Mi: its first chunk lies below the mark (refilled, loaded, flagged), its second only partly - refilled
    up to the mark, not above it, and not loaded.  The words below the mark are those of a scene that stored under masks; the
    planes hold nothing above it."""
    case, scene, prof = terrace(pta, "point", bounces=2, size=(1024, 768))
    # (the geometry and the camera of test_masked_sequences.test_terrace_is_fit_for_a_gpu, which walks their rays; this frame's
    # three million paths are not walked again)
    want = shared(("partial", 1024, 768, 2), lambda: oracle_frame(oracle, scene, prof))
    items, mi = 1024 * 768 * SPP, 1 << 20
    monkeypatch.setenv("PT_CONT_CACHE_GIB", str(2.5 * mi * 32 / 2 ** 30))
    monkeypatch.setenv("PT_QUEUE_GIB", "0.01")
    monkeypatch.setenv("PT_QUEUE_STEADY_GIB", "0.02")
    monkeypatch.setenv("PT_QUEUE_ONE_PASS_GIB", "0.02")   # (or the planned frame takes the whole frame as one chunk)
    ref = stored_under_masks(pta, monkeypatch, "partial", scene, prof, want)
    assert len(ref) == 2 * mi and 0 < answers(ref)[2] < answers(ref)[1]
    schedule(monkeypatch, "default")
    g = pta.GpuScene(scene)
    for k in range(2):
        assert_same(g.render(prof), want, ("partial", k))
    c = cont(g)
    assert g.info().queue_chunk_items == mi and (c["items"], c["cached"], c["stores"]) == (items, 2 * mi, 2), (g.info().queue_chunk_items, c)
    assert answers(g.cont_states())[1:] == (0, 0)
    monkeypatch.setenv("PT_QUEUE_GIB", "0.4")
    assert_same(g.render(prof), want, ("partial", "arrival"))
    chunk = g.info().queue_chunk_items
    e, c = esc(g), cont(g)
    print("arrival: chunk", chunk, e, c)
    assert g.info().escape_prims > 0 and mi < chunk < 2 * mi and g.info().frame_planned == 0, chunk   # (the premise)
    assert e == {"fill_launches": 2, "fill_items": 2 * mi, "flagged": 1, "fallback": 0}, e
    assert (c["cached"], c["stores"], c["loads"], c["missing"]) == (2 * mi, 2, 1, 0), c
    assert np.array_equal(g.cont_states(), ref)
    for k in range(2):   # (planned again: whatever its chunks, no further refill and no lane that runs the test under a flag)
        assert_same(g.render(prof), want, ("partial", "after", k))
        e = esc(g)
        print("after", k, g.info().queue_chunk_items, e, cont(g))
        assert (e["fill_launches"], e["fill_items"], e["fallback"]) == (2, 2 * mi, 0) and e["flagged"] == cont(g)["loads"], e
    assert np.array_equal(g.cont_states(), ref) and cont(g)["cached"] == 2 * mi
    g.close()
