"""Sample-coherent AOVs without a GPU: the numpy restatement (tests/aov_model.py) against the literal definitions of
include/ptgpu.h, the condition the GPU test's cases must meet (at most 1 % fragile samples), and the fixtures."""
import json
import sys

import numpy as np
import pytest

import aov_model as am
from conftest import GOLDEN, ROOT

f32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def literal_sum(values):
    """One float of one pixel: blocks of 64 sample numbers, x[j] = x[2j] + x[2j+1] six times, the blocks added in order."""
    total = None
    for base in range(0, len(values), 64):
        x = [f32(0.0)] * 64
        for j, v in enumerate(values[base:base + 64]):
            x[j] = f32(v)
        for _ in range(6):
            x = [f32(x[2 * j] + x[2 * j + 1]) for j in range(len(x) // 2)]
        total = x[0] if total is None else f32(total + x[0])
    return total


@pytest.mark.parametrize("n_samples", [1, 2, 3, 5, 64, 65, 130])
def test_the_tree_equals_its_literal_definition(n_samples):
    rng = np.random.default_rng(n_samples)
    n = 5
    r = np.zeros((n_samples, n, am.FLOATS), f32)
    r[:, :, :14] = (rng.normal(0, 1, (n_samples, n, 14)) * 10.0 ** rng.integers(-3, 4, (n_samples, n, 14))).astype(f32)
    covered = rng.random((n_samples, n)) < 0.7
    covered[:, 0] = False                  # a pixel without any surface
    covered[:, 1] = True
    r[:, 1, 0] = f32(-0.0)                 # a sum of negative zeros: the tree's zero additions make it +0 unless the block is full
    prim = rng.integers(0, 3, (n_samples, n)).astype(np.int32)
    r[~covered] = 0
    r[:, :, 7] = covered
    r[:, :, 15] = covered
    r[:, :, 14] = np.where(covered, prim, -1).astype(np.int32).view(f32)
    with np.errstate(all="ignore"):
        got = am.reduce_records(r)
        for p in range(n):
            for k in range(14):
                want = literal_sum([r[s, p, k] for s in range(n_samples)])
                assert bits(got[p, k]) == bits(want), (n_samples, p, k)
            seen = [int(prim[s, p]) for s in range(n_samples) if covered[s, p]]
            assert got[p, 14:15].view(np.int32)[0] == (seen[0] if seen else -1)
            assert got[p, 15] == (seen.count(seen[0]) if seen else 0)
    assert bits(got[1, 0]) == (0x80000000 if n_samples == 64 else 0), "(-0) + (+0) is +0; 64 samples leave no zero to add"


def test_the_guide_rule_on_hand_made_records():
    def record(cov, n3=(0.0, 3.0, 4.0), depth=6.0, albedo=(1.0, 2.0, 3.0), prim=7):
        r = np.zeros(am.FLOATS, f32)
        r[0:3], r[3], r[4:7], r[7] = n3, depth, albedo, cov
        r[14:15] = np.array([prim], np.int32).view(f32)
        return r
    n_samples = 6
    aov = np.stack([record(3.0), record(2.0), record(0.0), record(6.0), record(4.0, depth=np.inf)])
    g = am.guides_of(aov, n_samples)
    prim = g[:, 7].view(np.int32)
    # cov = N / 2 exactly is the majority; below it and cov = 0 are k_guides' miss record
    assert prim.tolist() == [7, -1, -1, 7, 7]
    assert np.array_equal(bits(g[1]), bits(g[2])) and g[1, 3] == -1.0 and (bits(g[1, [0, 1, 2, 4, 5, 6]]) == 0).all()
    assert g[0, 0:3].tolist() == [0.0, 3.0, 4.0], "the normal stays unnormalised"
    assert g[0, 3] == f32(6.0) / f32(3.0) and g[3, 3] == f32(1.0) and np.isinf(g[4, 3])
    assert np.array_equal(bits(g[0, 4:7]), bits(np.array([1.0, 2.0, 3.0], f32) / f32(6.0))), "albedo over N, not over the coverage"
    assert am.guides_of(np.stack([record(1.0)]), 3)[0, 7:8].view(np.int32)[0] == -1      # 1 of 3 is no majority
    assert am.guides_of(np.stack([record(2.0)]), 3)[0, 7:8].view(np.int32)[0] == 7       # 2 of 3 is one (odd N)


@pytest.fixture(scope="module")
def measured(pta, oracle):
    sys.path.insert(0, str(ROOT / "tools"))
    import measure_aov_deviation as tool
    return tool.measure(pta, oracle)


def test_at_most_one_percent_of_a_case_is_fragile(measured):
    """A condition on the cases of tests/test_aov_gpu.py, not a measurement: a case that fails gets another camera or seed
    offset, the cap stays."""
    assert set(measured["cases"]) == set(am.CASES)
    for name, row in measured["cases"].items():
        assert row["fragile"] <= am.FRAGILE_CAP * row["samples"], (name, row)
        assert row["covered"] > 0.5 * row["samples"], (name, row)


def test_the_cases_reach_what_they_are_there_for(pta, oracle):
    model, scene, camera = am.model_of(am.PANES, pta, oracle)
    prof = am.sample_profile(pta)
    rec = am.records_f64(model, prof)
    wall = am.N_PANES * 2                        # the wall's two triangles follow the panes'
    assert (rec.prim >= wall).any(), "walks that skip every pane and stop at the wall (more than 14 draws: ChaCha block 1)"
    assert (rec.prim == wall - 1).sum() + (rec.prim == wall - 2).sum() > 0.05 * rec.prim.size, \
        "walks that skip every entry keep the last pane (no wall behind the upper half)"
    # (a walk that stops in the second block: at one of the panes 15 .. 24)
    assert ((rec.prim >= 2 * 14) & (rec.prim < wall - 2)).any()


def test_the_guide_gain_fixture_reproduces(pta, oracle):
    """tests/golden/aov_guides_gain.json is a report, whichever way it falls; here: that it is what the tool computes (the two
    smallest scenes, alpha_transparency - the scene the sample guides were hoped to help - among them)."""
    sys.path.insert(0, str(ROOT / "tools"))
    import measure_aov_guides_gain as tool
    want = json.loads((GOLDEN / "aov_guides_gain.json").read_text())
    assert set(want["scenes"]) == set(tool.SCENES)
    some = ("alpha_transparency", "cube")
    got = tool.measure(pta, oracle, scenes=some)
    for name in some:
        for key, value in want["scenes"][name].items():
            if key == "valid_pixels":
                assert got["scenes"][name][key] == value, (name, key)
            else:
                assert got["scenes"][name][key] == pytest.approx(value, rel=1e-9), (name, key)
    assert {k: got[k] for k in got if k != "scenes"} == {k: want[k] for k in want if k != "scenes"}


def test_the_tolerance_fixture_reproduces(measured):
    want = json.loads((GOLDEN / "aov_tolerance.json").read_text())
    assert measured == want, "run tools/measure_aov_deviation.py"
    assert set(want["fields"]) == set(am.FIELDS)
