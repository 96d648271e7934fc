#!/usr/bin/env python3
"""What the filters gain from guides made of the frame's own samples (CPU only: the oracle, tests/denoise_model.py,
tests/denoise_var_model.py, tests/aov_model.py).

For the golden scenes at 64x48: the oracle's 4-spp frame (its moments from the differences of its partial sums), the
committed references (tests/golden/denoise_ref), and the MSE in mean radiance after the plain and the variance-guided filter
at their shipped defaults with three kinds of guides -
    centre        dm.guides_from_oracle: the pixel-centre ray's first list entry (what --denoise uses)
    samples       aov_model.guides_of over the reduced float64 sample records: the surfaces the samples' alpha walks stop at
    first_entry   the same with every sample's first list entry (jitter and anti-aliasing, no walk)
The table goes to tests/golden/aov_guides_gain.json and DESIGN 4m, whichever way it falls.

    python tools/measure_aov_guides_gain.py
"""
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import __graft_entry__ as entry  # noqa: E402
import aov_model as am  # noqa: E402
import denoise_model as dm  # noqa: E402
import denoise_var_model as dvm  # noqa: E402
import shading_model as sm  # noqa: E402

SCENES = ("alpha_transparency", "cube", "head", "reflection", "spheres", "white_furnace_direct")
W, H, SPP, BOUNCES = 64, 48, 4, 4
KINDS = ("centre", "samples", "first_entry")


def mse(a, b):
    return float(np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2))


def measure(pta, oracle, log=None, scenes=SCENES):
    golden = ROOT / "tests" / "golden"
    pd = json.loads((golden / "denoise_gain.json").read_text())["defaults"]
    vd = json.loads((golden / "denoise_var_gain.json").read_text())["defaults"]
    rec = {"width": W, "height": H, "spp": SPP, "bounces": BOUNCES, "references": "tests/golden/denoise_ref",
           "plain_defaults": pd, "variance_defaults": vd, "scenes": {}}
    for name in scenes:
        path = golden / "scenes" / name / "scene.isf"
        acc, mom, centre = dvm.inputs_from_oracle(pta, oracle, path, W, H, SPP, BOUNCES)
        ref = np.load(golden / "denoise_ref" / f"{name}.npy")
        hs = pta.HostScene.load_isf(path)
        model = sm.ShadingModel(hs.desc, oracle.OracleScene(hs.desc, oracle.PTO_BRUTE_FORCE), oracle, max_hits=am.MAX_HITS)
        prof = pta.Profile.make(W, H, SPP, BOUNCES)
        guides = {"centre": centre}
        for kind, first in (("samples", False), ("first_entry", True)):
            guides[kind] = am.guides_of(am.reduce_records(am.rounded(am.records_f64(model, prof, first_entry=first))), SPP)
        row = {"mse_raw": mse(acc / np.float32(SPP), ref),
               "valid_pixels": {k: int((guides[k][:, 3] >= 0).sum()) for k in KINDS}}
        for k in KINDS:
            row[f"mse_plain_{k}"] = mse(dm.denoise(W, H, SPP, acc, guides[k], pd["iterations"], pd["sigma_color"], pd["sigma_depth"],
                                                   pd["normal_power_log2"]), ref)
            row[f"mse_variance_{k}"] = mse(dvm.denoise_var(W, H, SPP, acc, mom, guides[k], vd["iterations"], vd["sigma_color"],
                                                           vd["sigma_depth"], vd["normal_power_log2"], vd["flags"]), ref)
        rec["scenes"][name] = row
        if log:
            print(name, row, file=log)
    return rec


def main():
    rec = measure(entry.load_package(), entry.load_oracle(), sys.stderr)
    (ROOT / "tests" / "golden" / "aov_guides_gain.json").write_text(json.dumps(rec, indent=1, sort_keys=True) + "\n")


if __name__ == "__main__":
    main()
