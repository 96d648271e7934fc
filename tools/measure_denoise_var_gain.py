#!/usr/bin/env python3
"""Pick the defaults of pt_denoise_var_params_default and record what the variance-guided filter gains (CPU only: oracle +
tests/denoise_var_model.py).

The setting of tools/measure_denoise_gain.py: the golden scenes at 64x48, the oracle's 4-spp frame, guides from the oracle, the
committed references tests/golden/denoise_ref/<scene>.npy, the score = mean over cube, head, reflection, spheres and
white_furnace_direct of log(MSE after / MSE before).  The moments are NOT the device's bits: the oracle has no per-sample
output, so sample k is taken as the difference of its partial sums after k and k - 1 passes (exact only up to the rounding of
those sums; denoise_var_model.moments_from_partial_sums).  The grid covers sigma_color (the luminance sigma), sigma_depth,
normal_power_log2, iterations AND the demodulation flag.  alpha_transparency, which the plain filter's winner makes worse, is
reported beside the five (its reference is rendered here and stored when the winner improves it).

Writes tests/golden/denoise_var_gain.json: the grid, the winner, per scene the MSE of the raw frame, of pt_denoise's defaults
and of the winner.  The winner goes into include/ptgpu.h by hand (PT_DENOISE_VAR_DEFAULT_*).

    python tools/measure_denoise_var_gain.py [--reference-spp 2048]
"""
import argparse
import itertools
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import __graft_entry__ as entry  # noqa: E402
import denoise_model as dm  # noqa: E402
import denoise_var_model as dvm  # noqa: E402

SCORED = ("cube", "head", "reflection", "spheres", "white_furnace_direct")
REPORTED = ("alpha_transparency",)
W, H, SPP, BOUNCES = 64, 48, 4, 4
GRID = {"sigma_color": (1.0, 2.0, 4.0, 8.0), "sigma_depth": (0.5, 1.0, 2.0, 4.0), "normal_power_log2": (3, 5, 7),
        "iterations": (1, 2, 3, 4, 5), "flags": (0, dm.NO_DEMODULATE)}
KEYS = ("sigma_color", "sigma_depth", "normal_power_log2", "iterations", "flags")


def mse(a, b):
    return float(np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2))


def score_of(after, before):
    return float(np.mean([np.log(max(after[n], 1e-30) / max(before[n], 1e-30)) for n in SCORED]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference-spp", type=int, default=2048)
    args = ap.parse_args()
    pta, oracle = entry.load_package(), entry.load_oracle()
    golden = ROOT / "tests" / "golden"
    plain_rec = json.loads((golden / "denoise_gain.json").read_text())
    assert (plain_rec["width"], plain_rec["height"], plain_rec["spp"], plain_rec["bounces"]) == (W, H, SPP, BOUNCES)
    data = {}
    for name in SCORED + REPORTED:
        acc, mom, guides = dvm.inputs_from_oracle(pta, oracle, golden / "scenes" / name / "scene.isf", W, H, SPP, BOUNCES)
        ref_path = golden / "denoise_ref" / f"{name}.npy"
        if ref_path.exists():
            ref = np.load(ref_path)
        else:
            hs = pta.HostScene.load_isf(golden / "scenes" / name / "scene.isf")
            _, ref, _ = oracle.OracleScene(hs.desc, oracle.PTO_BVH).render(pta.Profile.make(W, H, args.reference_spp, BOUNCES))
            ref = (ref / np.float32(args.reference_spp)).astype(np.float32)
        assert np.isfinite(ref).all() and np.isfinite(acc).all() and np.isfinite(mom).all(), name
        data[name] = (acc, mom, guides, ref)
        print(name, "rendered", file=sys.stderr)

    before = {n: mse(acc / np.float32(SPP), ref) for n, (acc, _, _, ref) in data.items()}
    pd = plain_rec["defaults"]
    plain = {n: mse(dm.denoise(W, H, SPP, acc, g, pd["iterations"], pd["sigma_color"], pd["sigma_depth"], pd["normal_power_log2"]), ref)
             for n, (acc, _, g, ref) in data.items()}
    best = None
    for combo in itertools.product(*(GRID[k] for k in KEYS)):
        sc, sd, npw, it, fl = combo
        after = {n: mse(dvm.denoise_var(W, H, SPP, acc, mom, g, it, sc, sd, npw, fl), ref) for n, (acc, mom, g, ref) in data.items()}
        score = score_of(after, before)
        if best is None or score < best[0]:
            best = (score, dict(zip(KEYS, combo)), after)
    score, win, after = best
    rec = {"width": W, "height": H, "spp": SPP, "bounces": BOUNCES, "references": "tests/golden/denoise_ref",
           "moments": "differences of the oracle's partial sums (not the device's bits)", "grid": GRID,
           "score_mean_log_ratio": score, "plain_score_mean_log_ratio": score_of(plain, before), "defaults": win,
           "scenes": {}, "reported": {}}
    for n in data:
        row = {"mse_raw": before[n], "mse_plain_default": plain[n], "mse_variance_guided": after[n]}
        if n in SCORED:
            rec["scenes"][n] = row
        else:
            row["improved"] = after[n] < before[n]
            rec["reported"][n] = row
            if row["improved"]:
                np.save(golden / "denoise_ref" / f"{n}.npy", data[n][3])
    (golden / "denoise_var_gain.json").write_text(json.dumps(rec, indent=1) + "\n")
    print(json.dumps(rec, indent=1))


if __name__ == "__main__":
    main()
