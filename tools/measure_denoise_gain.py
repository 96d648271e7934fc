#!/usr/bin/env python3
"""Pick the defaults of pt_denoise_params and record what the filter gains (CPU only: oracle + tests/denoise_model.py).

For every golden scene at 64x48: the oracle's 4-spp frame and a high-spp reference, guides from the oracle
(denoise_model.guides_from_oracle), the model over a small grid of sigma_color, sigma_depth, normal_power_log2 and
iterations.  The winner minimises the mean over the scenes of log(MSE after / MSE before), MSE in mean radiance against
the reference.  Writes tests/golden/denoise_gain.json (grid, winner, MSE before / after per scene) and, for the scenes the
winner improves, the references the test compares with (tests/golden/denoise_ref/<scene>.npy, f32 mean radiance); the
winner goes into include/ptgpu.h by hand (PT_DENOISE_DEFAULT_*).  Scenes the winner does not improve, or whose oracle
frame is not finite, are listed under "excluded" with the reason.

    python tools/measure_denoise_gain.py [--reference-spp 2048]
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

SCENES = ("alpha_transparency", "cube", "head", "reflection", "spheres", "white_furnace_direct", "white_furnace_indirect")
W, H, SPP, BOUNCES = 64, 48, 4, 4
GRID = {"sigma_color": (0.0, 0.25, 0.5, 1.0, 2.0, 4.0), "sigma_depth": (0.5, 1.0, 2.0, 4.0), "normal_power_log2": (3, 5, 7),
        "iterations": (1, 2, 3, 4, 5)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference-spp", type=int, default=2048)
    args = ap.parse_args()
    pta, oracle = entry.load_package(), entry.load_oracle()
    golden = ROOT / "tests" / "golden"
    (golden / "denoise_ref").mkdir(exist_ok=True)
    data, skipped = {}, {}
    for name in SCENES:
        hs = pta.HostScene.load_isf(golden / "scenes" / name / "scene.isf")
        osc = oracle.OracleScene(hs.desc, oracle.PTO_BVH)
        _, acc, _ = osc.render(pta.Profile.make(W, H, SPP, BOUNCES))
        _, ref, _ = osc.render(pta.Profile.make(W, H, args.reference_spp, BOUNCES))
        ref = (ref / np.float32(args.reference_spp)).astype(np.float32)
        if not (np.isfinite(ref).all() and np.isfinite(acc).all()):   # (non-finite radiance is outside the filter's contract)
            skipped[name] = {"reason": "the oracle's frame is not finite"}
            continue
        data[name] = (acc, ref, dm.guides_from_oracle(osc, hs.camera, W, H))
        print(name, "rendered", file=sys.stderr)

    def mse(a, b):
        return float(np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2))

    before = {n: mse(acc / np.float32(SPP), ref) for n, (acc, ref, _) in data.items()}
    best = None
    for sc, sd, npw, it in itertools.product(*(GRID[k] for k in ("sigma_color", "sigma_depth", "normal_power_log2", "iterations"))):
        after = {n: mse(dm.denoise(W, H, SPP, acc, g, it, sc, sd, npw), ref) for n, (acc, ref, g) in data.items()}
        score = float(np.mean([np.log(max(after[n], 1e-30) / max(before[n], 1e-30)) for n in data if before[n] > 0]))
        if best is None or score < best[0]:
            best = (score, {"sigma_color": sc, "sigma_depth": sd, "normal_power_log2": npw, "iterations": it}, after)
    score, win, after = best
    rec = {"width": W, "height": H, "spp": SPP, "reference_spp": args.reference_spp, "bounces": BOUNCES, "grid": GRID,
           "score_mean_log_ratio": score, "defaults": win, "scenes": {}, "excluded": skipped}
    for n in data:
        row = {"mse_raw": before[n], "mse_denoised": after[n]}
        if after[n] < before[n]:
            rec["scenes"][n] = row
            np.save(golden / "denoise_ref" / f"{n}.npy", data[n][1])
        else:
            rec["excluded"][n] = dict(row, reason="the winner does not lower its error")
    (golden / "denoise_gain.json").write_text(json.dumps(rec, indent=1) + "\n")
    print(json.dumps(rec, indent=1))


if __name__ == "__main__":
    main()
