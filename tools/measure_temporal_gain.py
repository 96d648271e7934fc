#!/usr/bin/env python3
"""What a camera path gains from the temporal history (CPU only: the oracle, tests/history_model.py, tests/aov_model.py,
tests/denoise_var_model.py, tests/film_denoise_model.py).

For four golden scenes at 64x48 and 4 spp, along the first 8 cameras of a 360-camera turntable (tools/make_orbit.py: one
degree a frame): per frame the oracle's reference at 512 spp, the raw 4-spp frame, and the frame's AOV records from the
float64 sample records.  MSE in mean radiance against the frame's reference, averaged over frames 4-7, of
    raw               the 4-spp frame
    filtered          the frame through the shipped single-frame variance filter (its defaults, the frame's sample guides)
    history           the resolved history (accum / count)
    history_filtered  the history through the film filter with every pixel's own count (the same defaults and guides)
for every point of a small grid over normal_cos, plane_tol, H (max_samples = H x 4) and K (rotate).  With K > 1 frame i is
the window [jN, jN + N), j = i mod K, of the oracle's K N-sample enumeration (differences of its partial sums: not the
device's bits); the AOV records are the N-sample frame's in either case, as pt_history_add_frame has them.
The best grid point by the mean over the scenes of history_filtered / filtered is reported next to the shipped defaults.
The table goes to tests/golden/temporal_gain.json and DESIGN 4n, whichever way it falls.

    python tools/measure_temporal_gain.py
"""
import itertools
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "tools"))
import __graft_entry__ as entry  # noqa: E402
import aov_model as am  # noqa: E402
import denoise_var_model as dvm  # noqa: E402
import film_denoise_model as fdm  # noqa: E402
import history_model as hm  # noqa: E402
import make_orbit  # noqa: E402
import shading_model as sm  # noqa: E402

SCENES = ("head", "cube", "spheres", "alpha_transparency")
W, H, SPP, BOUNCES, REF_SPP = 64, 48, 4, 4, 512
FRAMES, MEASURED, TURN = 8, (4, 5, 6, 7), 360
GRID = {"normal_cos": (0.8, 0.9, 0.97), "plane_tol": (0.01, 0.02, 0.05), "frames": (4, 8, 16), "rotate": (1, 8)}
f32 = np.float32


def mse(a, b):
    return float(np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2))


def frame_inputs(pta, oracle, path, camera, rotates):
    """The reference, the AOV records and, per K, the frames (accum, moments) of windows j = 0 .. K-1 of one camera."""
    hs = pta.HostScene.load_isf(path)
    hs.set_camera(camera)
    osc = oracle.OracleScene(hs.desc, oracle.PTO_BVH)
    ref = osc.render(pta.Profile.make(W, H, REF_SPP, BOUNCES))[1] / f32(REF_SPP)
    model = sm.ShadingModel(hs.desc, oracle.OracleScene(hs.desc, oracle.PTO_BRUTE_FORCE), oracle, max_hits=am.MAX_HITS)
    prof = pta.Profile.make(W, H, SPP, BOUNCES)
    aov = am.reduce_records(am.rounded(am.records_f64(model, prof)))
    return ref, aov, osc


def window(pta, osc, rotate, j):
    """(accum, moments) of the samples [jN, jN + N) of the K N-sample enumeration."""
    prof = pta.Profile.make(W, H, rotate * SPP, BOUNCES)
    zero = np.zeros((W * H, 3), f32)
    partials = np.stack([osc.render(prof, sample_count=k)[1] if k else zero for k in range(j * SPP, j * SPP + SPP + 1)])
    rel = (partials - partials[0]).astype(f32)
    return rel[-1], dvm.moments_from_partial_sums(rel[1:])


def measure(pta, oracle, log=None, scenes=SCENES, grid=GRID):
    golden = ROOT / "tests" / "golden"
    vd = json.loads((golden / "denoise_var_gain.json").read_text())["defaults"]
    points = [dict(zip(grid, v)) for v in itertools.product(*grid.values())]
    rec = {"width": W, "height": H, "spp": SPP, "bounces": BOUNCES, "reference_spp": REF_SPP, "frames": FRAMES,
           "measured_frames": list(MEASURED), "orbit": f"tools/make_orbit.py, {TURN} cameras about y, the first {FRAMES}",
           "variance_defaults": vd, "grid": {k: list(v) for k, v in grid.items()}, "scenes": {}}
    flt = lambda counts, acc, mom, guides: fdm.film_denoise(W, H, counts, acc, mom, guides, vd["iterations"], vd["sigma_color"],
                                                            vd["sigma_depth"], vd["normal_power_log2"], vd["flags"], True)[0]
    for name in scenes:
        path = golden / "scenes" / name / "scene.isf"
        cams = make_orbit.orbit(pta.HostScene.load_isf(path), TURN)[:FRAMES]
        views = [hm.view_constants(c, W, H) for c in cams]
        refs, aovs, frames = [], [], {k: [] for k in grid["rotate"]}
        for f, cam in enumerate(cams):
            ref, aov, osc = frame_inputs(pta, oracle, path, cam, grid["rotate"])
            refs.append(ref)
            aovs.append(aov)
            for k in grid["rotate"]:
                frames[k].append(window(pta, osc, k, f % k))
        guides = [am.guides_of(a, SPP) for a in aovs]
        acc1 = [frames[1][f] for f in MEASURED]
        row = {"mse_raw": float(np.mean([mse(frames[1][f][0] / f32(SPP), refs[f]) for f in MEASURED])),
               "mse_filtered": float(np.mean([mse(flt(SPP, frames[1][f][0], frames[1][f][1], guides[f]), refs[f]) for f in MEASURED])),
               "grid": []}
        del acc1
        for p in points:
            params = hm.Params(p["normal_cos"], p["plane_tol"], p["frames"] * SPP, p["rotate"])
            hist, shares, m_res, m_flt = None, [], [], []
            for f in range(FRAMES):
                a, m = frames[p["rotate"]][f]
                hist = hm.advance(hist, views[f - 1] if f else None, views[f], SPP, a, m, aovs[f], params, W, H)
                if f in MEASURED:
                    shares.append(hm.share(hist["map"], hist["surf"]))
                    with np.errstate(all="ignore"):
                        m_res.append(mse((hist["accum"] / hist["count"][:, None].astype(f32)).astype(f32), refs[f]))
                    m_flt.append(mse(flt(hist["count"], hist["accum"], hist["moments"], guides[f]), refs[f]))
            row["grid"].append(dict(p, share=float(np.mean(shares)), mse_history=float(np.mean(m_res)),
                                    mse_history_filtered=float(np.mean(m_flt))))
        rec["scenes"][name] = row
        if log:
            best = min(row["grid"], key=lambda g: g["mse_history_filtered"])
            print(name, {k: v for k, v in row.items() if k != "grid"}, "best", best, file=log, flush=True)
    # the grid point with the smallest mean ratio filtered history / single-frame filter over the scenes
    score = []
    for i, p in enumerate(points):
        score.append(float(np.mean([rec["scenes"][s]["grid"][i]["mse_history_filtered"] / rec["scenes"][s]["mse_filtered"] for s in scenes])))
    best = int(np.argmin(score))
    rec["best"] = dict(points[best], mean_ratio=score[best])
    rec["defaults"] = {"normal_cos": hm.DEFAULTS.normal_cos, "plane_tol": hm.DEFAULTS.plane_tol,
                       "max_samples": hm.DEFAULTS.max_samples, "rotate": hm.DEFAULTS.rotate}
    at = [i for i, p in enumerate(points) if (p["normal_cos"], p["plane_tol"], p["frames"] * SPP, p["rotate"]) == tuple(hm.DEFAULTS)]
    rec["defaults"]["mean_ratio"] = score[at[0]] if at else None
    return rec


def main():
    rec = measure(entry.load_package(), entry.load_oracle(), sys.stderr)
    (ROOT / "tests" / "golden" / "temporal_gain.json").write_text(json.dumps(rec, indent=1, sort_keys=True) + "\n")
    print(json.dumps({"best": rec["best"], "defaults": rec["defaults"]}))


if __name__ == "__main__":
    main()
