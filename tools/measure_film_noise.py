"""Does the film's noise figure track the truth?  For the golden scenes at 64x48: the film's mean_error after each pass of
4, 8, 16, 32 samples, and beside it the ACTUAL relative RMSE of the film's mean luminance against a --ref-spp pt_render, with
the same floor:   sqrt(mean_p((lum(film_p / n) - lum(ref_p))^2 / max(lum(ref_p), floor)^2)).   The estimate is the mean over
pixels of a per-pixel standard error, the truth a root mean square over pixels of one realisation's error - they are the same
quantity only up to a shape factor, so what to look for is that both fall together, as 1 / sqrt(n).  Reported, not asserted.
Pixels where the reference or the film is not finite are left out of the truth and counted.  One JSON line per scene.
    timeout -k 10 600 python tools/measure_film_noise.py [--scenes cube spheres ...] [--ref-spp 2048]
Needs the GPU."""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import torch  # noqa: E402
torch.zeros(1, device="cuda")   # (torch's HIP context first, as bench.py)
import __graft_entry__ as entry  # noqa: E402

SCENES = ROOT / "tests" / "golden" / "scenes"
ap = argparse.ArgumentParser()
ap.add_argument("--scenes", nargs="*", default=sorted(p.name for p in SCENES.iterdir() if (p / "scene.isf").exists()))
ap.add_argument("--width", type=int, default=64)
ap.add_argument("--height", type=int, default=48)
ap.add_argument("--bounces", type=int, default=4)
ap.add_argument("--ref-spp", type=int, default=2048)
ap.add_argument("--floor", type=float, default=0.01)
a = ap.parse_args()

pta = entry.load_package()
lum = lambda c: 0.2126 * c[:, 0] + 0.7152 * c[:, 1] + 0.0722 * c[:, 2]
for name in a.scenes:
    host = pta.HostScene.load_isf(SCENES / name / "scene.isf")
    g, ref_scene = pta.GpuScene(host), pta.GpuScene(host)
    ref = lum(ref_scene.render(pta.Profile.make(a.width, a.height, a.ref_spp, a.bounces))[1].astype(np.float64) / a.ref_spp)
    film = pta.Film(pta.Profile.make(a.width, a.height, 1, a.bounces))
    rows = []
    for n in (4, 8, 16, 32):
        film.add_pass(g, n)
        total = int(film.info.samples)
        est = film.noise(0.0, a.floor)
        got = lum(film.read()[0].astype(np.float64) / total)
        ok = np.isfinite(got) & np.isfinite(ref)   # (a NaN sample of the reference render takes its pixel out of the truth)
        rmse = float(np.sqrt(np.mean(((got[ok] - ref[ok]) / np.maximum(ref[ok], a.floor)) ** 2)))
        rows.append({"pass": n, "total": total, "mean_error": round(est.mean_error, 5), "max_block_error": round(est.max_block_error, 5),
                     "actual_rel_rmse": round(rmse, 5), "pixels_left_out": int((~ok).sum())})
    print(json.dumps({"scene": name, "image": f"{a.width}x{a.height}", "bounces": a.bounces, "ref_spp": a.ref_spp, "floor": a.floor,
                      "rows": rows}))
    film.close()
    g.close()
    ref_scene.close()
