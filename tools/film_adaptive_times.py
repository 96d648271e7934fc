"""What the adaptive film saves on config 3's workload (HostScene.generate_ps5(500000, 0, 8), 1920x1080): one JSON line with
the wall time and the pixel-samples of pt_film_render_until_adaptive beside pt_film_render_until with the same first pass and
budget - both run to the budget (a target that is never met) and to --target -, alternating in one process order, --runs
times each, every run on a fresh scene after a throwaway scene has taken the process's first launches; and the three new
kernels (HIP events inside the library, pt_film_adaptive_kernel_times, medians of --reps) on the film the last adaptive run
left.  The uniform film stops on the MEAN error, the adaptive one when no TILE's mean is above the target, so "to a target"
compares two different stop rules by design; no threshold is fixed in advance.
    timeout -k 10 900 python tools/film_adaptive_times.py [--first 8] [--max 512] [--target 0.01] [--tile 32] [--runs 3]
Needs the GPU; every step is bounded by the caller's time limit."""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import torch  # noqa: E402
torch.zeros(1, device="cuda")   # (torch's HIP context first, as bench.py)
import __graft_entry__ as entry  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--tris", type=int, default=500000)
ap.add_argument("--width", type=int, default=1920)
ap.add_argument("--height", type=int, default=1080)
ap.add_argument("--bounces", type=int, default=5)
ap.add_argument("--first", type=int, default=8)
ap.add_argument("--max", type=int, default=512)
ap.add_argument("--target", type=float, default=0.01)
ap.add_argument("--tile", type=int, default=32)
ap.add_argument("--uniform-samples", type=int, default=24)
ap.add_argument("--dilate", type=int, default=1)
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--reps", type=int, default=20)
a = ap.parse_args()

pta = entry.load_package()
w, h, n = a.width, a.height, a.width * a.height
prof = pta.Profile.make(w, h, a.first, a.bounces, "FILMIC")
opts = pta.Opts.make(tile_w=a.tile, tile_h=a.tile)
host = pta.HostScene.generate_ps5(a.tris, 0, 8)
med = lambda v: round(float(statistics.median(v)), 4)


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def params(target):
    return pta.FilmAdaptiveParams.default(target=target, first_pass_samples=a.first, max_samples=a.max,
                                          uniform_samples=a.uniform_samples, dilate=a.dilate)


def run(adaptive, target, keep=False):
    """One film on a fresh scene: wall ms, what it rendered, its last figures."""
    g = pta.GpuScene(host, device=0)
    film = pta.Film(prof, opts)
    passes = []
    if adaptive:
        ms = timed(lambda: film.render_until_adaptive(g, params(target), lambda i, s: passes.append(
            {"samples": int(i.last_pass_samples), "tiles": int(film.adaptive_info.last_pass_tiles), "mean_error": round(s.mean_error, 5)})))
    else:
        ms = timed(lambda: film.render_until(g, a.first, a.max, target, on_pass=lambda i, s: passes.append(
            {"samples": int(i.last_pass_samples), "mean_error": round(s.mean_error, 5)})))
    st = film.tile_noise(target)
    out = {"wall_ms": round(ms, 1), "samples": int(film.info.samples), "pixel_samples": int(st.pixel_samples),
           "mean_error": round(st.mean_error, 5), "max_tile_error": round(st.max_tile_error, 5), "over_tiles": int(st.over_tiles),
           "passes": passes}
    g.close()
    if keep:
        return out, film
    film.close()
    return out


warm = pta.GpuScene(host, device=0)   # a throwaway scene takes the first launches of the process (code objects, allocator)
warm_film = pta.Film(prof, opts)
warm_film.render_until_adaptive(warm, pta.FilmAdaptiveParams.default(target=0.0, first_pass_samples=2, uniform_samples=2, max_samples=6))
warm_film.tile_noise(0.0)
warm_film.resolve()
warm_film.close()
warm.close()

result = {"image": f"{w}x{h}", "tris": a.tris, "bounces": a.bounces, "first": a.first, "max": a.max, "tile": a.tile,
          "uniform_samples": a.uniform_samples, "dilate": a.dilate, "n_tiles": ((w + a.tile - 1) // a.tile) * ((h + a.tile - 1) // a.tile)}
kept = None
for label, target in (("to_budget", 0.0), ("to_target", a.target)):
    adaptive, uniform = [], []
    for r in range(a.runs):   # alternating, one process order
        if r == a.runs - 1:   # (the kernels are timed on a film that did take tile passes)
            one, film = run(True, target, keep=True)
            if kept is None and not film.adaptive_info.uniform:
                kept = film
            else:
                film.close()
        else:
            one = run(True, target)
        adaptive.append(one)
        uniform.append(run(False, target))
    am, um = statistics.median(x["wall_ms"] for x in adaptive), statistics.median(x["wall_ms"] for x in uniform)
    result[label] = {"target": target, "adaptive": adaptive[-1], "uniform": uniform[-1],
                     "adaptive_wall_ms": [x["wall_ms"] for x in adaptive], "uniform_wall_ms": [x["wall_ms"] for x in uniform],
                     "pixel_samples_ratio": round(adaptive[-1]["pixel_samples"] / uniform[-1]["pixel_samples"], 4),
                     "wall_ratio": round(am / um, 4)}
if kept is not None and not kept.adaptive_info.uniform and kept.adaptive_info.min_samples >= 2:
    kept.adaptive_kernel_times(reps=3)   # (warm)
    merge_ms, noise_ms, resolve_ms = kept.adaptive_kernel_times(reps=a.reps)
    result.update({"merge_tiles_ms": med(merge_ms), "merge_tiles_mb": round(n * (3 * 20 + 8) / 1e6, 1),
                   "tile_noise_with_err_ms": med(noise_ms), "tile_noise_mb": round(n * (8 + 4 + 4) / 1e6, 1),
                   "resolve_counts_rgb8_ms": med(resolve_ms), "resolve_mb": round(n * (12 + 4 + 3) / 1e6, 1),
                   "film_mb": round(kept.info.device_bytes / 1e6, 1)})
    kept.close()
print(json.dumps(result))
