"""What windows are worth to a film: one JSON line per scene - config 3's stand-in (HostScene.generate_ps5(500000, 0,
8)) and the head scene, 1920x1080 - with the doubling uniform film (pt_film_render_until) and the doubling adaptive film
(pt_film_render_until_adaptive) beside pt_film_render_until_windowed with adaptive 0 and 1 and window_samples 8, 16, 32, 64,
all to --target within N = --max samples.  Per configuration: the pixel-samples spent, the largest count, the passes and the
wall time - the median of --runs runs, the configurations ALTERNATING inside every round, every run on a fresh scene (made
from one Prep) after a throwaway scene has taken the process's first launches.  And the two new kernels by HIP events inside
the library (pt_film_window_kernel_times, medians of --reps) on a film the adaptive windowed loop left non-uniform.  The
uniform film stops on the MEAN error, the others when no TILE's mean is above the target: two stop rules by design.  No ratio is
promised in advance.
    timeout -k 10 900 python tools/film_window_times.py [--scene ps5|head|both] [--max 512] [--target 0.02] [--runs 3]
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
ap.add_argument("--scene", default="both", choices=("ps5", "head", "both"))
ap.add_argument("--tris", type=int, default=500000)
ap.add_argument("--width", type=int, default=1920)
ap.add_argument("--height", type=int, default=1080)
ap.add_argument("--bounces", type=int, default=5)
ap.add_argument("--first", type=int, default=8)
ap.add_argument("--max", type=int, default=512)
ap.add_argument("--target", type=float, default=0.02)
ap.add_argument("--tile", type=int, default=32)
ap.add_argument("--uniform-samples", type=int, default=24)
ap.add_argument("--dilate", type=int, default=1)
ap.add_argument("--windows", default="8,16,32,64")
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--reps", type=int, default=20)
a = ap.parse_args()

pta = entry.load_package()
w, h, n = a.width, a.height, a.width * a.height
opts = pta.Opts.make(tile_w=a.tile, tile_h=a.tile)
med = lambda v: round(float(statistics.median(v)), 4)   # noqa: E731
WINDOWS = [int(x) for x in a.windows.split(",")]
CONFIGS = [("doubling_uniform", None, None), ("doubling_adaptive", None, None)]
CONFIGS += [(f"windowed_{'adaptive' if ad else 'uniform'}_{ws}", ad, ws) for ad in (0, 1) for ws in WINDOWS]


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def run(host, prep, config, keep=False):
    """One film on a fresh scene: wall ms and what it spent."""
    label, adaptive, window = config
    g = pta.GpuScene(host, device=0, prep=prep)
    passes = []
    note = lambda i, s: passes.append(int(i.last_pass_samples))   # noqa: E731
    if window is not None:
        film = pta.Film.windowed(pta.Profile.make(w, h, a.max, a.bounces, "FILMIC"), opts)
        p = pta.FilmWindowParams.default(target=a.target, window_samples=window, adaptive=adaptive,
                                         uniform_samples=a.uniform_samples, dilate=a.dilate)
        ms = timed(lambda: film.render_until_windowed(g, p, note))
    else:
        film = pta.Film(pta.Profile.make(w, h, a.first, a.bounces, "FILMIC"), opts)
        if label == "doubling_adaptive":
            p = pta.FilmAdaptiveParams.default(target=a.target, first_pass_samples=a.first, max_samples=a.max,
                                               uniform_samples=a.uniform_samples, dilate=a.dilate)
            ms = timed(lambda: film.render_until_adaptive(g, p, note))
        else:
            ms = timed(lambda: film.render_until(g, a.first, a.max, a.target, on_pass=note))
    st = film.tile_noise(a.target)
    out = {"wall_ms": round(ms, 1), "largest_count": int(film.info.samples), "pixel_samples": int(st.pixel_samples),
           "passes": len(passes), "mean_error": round(st.mean_error, 5), "max_tile_error": round(st.max_tile_error, 5),
           "over_tiles": int(st.over_tiles)}
    g.close()
    if keep and not film.adaptive_info.uniform:
        return out, film
    film.close()
    return out, None


def measure(name, host):
    prep = pta.Prep(host)
    warm = pta.GpuScene(host, device=0, prep=prep)   # a throwaway scene takes the first launches of the process
    wf = pta.Film.windowed(pta.Profile.make(w, h, 6, a.bounces, "FILMIC"), opts)
    wf.render_until_windowed(warm, pta.FilmWindowParams.default(target=0.0, window_samples=2, uniform_samples=2))
    wf.resolve()
    wf.close()
    warm.close()
    result = {"scene": name, "image": f"{w}x{h}", "bounces": a.bounces, "target": a.target, "max": a.max, "first": a.first,
              "tile": a.tile, "uniform_samples": a.uniform_samples, "dilate": a.dilate, "runs": a.runs}
    runs = {c[0]: [] for c in CONFIGS}
    kept = None
    for r in range(a.runs):        # alternating: every round runs every configuration once
        for c in CONFIGS:
            want = kept is None and c[1] == 1 and r == a.runs - 1
            one, film = run(host, prep, c, keep=want)
            runs[c[0]].append(one)
            if film is not None:
                kept = film
    for label, rs in runs.items():
        last = dict(rs[-1])
        last["wall_ms"] = med([x["wall_ms"] for x in rs])
        last["wall_ms_runs"] = [x["wall_ms"] for x in rs]
        result[label] = last
    if kept is not None:
        kept.window_kernel_times(reps=3)   # (warm)
        gather_ms, scatter_ms = kept.window_kernel_times(reps=a.reps)
        result.update({"gather_tiles_ms": med(gather_ms), "scatter_tiles_ms": med(scatter_ms),
                       "gather_mb": round(n * 40 / 1e6, 1), "scatter_mb": round(n * 48 / 1e6, 1)})
        kept.close()
    prep.close()
    print(json.dumps(result), flush=True)


if a.scene in ("ps5", "both"):
    measure("ps5_500k", pta.HostScene.generate_ps5(a.tris, 0, 8))
if a.scene in ("head", "both"):
    measure("head", pta.HostScene.load_isf(ROOT / "tests" / "golden" / "scenes" / "head" / "scene.isf"))
