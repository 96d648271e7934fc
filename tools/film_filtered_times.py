"""What stopping on the FILTERED error buys: one JSON line comparing, on one scene at 1920x1080,
    A  pt_film_render_until_adaptive (tiles selected by the raw error) followed by pt_film_denoise (variance), and
    B  pt_film_render_until_filtered (tiles selected by ferr) followed by the same pt_film_denoise
with the same target, first pass and budget: pixel-samples, passes, wall time (loop + final filter, medians of --runs,
alternating in one process order, every run on a fresh scene after a throwaway scene has taken the process's first launches),
and the RMSE of both final filtered images - and of both unfiltered films - against one uniform render of --ref-samples
samples on the same GPU path.  Also pt_film_denoise_kernel_times (prep / passes / finish + ferr / tile reduce, medians of
--reps) on the film run B left, and on one uniform film beside pt_denoise_var_stage_times on the same planes.  No ratio is
fixed in advance: the numbers go into DESIGN 4j as they come.
    timeout -k 10 900 python tools/film_filtered_times.py --scene head
    timeout -k 10 900 python tools/film_filtered_times.py --tris 500000
Needs the GPU; every step is bounded by the caller's time limit."""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import numpy as np  # noqa: E402
import torch  # noqa: E402
torch.zeros(1, device="cuda")   # (torch's HIP context first, as bench.py)
import __graft_entry__ as entry  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--scene", default=None, help="a golden scene's name (tests/golden/scenes/<name>); default: the generated scene")
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
ap.add_argument("--iterations", type=int, default=-1, help="filter passes; default: the library's for the variance filter")
ap.add_argument("--ref-samples", type=int, default=4096)
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--reps", type=int, default=20)
a = ap.parse_args()

pta = entry.load_package()
w, h, n = a.width, a.height, a.width * a.height
prof = pta.Profile.make(w, h, a.first, a.bounces, "FILMIC")
opts = pta.Opts.make(tile_w=a.tile, tile_h=a.tile)
if a.scene:
    host = pta.HostScene.load_isf(ROOT / "tests" / "golden" / "scenes" / a.scene / "scene.isf")
else:
    host = pta.HostScene.generate_ps5(a.tris, 0, 8)
flt = pta.DenoiseParams.default_var() if a.iterations < 0 else pta.DenoiseParams.default_var(iterations=a.iterations)
adaptive = dict(target=a.target, first_pass_samples=a.first, max_samples=a.max, uniform_samples=a.uniform_samples, dilate=a.dilate)
med = lambda v: round(float(statistics.median(v)), 4)   # noqa: E731


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def run(filtered, keep=False):
    """One film on a fresh scene: the loop, then the final filter.  Wall ms of both, what was rendered, the images."""
    g = pta.GpuScene(host, device=0)
    film = pta.Film(prof, opts)
    passes, images = [], {}

    def on_pass(i, s):
        passes.append({"samples": int(i.last_pass_samples), "tiles": int(film.adaptive_info.last_pass_tiles),
                       "mean_error": round(s.mean_error, 5)})
    if filtered:
        loop_ms = timed(lambda: film.render_until_filtered(g, pta.FilmFilteredParams.default(filter=flt, **adaptive), on_pass))
    else:
        loop_ms = timed(lambda: film.render_until_adaptive(g, pta.FilmAdaptiveParams.default(**adaptive), on_pass))
    filter_ms = timed(lambda: images.update(filtered=film.denoise(g, flt)[0]))
    images["raw"] = film.resolve(want_color=True)[1]
    raw, fil = film.tile_noise(a.target), film.filtered_noise(g, flt, a.target)
    out = {"wall_ms": round(loop_ms + filter_ms, 1), "loop_ms": round(loop_ms, 1), "final_filter_ms": round(filter_ms, 1),
           "passes": len(passes), "tile_passes": int(film.adaptive_info.tile_passes), "samples": int(film.info.samples),
           "pixel_samples": int(raw.pixel_samples), "raw_mean_error": round(raw.mean_error, 5), "raw_over_tiles": int(raw.over_tiles),
           "filtered_mean_error": round(fil.mean_error, 5), "filtered_over_tiles": int(fil.over_tiles), "pass_list": passes}
    if keep:
        return out, images, film, g
    film.close()
    g.close()
    return out, images


warm = pta.GpuScene(host, device=0)   # a throwaway scene takes the first launches of the process (code objects, allocator)
warm_film = pta.Film(prof, opts)
warm_film.render_until_filtered(warm, pta.FilmFilteredParams.default(filter=flt, target=0.0, first_pass_samples=2, uniform_samples=2,
                                                                     max_samples=6))
warm_film.denoise(warm, flt)
warm_film.close()
_, ref_acc = warm.render(pta.Profile.make(w, h, a.ref_samples, a.bounces, "FILMIC"))
ref = ref_acc.astype(np.float64) / a.ref_samples
warm.close()
print(f"reference of {a.ref_samples} samples rendered", file=sys.stderr, flush=True)


ref_ok = np.isfinite(ref).all(axis=1)


def rmse(img):
    """Over the pixels that are finite in the reference and in the image (the others are counted, not hidden)."""
    ok = ref_ok & np.isfinite(img).all(axis=1)
    return round(float(np.sqrt(np.mean((img[ok].astype(np.float64) - ref[ok]) ** 2))), 6), int((~ok).sum())


result = {"scene": a.scene or f"generate_ps5({a.tris}, 0, 8)", "image": f"{w}x{h}", "bounces": a.bounces, "target": a.target,
          "first": a.first, "max": a.max, "tile": a.tile, "uniform_samples": a.uniform_samples, "dilate": a.dilate,
          "filter_iterations": int(flt.iterations), "ref_samples": a.ref_samples, "ref_non_finite_pixels": int((~ref_ok).sum()),
          "n_tiles": ((w + a.tile - 1) // a.tile) * ((h + a.tile - 1) // a.tile)}
raw_loop, filtered_loop, kept = [], [], None
for r in range(a.runs):   # alternating, one process order
    one, images = run(False)
    one.update(rmse_filtered=rmse(images["filtered"])[0], rmse_unfiltered=rmse(images["raw"])[0],
               non_finite_pixels=rmse(images["filtered"])[1])
    raw_loop.append(one)
    if r == a.runs - 1:
        one, images, film, g = run(True, keep=True)
        kept = (film, g)
    else:
        one, images = run(True)
    one.update(rmse_filtered=rmse(images["filtered"])[0], rmse_unfiltered=rmse(images["raw"])[0],
               non_finite_pixels=rmse(images["filtered"])[1])
    filtered_loop.append(one)
    print(f"run {r + 1} of {a.runs}: {raw_loop[-1]['wall_ms']} ms / {one['wall_ms']} ms", file=sys.stderr, flush=True)
A, B = raw_loop[-1], filtered_loop[-1]
result.update({"adaptive_then_denoise": A, "render_until_filtered": B,
               "adaptive_wall_ms": [x["wall_ms"] for x in raw_loop], "filtered_wall_ms": [x["wall_ms"] for x in filtered_loop],
               "pixel_samples_ratio": round(B["pixel_samples"] / A["pixel_samples"], 4),
               "wall_ratio": round(statistics.median(x["wall_ms"] for x in filtered_loop) / statistics.median(x["wall_ms"] for x in raw_loop), 4),
               "rmse_ratio": round(B["rmse_filtered"] / A["rmse_filtered"], 4) if A["rmse_filtered"] else None})
film, g = kept
if film.adaptive_info.min_samples >= 2:
    film.denoise_kernel_times(g, flt, reps=3)   # (warm)
    prep, passes, finish, reduce = film.denoise_kernel_times(g, flt, reps=a.reps)
    result.update({"prep_ms": med(prep), "passes_ms": med(passes), "finish_ferr_ms": med(finish), "tile_reduce_ms": med(reduce),
                   "filter_scratch_mb": round(film.denoise_scratch_bytes() / 1e6, 1)})
film.close()
# the same stages on one uniform film's planes through pt_denoise_var_stage_times and through the film filter's hook
import ctypes as C  # noqa: E402
flat = pta.Film(prof, opts)
flat.add_pass(g, a.first)
d_acc, d_mom = flat.planes_device()
d_guides = torch.empty(n * 8, dtype=torch.float32, device="cuda")
d_scratch = torch.empty(pta.denoise_var_scratch_bytes(w, h), dtype=torch.uint8, device="cuda")
d_col = torch.empty(n * 3, dtype=torch.float32, device="cuda")
g.render_guides_device(w, h, d_guides.data_ptr())
torch.cuda.synchronize()
ms, rows = (C.c_float * pta.PT_DENOISE_STAGES)(), []
for k in range(a.reps + 3):
    pta.check_gpu(pta.gpu_lib().pt_denoise_var_stage_times(0, w, h, a.first, C.byref(flt), d_acc, d_mom, d_guides.data_ptr(),
                                                           d_col.data_ptr(), None, d_scratch.data_ptr(), ms))
    if k >= 3:
        rows.append(list(ms))
its = int(flt.iterations)
flat.denoise_kernel_times(g, flt, reps=3)
prep, passes, finish, reduce = flat.denoise_kernel_times(g, flt, reps=a.reps)
result["uniform_film_same_planes"] = {
    "samples": a.first,
    "denoise_var_stage_times": {"prep_ms": med([r[0] for r in rows]), "passes_ms": med([sum(r[1:1 + its]) for r in rows]),
                                "finish_ms": med([r[pta.PT_DENOISE_STAGES - 1] for r in rows])},
    "film_denoise_kernel_times": {"prep_ms": med(prep), "passes_ms": med(passes), "finish_ferr_ms": med(finish),
                                  "tile_reduce_ms": med(reduce)}}
flat.close()
g.close()
print(json.dumps(result))
