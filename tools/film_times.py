"""What the progressive film costs on config 3's workload (HostScene.generate_ps5(500000, 0, 8), 1920x1080): one JSON line with
k_film_merge and k_film_noise (HIP events inside the library, pt_film_kernel_times, medians of --reps) and the rates their
compulsory traffic makes of that beside pt_measure_copy_bandwidth of the same device, and the wall time of
pt_film_render_until (first pass --first, budget --max, a target that is never met) beside one pt_render of the same total
samples on a fresh scene, both after a throwaway scene has taken the process's first launches.  Every pass of the film is the
first frame of its configuration (unplanned, no cache keyed).
    timeout -k 10 900 python tools/film_times.py [--first 8] [--max 512] [--reps 20]
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
ap.add_argument("--reps", type=int, default=20)
a = ap.parse_args()

pta = entry.load_package()
w, h, n = a.width, a.height, a.width * a.height
prof = pta.Profile.make(w, h, a.first, a.bounces, "FILMIC")
host = pta.HostScene.generate_ps5(a.tris, 0, 8)
med = lambda v: round(float(statistics.median(v)), 4)


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


warm = pta.GpuScene(host, device=0)   # a throwaway scene takes the first launches of the process (code objects, allocator)
warm_film = pta.Film(prof)
warm_film.render_until(warm, 2, 6, 0.0)
warm.render(pta.Profile.make(w, h, 3, a.bounces, "FILMIC"))
warm_film.close()
warm.close()
g = pta.GpuScene(host, device=0)
film = pta.Film(prof)
passes = []
until_ms = timed(lambda: film.render_until(g, a.first, a.max, 0.0, on_pass=lambda i, s: passes.append(
    {"samples": int(i.last_pass_samples), "total": int(i.samples), "mean_error": round(s.mean_error, 5)})))
total = int(film.info.samples)
film.kernel_times(reps=3)   # (warm)
merge_ms, noise_ms = film.kernel_times(reps=a.reps)
_, noise_err_ms = film.kernel_times(with_err=True, reps=a.reps)
merge_mb = 3 * n * 20 / 1e6                 # film and pass read, film written: 3 x (12 + 8) bytes per pixel
noise_mb = (n * 8 + ((n + 255) // 256) * 8) / 1e6
fresh = pta.GpuScene(host, device=0)
one = pta.Profile.make(w, h, total, a.bounces, "FILMIC")
render_ms = timed(lambda: fresh.render(one))
out = {"image": f"{w}x{h}", "tris": a.tris, "bounces": a.bounces, "first": a.first, "max": a.max, "total_samples": total,
       "passes": passes, "render_until_wall_ms": round(until_ms, 1), "one_render_same_samples_wall_ms": round(render_ms, 1),
       "merge_ms": med(merge_ms), "merge_mb": round(merge_mb, 1), "merge_gb_per_s": round(merge_mb / med(merge_ms), 1),
       "noise_ms": med(noise_ms), "noise_mb": round(noise_mb, 1), "noise_gb_per_s": round(noise_mb / med(noise_ms), 1),
       "noise_with_err_ms": med(noise_err_ms), "noise_with_err_gb_per_s": round((noise_mb + n * 4 / 1e6) / med(noise_err_ms), 1),
       "film_mb": round(film.info.device_bytes / 1e6, 1),
       "copy_bandwidth_gb_per_s": round(pta.measure_copy_bandwidth(0, 1 << 30, 5), 1)}
print(json.dumps(out))
