"""What N GPUs would make of an adaptive film, PROJECTED FROM ONE GPU: config 3's stand-in
(HostScene.generate_ps5(500000, 0, 8), 1920x1080), tile 32, target 0.02, budget 512.  For N = 1, 2, 4, 8 the N shard films of
one film live on the one GPU and are driven in lock-step through the stepper calls - pt_film_add_pass / pt_film_add_tile_pass,
pt_film_shard_tile_noise, the combination on the host, pt_film_select_tiles - the ranks one after the other, every rank's pass
and local noise timed on the host clock around a device synchronise.  The projected N-GPU time of a run is the sum over its
passes of the SLOWEST rank, plus the host's selection step; no exchange latency is in it (2 * n_tiles floats per pass), and
no contention for the host.  Beside it: pt_film_render_until_adaptive on an unsharded film - what the library could do before
shard films existed - measured in the same process, alternating with the emulated runs, --runs times each (medians), every run
on a fresh film; the resulting efficiency T_1 / (N * T_N); and the packed kernels (HIP events inside the library,
pt_film_adaptive_kernel_times and pt_film_window_kernel_times, medians of --reps) on one rank's film beside the image-order
kernels on the unsharded film.  One JSON line.
    timeout -k 10 900 python tools/film_sharded_times.py [--first 8] [--max 512] [--target 0.02] [--tile 32] [--runs 3]
Needs the GPU; every step is bounded by the caller's time limit."""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

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
ap.add_argument("--target", type=float, default=0.02)
ap.add_argument("--tile", type=int, default=32)
ap.add_argument("--uniform-samples", type=int, default=24)
ap.add_argument("--dilate", type=int, default=1)
ap.add_argument("--ranks", type=int, nargs="+", default=[1, 2, 4, 8])
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--reps", type=int, default=20)
a = ap.parse_args()

pta = entry.load_package()
w, h = a.width, a.height
prof = pta.Profile.make(w, h, a.first, a.bounces, "FILMIC")
n_tiles = ((w + a.tile - 1) // a.tile) * ((h + a.tile - 1) // a.tile)
host = pta.HostScene.generate_ps5(a.tris, 0, 8)
med = lambda v: round(float(statistics.median(v)), 4)   # noqa: E731
LUM_FLOOR = 0.01


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, out


def params():
    return pta.FilmAdaptiveParams.default(target=a.target, lum_floor=LUM_FLOOR, first_pass_samples=a.first, max_samples=a.max,
                                          uniform_samples=a.uniform_samples, dilate=a.dilate)


def unsharded(g, keep=False):
    film = pta.Film(prof, pta.Opts.make(tile_w=a.tile, tile_h=a.tile))
    passes = []
    ms, st = timed(lambda: film.render_until_adaptive(g, params(), lambda i, s: passes.append(
        (int(i.last_pass_samples), int(film.adaptive_info.last_pass_tiles)))))
    out = {"wall_ms": round(ms, 1), "passes": passes, "samples": int(film.info.samples), "pixel_samples": int(st.pixel_samples),
           "converged": int(st.converged)}
    if keep:
        return out, film
    film.close()
    return out


def lockstep(g, n, keep=False):
    """The loop of pt_film_render_until_adaptive over n shard films, the ranks one after the other."""
    films = [pta.Film.shard(prof, pta.Opts.make(tile_w=a.tile, tile_h=a.tile, shard_rank=r, shard_count=n)) for r in range(n)]
    passes, active, stats, last, total = [], None, None, 0, 0
    while stats is None or not stats.converged:
        nxt = 2 * last if last else a.first
        if total + nxt > min(a.max, 1 << 24):
            break
        everything = stats is None or total < a.uniform_samples or len(active) == n_tiles
        rank_ms, sums = [], []
        for f in films:
            ms, part = timed(lambda f=f: ((f.add_pass(g, nxt) if everything else f.add_tile_pass(g, nxt, active)),
                                          f.shard_tile_noise(LUM_FLOOR))[1])
            rank_ms.append(ms)
            sums.append(part[0])
        t = time.perf_counter()
        tsum = np.maximum.reduce(sums)
        active = films[0].select_tiles(tsum, a.target, a.dilate)
        stats = films[0].tile_stats_from_sums(tsum, a.target)
        host_ms = (time.perf_counter() - t) * 1e3
        last, total = nxt, int(films[0].info.samples)
        passes.append({"samples": nxt, "tiles": int(films[0].adaptive_info.last_pass_tiles),
                       "rank_ms": [round(x, 2) for x in rank_ms], "host_ms": round(host_ms, 3)})
    out = {"ranks": n, "passes": passes, "samples": total, "pixel_samples": int(stats.pixel_samples), "converged": int(stats.converged),
           "projected_ms": round(sum(max(p["rank_ms"]) + p["host_ms"] for p in passes), 1),
           "one_gpu_serial_ms": round(sum(sum(p["rank_ms"]) + p["host_ms"] for p in passes), 1)}
    if keep:
        return out, films
    for f in films:
        f.close()
    return out


warm = pta.GpuScene(host, device=0)   # a throwaway scene takes the first launches of the process (code objects, allocator)
wf = pta.Film(prof, pta.Opts.make(tile_w=a.tile, tile_h=a.tile))
wf.render_until_adaptive(warm, pta.FilmAdaptiveParams.default(target=0.0, first_pass_samples=2, uniform_samples=2, max_samples=6))
wf.close()
ws = pta.Film.shard(prof, pta.Opts.make(tile_w=a.tile, tile_h=a.tile, shard_rank=0, shard_count=2))
ws.add_pass(warm, 2)
ws.add_tile_pass(warm, 4, [0, 1, 2, 3])
ws.shard_tile_noise(LUM_FLOOR)
ws.close()
warm.close()

g = pta.GpuScene(host, device=0)
result = {"image": f"{w}x{h}", "tris": a.tris, "bounces": a.bounces, "first": a.first, "max": a.max, "target": a.target, "tile": a.tile,
          "uniform_samples": a.uniform_samples, "dilate": a.dilate, "n_tiles": n_tiles, "runs": a.runs,
          "what": "projection from one GPU: sum over passes of the slowest rank; no exchange latency, no host contention"}
base, runs = [], {n: [] for n in a.ranks}
for r in range(a.runs):   # alternating, one process order
    base.append(unsharded(g))
    for n in a.ranks:
        runs[n].append(lockstep(g, n))
t1 = statistics.median(x["wall_ms"] for x in base)
result["unsharded"] = dict(base[-1], wall_ms_runs=[x["wall_ms"] for x in base], wall_ms=round(t1, 1))
result["sharded"] = []
for n in a.ranks:
    tn = statistics.median(x["projected_ms"] for x in runs[n])
    last = runs[n][-1]
    assert [(p["samples"], p["tiles"]) for p in last["passes"]] == [tuple(p) for p in base[-1]["passes"]], "the ranks took other passes"
    assert last["pixel_samples"] == base[-1]["pixel_samples"]
    result["sharded"].append(dict(last, projected_ms_runs=[x["projected_ms"] for x in runs[n]], projected_ms=round(tn, 1),
                                  speedup=round(t1 / tn, 3), efficiency=round(t1 / (n * tn), 3)))
# the kernels: one rank's packed film beside the unsharded film, both after the same run
_, whole = unsharded(g, keep=True)
kernels = {}
if not whole.adaptive_info.uniform:
    whole.adaptive_kernel_times(reps=3)
    m, s, _r = whole.adaptive_kernel_times(reps=a.reps)
    whole.window_kernel_times(reps=3)
    ga, sc = whole.window_kernel_times(reps=a.reps)
    kernels["image_order_all_tiles"] = {"merge_tiles_ms": med(m), "tile_noise_with_err_ms": med(s), "gather_tiles_ms": med(ga),
                                        "scatter_tiles_ms": med(sc), "tiles": n_tiles}
    for n in [x for x in a.ranks if x > 1]:
        _, films = lockstep(g, n, keep=True)
        f = films[0]
        f.adaptive_kernel_times(reps=3)
        m, s, _r = f.adaptive_kernel_times(reps=a.reps)
        f.window_kernel_times(reps=3)
        ga, sc = f.window_kernel_times(reps=a.reps)
        kernels[f"packed_rank0_of_{n}"] = {"merge_tiles_ms": med(m), "tile_noise_with_err_ms": med(s), "gather_tiles_ms": med(ga),
                                          "scatter_tiles_ms": med(sc), "tiles": int(f.shard_info.own_tiles)}
        for x in films:
            x.close()
whole.close()
result["kernels"] = kernels
g.close()
print(json.dumps(result))
