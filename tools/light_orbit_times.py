"""What a frame costs while a light moves and the camera stays, on config 3's workload (HostScene.generate_ps5(500000, 0, 8),
1920x1080, 128 spp, 5 bounces, FILMIC): the case the camera-hit cache is for (DESIGN section 4 "The camera-hit cache").  One
JSON line with the scene's first frames one by one (the second is the one that fills the word cache and stores the camera
hits), the median steady frame, the frame after each of `--moves` moves of the first point light along a circle about the
vertical axis, and the numbers of the camera-hit, bounce-1 hit, bounce-2 hit and bounce-1 visibility caches where the library has them (an A/B library of an earlier commit, PT_GPU_LIB, has none).
    timeout -k 10 600 python tools/light_orbit_times.py [--tris 500000] [--moves 8] [--steady 8]
Needs the GPU; every step below is bounded by the caller's time limit."""
import argparse
import ctypes as C
import json
import math
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
ap.add_argument("--spp", type=int, default=128)
ap.add_argument("--bounces", type=int, default=5)
ap.add_argument("--moves", type=int, default=8)
ap.add_argument("--steady", type=int, default=8)
a = ap.parse_args()

pta = entry.load_package()
prof = pta.Profile.make(a.width, a.height, a.spp, a.bounces, "FILMIC")
n = a.width * a.height
rgb = torch.empty(n * 3, dtype=torch.uint8, device="cuda")
acc = torch.empty(n * 3, dtype=torch.float32, device="cuda")


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


host = pta.HostScene.generate_ps5(a.tris, 0, 8)
g = pta.GpuScene(host, device=0)
frame = lambda: timed(lambda: g.render_device(prof, pta.Opts.make(), rgb.data_ptr(), acc.data_ptr(), 0))
has_stats = hasattr(g.lib, "pt_get_hit_cache_stats")
stats = lambda: dict(zip(("bytes", "items", "cached", "stores", "loads"), g.hit_cache_stats())) if has_stats else None
has_hit1 = hasattr(g.lib, "pt_get_hit1_cache_stats")
hit1 = lambda: dict(zip(("bytes", "items", "cached", "resets", "stores", "loads", "unknown_casts"), g.hit1_cache_stats())) if has_hit1 else None
has_hit2 = hasattr(g.lib, "pt_get_hit2_cache_stats")
hit2 = lambda: dict(zip(("bytes", "items", "cached", "resets", "stores", "loads", "unknown_casts"), g.hit2_cache_stats())) if has_hit2 else None
has_vis1 = hasattr(g.lib, "pt_get_vis1_cache_stats")
vis1 = lambda: dict(zip(("bytes", "items", "resets", "launches"), g.vis1_cache_stats())) if has_vis1 else None
has_cont = hasattr(g.lib, "pt_get_cont_cache_stats")
cont = lambda: dict(zip(("bytes", "items", "cached", "resets", "stores", "loads", "missing"), g.cont_cache_stats())) if has_cont else None
first = [frame() for _ in range(5)]   # (the first frame, the filling and storing frame, escape masks, the plan, a steady one)
after_first = stats()
steady = [frame() for _ in range(a.steady)]
base = host.lights
p0 = list(base[0].vec)
r = math.hypot(p0[0], p0[2])
moved = []
for k in range(a.moves):
    ang = math.atan2(p0[2], p0[0]) + 2 * math.pi * (k + 1) / (a.moves + 1)
    lights = [pta.Light(pta.PT_LIGHT_POINT, (C.c_float * 3)(r * math.cos(ang), p0[1], r * math.sin(ang)),
                        (C.c_float * 3)(*base[0].color), 0.1)] + base[1:]
    g.set_lights(lights)
    moved.append(frame())
print(json.dumps({"image": f"{a.width}x{a.height}", "spp": a.spp, "bounces": a.bounces, "tris": a.tris,
                  "first_frames_ms": [round(v, 2) for v in first], "hit_cache_after_first_frames": after_first,
                  "steady_frame_ms_median": round(statistics.median(steady), 2),
                  "frame_after_light_move_ms": [round(v, 2) for v in moved],
                  "frame_after_light_move_ms_median": round(statistics.median(moved), 2), "hit_cache": stats(),
                  "hit1_cache": hit1(), "hit2_cache": hit2(), "vis1_cache": vis1(), "cont_cache": cont()}))
g.close()
