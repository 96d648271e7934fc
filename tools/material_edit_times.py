"""What a frame costs after a material edit and after a light-colour edit while camera and light positions stay, on config 3's
workload (HostScene.generate_ps5(500000, 0, 8), 1920x1080, 128 spp, 5 bounces, FILMIC): the cases the shadow-visibility cache
is for (DESIGN section 4 "The shadow-visibility cache").  One JSON line with the scene's first five frames one by one (the
second stores the camera hits and zeroes the visibility plane, the third fills it), the median steady frame, the frame after
each of `--edits` material edits (every albedo scaled), after each of as many colour-only edits of the first light, and - the
control - after each of as many MOVES of that light, with the planes zeroed and the launches of the visibility variant
during the moves (both must be zero), and the numbers of the bounce-2 hit and bounce-1 visibility caches, where the library has the numbers (an A/B library of an earlier commit, PT_GPU_LIB,
has none).
    timeout -k 10 600 python tools/material_edit_times.py [--tris 500000] [--edits 8] [--steady 8]
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
ap.add_argument("--edits", type=int, default=8)
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
has_stats = hasattr(g.lib, "pt_get_vis_cache_stats")
stats = lambda: dict(zip(("bytes", "items", "resets", "launches"), g.vis_cache_stats())) if has_stats else None
has_hit2 = hasattr(g.lib, "pt_get_hit2_cache_stats")
hit2 = lambda: dict(zip(("bytes", "items", "cached", "resets", "stores", "loads", "unknown_casts"), g.hit2_cache_stats())) if has_hit2 else None
has_vis1 = hasattr(g.lib, "pt_get_vis1_cache_stats")
vis1 = lambda: dict(zip(("bytes", "items", "resets", "launches"), g.vis1_cache_stats())) if has_vis1 else None
first = [frame() for _ in range(5)]
after_first = stats()
steady = [frame() for _ in range(a.steady)]

d = host.desc.contents
mats = [pta.Material.from_buffer_copy(d.materials[k]) for k in range(d.n_materials)]
after_material = []
for k in range(a.edits):
    table = [pta.Material.from_buffer_copy(m) for m in mats]
    for m in table:
        for c in range(3):
            m.albedo[c] = m.albedo[c] * (0.5 + 0.05 * k)
    g.set_materials(table)
    after_material.append(frame())
g.set_materials(mats)
frame()

base = host.lights
after_colour = []
for k in range(a.edits):
    first_light = pta.Light(base[0].kind, (C.c_float * 3)(*base[0].vec), (C.c_float * 3)(*[v * (0.6 + 0.05 * k) for v in base[0].color]), 0.1)
    g.set_lights([first_light] + base[1:])
    after_colour.append(frame())
before_moves = stats()

p0 = list(base[0].vec)
r = math.hypot(p0[0], p0[2])
after_move = []
for k in range(a.edits):
    ang = math.atan2(p0[2], p0[0]) + 2 * math.pi * (k + 1) / (a.edits + 1)
    lights = [pta.Light(pta.PT_LIGHT_POINT, (C.c_float * 3)(r * math.cos(ang), p0[1], r * math.sin(ang)),
                        (C.c_float * 3)(*base[0].color), 0.1)] + base[1:]
    g.set_lights(lights)
    after_move.append(frame())
end = stats()
r2 = lambda v: [round(x, 2) for x in v]
print(json.dumps({"image": f"{a.width}x{a.height}", "spp": a.spp, "bounces": a.bounces, "tris": a.tris,
                  "first_frames_ms": r2(first), "vis_cache_after_first_frames": after_first,
                  "steady_frame_ms_median": round(statistics.median(steady), 2),
                  "frame_after_material_edit_ms": r2(after_material),
                  "frame_after_material_edit_ms_median": round(statistics.median(after_material), 2),
                  "frame_after_colour_edit_ms": r2(after_colour),
                  "frame_after_colour_edit_ms_median": round(statistics.median(after_colour), 2),
                  "frame_after_light_move_ms": r2(after_move),
                  "frame_after_light_move_ms_median": round(statistics.median(after_move), 2),
                  "resets_during_moves": end["resets"] - before_moves["resets"] if has_stats else None,
                  "launches_during_moves": end["launches"] - before_moves["launches"] if has_stats else None,
                  "vis_cache": end, "hit2_cache": hit2(), "vis1_cache": vis1()}))
g.close()
