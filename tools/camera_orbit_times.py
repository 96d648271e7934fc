"""What a camera change costs on config 3's workload (bench.py's defaults: HostScene.generate_ps5(500000, 0, 8), 1920x1080,
128 spp, 5 bounces, FILMIC):
one JSON line with pt_scene_create's seconds, the median pt_scene_set_camera time, the median first frame after a move
(every frame after a move runs unplanned, as a first frame) and the median planned frame at a fixed camera.
    timeout -k 10 600 python tools/camera_orbit_times.py [--tris 500000] [--moves 8] [--steady 8]
Needs the GPU; every step below is bounded by the caller's time limit."""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
import torch  # noqa: E402
torch.zeros(1, device="cuda")   # (torch's HIP context first, as bench.py)
import __graft_entry__ as entry  # noqa: E402
import make_orbit  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--tris", type=int, default=500000)
ap.add_argument("--width", type=int, default=1920)
ap.add_argument("--height", type=int, default=1080)
ap.add_argument("--spp", type=int, default=128)
ap.add_argument("--scene-flags", type=int, default=8)
ap.add_argument("--bounces", type=int, default=5)
ap.add_argument("--moves", type=int, default=8)
ap.add_argument("--steady", type=int, default=8)
a = ap.parse_args()

pta = entry.load_package()
host = pta.HostScene.generate_ps5(a.tris, 0, a.scene_flags)
prof = pta.Profile.make(a.width, a.height, a.spp, a.bounces, "FILMIC")
n = a.width * a.height
rgb = torch.empty(n * 3, dtype=torch.uint8, device="cuda")
acc = torch.empty(n * 3, dtype=torch.float32, device="cuda")
t0 = time.perf_counter()
g = pta.GpuScene(host, device=0)
create_s = time.perf_counter() - t0


def frame():
    torch.cuda.synchronize()
    t = time.perf_counter()
    g.render_device(prof, pta.Opts.make(), rgb.data_ptr(), acc.data_ptr(), 0)
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


for _ in range(4):   # (first frames, escape masks, the plan of the scene camera)
    frame()
steady = [frame() for _ in range(a.steady)]
cams = make_orbit.orbit(host, a.moves + 1)[1:]
set_ms, first_ms = [], []
has_hits = hasattr(g.lib, "pt_get_hit_cache_stats")   # (an A/B library of an earlier commit, PT_GPU_LIB, has none)
stores_before = g.hit_cache_stats()[3] if has_hits else None
for cam in cams:
    torch.cuda.synchronize()
    t = time.perf_counter()
    g.set_camera(cam)
    set_ms.append((time.perf_counter() - t) * 1e3)
    first_ms.append(frame())
info = g.info().as_dict()
print(json.dumps({"tris": a.tris, "prims": int(info["n_prims"]), "image": f"{a.width}x{a.height}", "spp": a.spp,
                  "bounces": a.bounces, "scene_create_s": round(create_s, 3),
                  "set_camera_ms_median": round(statistics.median(set_ms), 2), "set_camera_ms": [round(v, 1) for v in set_ms],
                  "first_frame_after_move_ms_median": round(statistics.median(first_ms), 2),
                  "steady_planned_frame_ms_median": round(statistics.median(steady), 2),
                  "cam_grid_res": int(info["cam_grid_res"]),
                  # the camera-hit cache stores at a view's second frame: a camera path must never store
                  "hit_cache_stores_during_moves": g.hit_cache_stats()[3] - stores_before if has_hits else None}))
