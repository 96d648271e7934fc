"""What the AOV pass costs on config 3's workload (HostScene.generate_ps5(500000, 0, 8), 1920x1080): one JSON line with
pt_render_aov_device through the camera grid and through the KD-tree (PT_FLAG_NO_GRIDS), k_aov_guides, the pixel-centre guide
pass (k_guides) and the frame of the same sample count, at 4 and at 128 samples per pixel.  Host clock around work that ends in
a device synchronise, medians of --reps, after warm-up.
    timeout -k 10 600 python tools/aov_times.py [--reps 20] [--spp 4,128]
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
ap.add_argument("--spp", default="4,128")
ap.add_argument("--bounces", type=int, default=5)
ap.add_argument("--reps", type=int, default=20)
a = ap.parse_args()

pta = entry.load_package()
w, h, n = a.width, a.height, a.width * a.height
g = pta.GpuScene(pta.HostScene.generate_ps5(a.tris, 0, 8), device=0)
rgb = torch.empty(n * 3, dtype=torch.uint8, device="cuda")
acc = torch.empty(n * 3, dtype=torch.float32, device="cuda")
aov = torch.empty(n * pta.PT_AOV_FLOATS, dtype=torch.float32, device="cuda")
guides = torch.empty(n * pta.PT_GUIDE_FLOATS, dtype=torch.float32, device="cuda")
med = lambda v: round(statistics.median(v), 4)


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def series(fn, reps, warm=2):
    for _ in range(warm):
        fn()
    return med([fn() for _ in range(reps)])


out = {"image": f"{w}x{h}", "tris": a.tris, "bounces": a.bounces, "reps": a.reps, "translucent": bool(g.info().has_translucent),
       "cam_grid_res": int(g.info().cam_grid_res)}
out["k_guides_ms"] = series(lambda: timed(lambda: g.render_guides_device(w, h, guides.data_ptr(), 0)), a.reps)
for spp in (int(s) for s in a.spp.split(",")):
    prof = pta.Profile.make(w, h, spp, a.bounces, "FILMIC")
    row = {}
    row["frame_ms"] = series(lambda: timed(lambda: g.render_device(prof, pta.Opts.make(), rgb.data_ptr(), acc.data_ptr(), 0)),
                             8 if spp <= 16 else 5, warm=4 if spp <= 16 else 2)
    for label, flags in (("aov_grid_ms", 0), ("aov_kd_ms", pta.PT_FLAG_NO_GRIDS)):
        row[label] = series(lambda: timed(lambda: g.render_aov_device(prof, pta.Opts.make(flags=flags), aov.data_ptr(), 0, 0)), a.reps)
    row["aov_guides_ms"] = series(lambda: timed(lambda: pta.check_gpu(pta.gpu_lib().pt_aov_guides_device(
        0, n, spp, aov.data_ptr(), guides.data_ptr(), 0))), a.reps)
    row["covered_pixel_fraction"] = round(float((aov.view(n, 16)[:, 7] > 0).float().mean()), 4)
    row["aov_over_frame"] = round(row["aov_grid_ms"] / row["frame_ms"], 4)
    out[f"spp{spp}"] = row
print(json.dumps(out))
