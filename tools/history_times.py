"""What the temporal history costs on config 3's workload (HostScene.generate_ps5(500000, 0, 8), 1920x1080), along a turntable
of one degree a frame: one JSON line with, at 4 and at 128 samples per pixel, the medians of --reps after warm-up of
    frame_ms        pt_render_moments_device (host clock around a device synchronise)
    aov_ms          pt_render_aov_device
    add_frame_ms    pt_history_add_frame (frame or window frame, AOV pass, k_hist_advance, k_aov_guides) along the orbit
    advance_ms      k_hist_advance alone (pt_history_kernel_times: HIP events)
    filter_ms       pt_history_denoise_device, variance-guided at its defaults
and the bytes k_hist_advance moves (per pixel: 64 B of AOV record, 20 B of frame sums, 56 B written, and - where a source is
found - 24 B of its sums and count and 32 B of its surface, counted for every pixel) over its time, as a fraction of
pt_measure_copy_bandwidth on the same run.
    timeout -k 10 900 python tools/history_times.py [--reps 20] [--spp 4,128] > profiles/history_times.txt
Needs the GPU; every step is bounded by the caller's time limit."""
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
ap.add_argument("--spp", default="4,128")
ap.add_argument("--bounces", type=int, default=5)
ap.add_argument("--reps", type=int, default=20)
a = ap.parse_args()

pta = entry.load_package()
w, h, n = a.width, a.height, a.width * a.height
host = pta.HostScene.generate_ps5(a.tris, 0, 8)
cams = make_orbit.orbit(host, 360)
g = pta.GpuScene(host, device=0)
acc = torch.empty(n * 3, dtype=torch.float32, device="cuda")
mom = torch.empty(n * 2, dtype=torch.float32, device="cuda")
aov = torch.empty(n * pta.PT_AOV_FLOATS, dtype=torch.float32, device="cuda")
rgb = torch.empty(n * 3, dtype=torch.uint8, device="cuda")
med = lambda v: round(statistics.median(v), 4)
BYTES_PER_PIXEL = 64 + 20 + 56 + 24 + 32


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


out = {"image": f"{w}x{h}", "tris": a.tris, "bounces": a.bounces, "reps": a.reps,
       "copy_gb_per_s": round(pta.measure_copy_bandwidth(0, 1 << 30, 5), 1), "bytes_per_pixel": BYTES_PER_PIXEL}
for spp in (int(s) for s in a.spp.split(",")):
    reps = a.reps if spp <= 16 else max(3, a.reps // 4)
    prof = pta.Profile.make(w, h, spp, a.bounces, "FILMIC")
    row = {}
    for rotate in (1, pta.HistoryParams.default().rotate):
        hist = pta.History(w, h, pta.HistoryParams.default(rotate=rotate, max_samples=4 * spp))
        times = []
        for f in range(2 + reps):
            g.set_camera(cams[f])
            times.append(timed(lambda: hist.add_frame(g, prof, f)))
        row[f"add_frame_rotate{rotate}_ms"] = med(times[2:])
        if rotate == 1:
            row["reprojected_share"] = round(float((hist.read_map() >= 0).mean()), 4)
            row["advance_ms"] = med([float(v) for v in hist.kernel_times(reps)])
            params = pta.DenoiseParams.default_var()
            flt = lambda: hist.denoise_device(params, 1, rgb.data_ptr(), acc.data_ptr())
            if spp >= 2:
                flt()
                row["filter_ms"] = med([timed(flt) for _ in range(reps)])
        hist.close()
    frame = lambda: g.render_moments_device(prof, pta.Opts.make(), None, acc.data_ptr(), mom.data_ptr(), 0)
    for _ in range(3):
        frame()
    row["frame_ms"] = med([timed(frame) for _ in range(reps)])
    pass_ = lambda: g.render_aov_device(prof, pta.Opts.make(), aov.data_ptr(), 0, 0)
    pass_()
    row["aov_ms"] = med([timed(pass_) for _ in range(reps)])
    gbs = BYTES_PER_PIXEL * n / (row["advance_ms"] * 1e-3) / 1e9
    row["advance_gb_per_s"] = round(gbs, 1)
    row["advance_over_copy"] = round(gbs / out["copy_gb_per_s"], 3)
    out[f"spp{spp}"] = row
print(json.dumps(out))
