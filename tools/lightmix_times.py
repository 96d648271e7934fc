"""What the light mixer costs and saves on config 3's workload (HostScene.generate_ps5(500000, 0, 8) given --lights point
lights, 1920x1080): one JSON line with the capture (host wall time, n_lights + 1 frames), k_lightmix_apply with rgb8 alone and
with rgb8 + accum (HIP events, median of --reps) and the rate its compulsory traffic makes of that, a colour-edit frame
rendered the usual way on a second scene of the same code (pt_scene_set_lights + pt_render_device in the steady state) timed
alternately with the mix of the same colours, and pt_measure_copy_bandwidth as the yardstick.
    timeout -k 10 600 python tools/lightmix_times.py [--lights 4] [--spp 128] [--reps 20]
Needs the GPU; every step is bounded by the caller's time limit."""
import argparse
import ctypes as C
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
ap.add_argument("--spp", type=int, default=128)
ap.add_argument("--bounces", type=int, default=5)
ap.add_argument("--lights", type=int, default=4)
ap.add_argument("--reps", type=int, default=20)
a = ap.parse_args()

pta = entry.load_package()
w, h, n = a.width, a.height, a.width * a.height
prof = pta.Profile.make(w, h, a.spp, a.bounces, "FILMIC")
host = pta.HostScene.generate_ps5(a.tris, 0, 8)
first = host.lights[0]
p0 = np.array(list(first.vec), np.float64)
lights = []
for k in range(a.lights):   # the scene's light and copies of it nearby, in other colours
    l = type(first).from_buffer_copy(first)
    for j in range(3):
        l.vec[j] = float(p0[j] + (0.0 if k == 0 else 0.15 * abs(p0).max() * ((k * (j + 2)) % 3 - 1)))
        l.color[j] = float(first.color[j] * (1.0, 0.6, 0.3, 0.8)[(k + j) % 4])
    lights.append(l)
host.set_lights(lights)
g, other = pta.GpuScene(host, device=0), pta.GpuScene(host, device=0)
rgb = torch.empty(n * 3, dtype=torch.uint8, device="cuda")
acc = torch.empty(n * 3, dtype=torch.float32, device="cuda")
med = lambda v: round(statistics.median(v), 4)


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def events(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def colours(k):
    out = np.array([[l.color[0], l.color[1], l.color[2]] for l in lights], np.float32)
    return out * np.float32(0.5 + 0.1 * (k % 7))


def recoloured(k):
    out = []
    for l, c in zip(lights, colours(k)):
        m = type(l).from_buffer_copy(l)
        m.color[0], m.color[1], m.color[2] = float(c[0]), float(c[1]), float(c[2])
        out.append(m)
    return out


frame = lambda s: timed(lambda: s.render_device(prof, pta.Opts.make(), rgb.data_ptr(), acc.data_ptr(), 0))
for _ in range(4):   # (first frames, escape masks, the plan, the keyed caches)
    frame(g), frame(other)
steady_ms = med([frame(other) for _ in range(5)])
holder = []
capture_ms = timed(lambda: holder.append(g.lightmix_capture(prof)))
mix = holder[0]
stream = torch.cuda.current_stream().cuda_stream
mix_rgb = lambda k: events(lambda: mix.apply_device(colours(k), "FILMIC", rgb.data_ptr(), 0, stream))
mix_both = lambda k: events(lambda: mix.apply_device(colours(k), "FILMIC", rgb.data_ptr(), acc.data_ptr(), stream))
for k in range(3):
    mix_rgb(k), mix_both(k)
apply_rgb_ms = med([mix_rgb(k) for k in range(a.reps)])
apply_both_ms = med([mix_both(k) for k in range(a.reps)])


def edit_frame(k):   # what a colour edit costs without the mixer: the edit (grids rebuilt, plans dropped) and its frame
    return timed(lambda: (other.set_lights(recoloured(k)),
                          other.render_device(prof, pta.Opts.make(), rgb.data_ptr(), acc.data_ptr(), 0)))


rows = [(edit_frame(k), timed(lambda: mix.apply_device(colours(k), "FILMIC", rgb.data_ptr(), 0, stream))) for k in range(a.reps)]
read_mb = (a.lights + 1) * n * 12 / 1e6
info = mix.info
out = {"image": f"{w}x{h}", "tris": a.tris, "spp": a.spp, "bounces": a.bounces, "lights": a.lights,
       "steady_frame_ms": steady_ms, "capture_ms": round(capture_ms, 3), "planes_mb": round(info.device_bytes / 1e6, 1),
       "apply_rgb8_ms": apply_rgb_ms, "apply_rgb8_accum_ms": apply_both_ms,
       "apply_read_mb": round(read_mb, 1), "apply_rgb8_gb_per_s": round((read_mb + n * 3 / 1e6) / apply_rgb_ms, 1),
       "apply_rgb8_accum_gb_per_s": round((read_mb + n * 15 / 1e6) / apply_both_ms, 1),
       "colour_edit_frame_ms": med([r[0] for r in rows]), "colour_edit_mixed_wall_ms": med([r[1] for r in rows]),
       "copy_bandwidth_gb_per_s": round(pta.measure_copy_bandwidth(0, 1 << 30, 5), 1)}
print(json.dumps(out))
