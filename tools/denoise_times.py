"""What a denoised preview costs on config 3's workload (HostScene.generate_ps5(500000, 0, 8), 1920x1080): one JSON line with
the guide pass, the filter's prep / per-pass / finish kernels (HIP events, medians) and their total, beside the frame time
at --spp samples and each pass's compulsory traffic (read 32 B + write 16 B per pixel) as a rate.  With --ab the passes are
also timed with PT_DN_LDS=0: steps 1 and 2 through global gathers instead of the LDS tile with a halo.  With --variance the
line also carries "variance": the frame with moments (pt_render_moments_device) against the same frame without, alternating,
at --spp and at 128 spp, and the stages of pt_denoise_var beside pt_denoise's on the same inputs (a pass reads the same two
16-byte planes per tap and writes 16 B: the same compulsory 48 B per pixel).
    timeout -k 10 600 python tools/denoise_times.py [--spp 4] [--iterations 5] [--reps 20] [--ab] [--variance]
Needs the GPU; every step is bounded by the caller's time limit."""
import argparse
import ctypes as C
import json
import os
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
ap.add_argument("--spp", type=int, default=4)
ap.add_argument("--bounces", type=int, default=5)
ap.add_argument("--iterations", type=int, default=5)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--ab", action="store_true")
ap.add_argument("--variance", action="store_true")
a = ap.parse_args()

pta = entry.load_package()
lib = pta.gpu_lib()
w, h, n = a.width, a.height, a.width * a.height
prof = pta.Profile.make(w, h, a.spp, a.bounces, "FILMIC")
g = pta.GpuScene(pta.HostScene.generate_ps5(a.tris, 0, 8), device=0)
rgb = torch.empty(n * 3, dtype=torch.uint8, device="cuda")
acc = torch.empty(n * 3, dtype=torch.float32, device="cuda")
col = torch.empty(n * 3, dtype=torch.float32, device="cuda")
guides = torch.empty(n * pta.PT_GUIDE_FLOATS, dtype=torch.float32, device="cuda")
scratch = torch.empty(pta.denoise_scratch_bytes(w, h), dtype=torch.uint8, device="cuda")
med = lambda v: round(statistics.median(v), 4)


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


frame = lambda: timed(lambda: g.render_device(prof, pta.Opts.make(), rgb.data_ptr(), acc.data_ptr(), 0))
for _ in range(4):   # (first frames, escape masks, the plan)
    frame()
frame_ms = med([frame() for _ in range(8)])
prof_full = pta.Profile.make(w, h, 128, a.bounces, "FILMIC")   # (the frame the previews stand in for: bench.py's)
full = lambda: timed(lambda: g.render_device(prof_full, pta.Opts.make(), rgb.data_ptr(), acc.data_ptr(), 0))
for _ in range(3):
    full()
frame_128spp_ms = med([full() for _ in range(5)])
frame()   # (the accumulator of the low-spp frame again)
guide = lambda: timed(lambda: g.render_guides_device(w, h, guides.data_ptr(), 0))
guide()
guides_ms = med([guide() for _ in range(a.reps)])
valid = float((guides.view(n, 8)[:, 3] >= 0).float().mean())


def stages(params, moments=None):
    ms = (C.c_float * pta.PT_DENOISE_STAGES)()
    rows = []
    for k in range(a.reps + 2):
        if moments is None:
            pta.check_gpu(lib.pt_denoise_stage_times(0, w, h, a.spp, C.byref(params), acc.data_ptr(), guides.data_ptr(), col.data_ptr(),
                                                     rgb.data_ptr(), scratch.data_ptr(), ms))
        else:
            pta.check_gpu(lib.pt_denoise_var_stage_times(0, w, h, a.spp, C.byref(params), acc.data_ptr(), moments.data_ptr(),
                                                         guides.data_ptr(), col.data_ptr(), rgb.data_ptr(), scratch.data_ptr(), ms))
        if k >= 2:
            rows.append(list(ms))
    m = [med([r[j] for r in rows]) for j in range(pta.PT_DENOISE_STAGES)]
    passes = m[1:1 + params.iterations]
    return {"prep_ms": m[0], "pass_ms": passes, "finish_ms": m[-1], "total_ms": round(m[0] + sum(passes) + m[-1], 4),
            "pass_compulsory_gb_per_s": [round(48.0 * n / (p * 1e-3) / 1e9, 1) if p > 0 else None for p in passes]}


params = pta.DenoiseParams.default(iterations=a.iterations)
out = {"image": f"{w}x{h}", "tris": a.tris, "spp": a.spp, "bounces": a.bounces, "frame_ms": frame_ms, "frame_128spp_ms": frame_128spp_ms, "guides_ms": guides_ms,
       "valid_pixel_fraction": round(valid, 4), "iterations": a.iterations, "pass_compulsory_mb": round(48.0 * n / 1e6, 1),
       "scratch_mb": round(scratch.numel() / 1e6, 1)}
os.environ.pop("PT_DN_LDS", None)
out["filter"] = stages(params)
if a.ab:
    os.environ["PT_DN_LDS"] = "0"
    out["filter_global_gathers_only"] = stages(params)
    os.environ.pop("PT_DN_LDS", None)
dflt = pta.DenoiseParams.default()
out["defaults"] = dict({k: getattr(dflt, k) for k, _ in dflt._fields_}, **stages(dflt))
end_to_end = lambda: timed(lambda: g.render_denoised(prof, dflt))
end_to_end()
out["render_denoised_host_ms"] = med([end_to_end() for _ in range(5)])
if a.variance:
    mom = torch.empty(n * 2, dtype=torch.float32, device="cuda")
    var = {}
    for label, p in (("frame", prof), ("frame_128spp", prof_full)):
        plain = lambda: timed(lambda: g.render_device(p, pta.Opts.make(), rgb.data_ptr(), acc.data_ptr(), 0))
        with_m = lambda: timed(lambda: g.render_moments_device(p, pta.Opts.make(), rgb.data_ptr(), acc.data_ptr(), mom.data_ptr(), 0))
        for _ in range(2):
            plain(), with_m()
        rows = [(plain(), with_m()) for _ in range(a.reps)]   # alternating: drift hits both alike
        var[label + "_ms"] = med([r[0] for r in rows])
        var[label + "_moments_ms"] = med([r[1] for r in rows])
        var[label + "_spread_ms"] = round(max(r[0] for r in rows) - min(r[0] for r in rows), 4)
    plain(), frame(), timed(lambda: g.render_moments_device(prof, pta.Opts.make(), rgb.data_ptr(), acc.data_ptr(), mom.data_ptr(), 0))
    vd = pta.DenoiseParams.default_var()
    same = pta.DenoiseParams.default_var(iterations=a.iterations)
    var["filter"] = stages(same, mom)
    var["filter_plain_same_parameters"] = stages(same)
    var["defaults"] = dict({k: getattr(vd, k) for k, _ in vd._fields_}, **stages(vd, mom))
    e2e = lambda: timed(lambda: g.render_denoised_var(prof, vd))
    e2e()
    var["render_denoised_var_host_ms"] = med([e2e() for _ in range(5)])
    out["variance"] = var
print(json.dumps(out))
