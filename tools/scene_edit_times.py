"""What a light or material edit costs, against pt_scene_create, on config 3's workload (HostScene.generate_ps5(500000, 0, 8),
1920x1080, 128 spp, 5 bounces, FILMIC) and on the closed room (generator flag 4) lit by four point lights:
one JSON line with, per scene, pt_scene_create's seconds, the median pt_scene_set_lights time of moves of one point light and
of that light turned directional, the median pt_scene_set_materials time, the median first frame after each kind of edit
(every frame after an edit runs unplanned, as a first frame) and the median planned frame of the unedited scene.
    timeout -k 10 900 python tools/scene_edit_times.py [--tris 500000] [--edits 8] [--steady 8]
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


def light(kind, vec, color):
    return pta.Light(kind, (C.c_float * 3)(*vec), (C.c_float * 3)(*color), 0.1)


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def measure(label, host):
    t0 = time.perf_counter()
    g = pta.GpuScene(host, device=0)
    create_s = time.perf_counter() - t0
    frame = lambda: timed(lambda: g.render_device(prof, pta.Opts.make(), rgb.data_ptr(), acc.data_ptr(), 0))
    for _ in range(4):   # (first frames, escape masks, the plan)
        frame()
    steady = [frame() for _ in range(a.steady)]
    base = host.lights
    p0 = list(base[0].vec)
    r = math.hypot(p0[0], p0[2])
    others = base[1:]
    move_ms, move_first, dir_ms, dir_first, mat_ms, mat_first = [], [], [], [], [], []
    for k in range(a.edits):   # one point light moved along a circle about the vertical axis, at its height
        ang = math.atan2(p0[2], p0[0]) + 2 * math.pi * (k + 1) / (a.edits + 1)
        lights = [light(pta.PT_LIGHT_POINT, [r * math.cos(ang), p0[1], r * math.sin(ang)], list(base[0].color))] + others
        move_ms.append(timed(lambda: g.set_lights(lights)))
        move_first.append(frame())
    for k in range(a.edits):   # the same light turned directional (from a point light every time)
        g.set_lights(base)
        ang = 2 * math.pi * k / a.edits
        d = [0.4 * math.cos(ang), -1.0, 0.4 * math.sin(ang)]
        lights = [light(pta.PT_LIGHT_DIRECTIONAL, d, [3.0, 2.9, 2.8])] + others
        dir_ms.append(timed(lambda: g.set_lights(lights)))
        dir_first.append(frame())
    g.set_lights(base)
    mats = host.materials
    for k in range(a.edits):   # one material's albedo and roughness
        edited = [type(m).from_buffer_copy(bytes(C.string_at(C.addressof(m), C.sizeof(m)))) for m in mats]
        edited[0].albedo[0] = 0.2 + 0.05 * k
        edited[0].roughness = 0.3 + 0.05 * k
        mat_ms.append(timed(lambda: g.set_materials(edited)))
        mat_first.append(frame())
    info = g.info().as_dict()
    med = lambda v: round(statistics.median(v), 2)
    out = {"scene": label, "prims": int(info["n_prims"]), "lights": len(base), "scene_create_s": round(create_s, 3),
           "set_lights_move_ms_median": med(move_ms), "set_lights_move_ms": [round(v, 1) for v in move_ms],
           "first_frame_after_move_ms_median": med(move_first),
           "set_lights_to_directional_ms_median": med(dir_ms), "first_frame_after_to_directional_ms_median": med(dir_first),
           "set_materials_ms_median": med(mat_ms), "set_materials_ms": [round(v, 2) for v in mat_ms],
           "first_frame_after_materials_ms_median": med(mat_first),
           "steady_planned_frame_ms_median": med(steady), "light_grids": int(info["light_grids"])}
    g.close()
    return out


cfg3 = pta.HostScene.generate_ps5(a.tris, 0, 8)
room = pta.HostScene.generate_ps5(a.tris, 0, 4)
l0 = room.lights[0]
room.set_lights([l0] + [light(pta.PT_LIGHT_POINT, v, [800.0, 780.0, 760.0]) for v in ([-6.0, 8.0, -4.0], [5.0, 6.0, -6.0], [-3.0, 9.0, 6.0])])
print(json.dumps({"image": f"{a.width}x{a.height}", "spp": a.spp, "bounces": a.bounces, "tris": a.tris,
                  "scenes": [measure("config3", cfg3), measure("closed_room_4_point_lights", room)]}))
