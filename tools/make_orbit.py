"""A turntable camera path for `path-tracer render --camera-path`:
    python tools/make_orbit.py SCENE.isf N [--axis y] [-o cams.json]
N cameras: the scene camera's transform rotated by 2 pi i / N about the axis (x, y or z) through the centre of the scene's
bounding box (vertices of every triangle, centre -+ radius of every sphere).  Frame 0 is the scene camera exactly; fov,
zfar and znear are kept.  Host only (libpthost.so)."""
import argparse
import json
import math
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def scene_box_centre(host_scene):
    import numpy as np
    d = host_scene.desc.contents
    lo, hi = np.full(3, np.inf), np.full(3, -np.inf)
    if d.n_triangles:
        tri = np.ctypeslib.as_array(d.triangles, (int(d.n_triangles) * 24,)).reshape(-1, 3, 8)[:, :, :3].reshape(-1, 3)
        lo, hi = np.minimum(lo, tri.min(axis=0)), np.maximum(hi, tri.max(axis=0))
    for m in range(d.n_models):
        mo = d.models[m]
        if mo.kind == 1:   # PT_MODEL_SPHERE
            c = np.array(list(mo.center), np.float64)
            lo, hi = np.minimum(lo, c - abs(mo.radius)), np.maximum(hi, c + abs(mo.radius))
    if not np.all(np.isfinite(lo)) or not np.all(np.isfinite(hi)):
        return np.zeros(3)
    return 0.5 * (lo.astype(np.float64) + hi.astype(np.float64))


def orbit(host_scene, n, axis="y"):
    """List of n cameras in ISF form (dicts); [0] is the scene camera."""
    import numpy as np
    pta = _pta()
    base = host_scene.camera
    pivot = scene_box_centre(host_scene)
    M = np.array(list(base.transform), np.float64).reshape(4, 4).T   # columns of the ISF transform -> matrix
    a = "xyz".index(axis)
    cams = [pta.camera_to_dict(base)]
    for i in range(1, n):
        t = 2.0 * math.pi * i / n
        c, s = math.cos(t), math.sin(t)
        R = np.eye(4)
        b, e = (a + 1) % 3, (a + 2) % 3   # right-handed rotation about axis a: b -> e
        R[b, b], R[b, e], R[e, b], R[e, e] = c, -s, s, c
        T, Ti = np.eye(4), np.eye(4)
        T[:3, 3], Ti[:3, 3] = pivot, -pivot
        N = (T @ R @ Ti @ M).astype(np.float32)
        cam = pta.Camera((pta.C.c_float * 16)(*[float(v) for v in N.T.reshape(-1)]), base.fov, base.zfar, base.znear)
        cams.append(pta.camera_to_dict(cam))
    return cams


def _pta():
    import importlib.util
    spec = importlib.util.spec_from_file_location("__graft_entry__", ROOT / "__graft_entry__.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.load_package()


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("scene")
    ap.add_argument("n", type=int)
    ap.add_argument("--axis", choices=("x", "y", "z"), default="y")
    ap.add_argument("-o", "--output", default="cams.json")
    a = ap.parse_args(argv)
    if a.n < 1:
        ap.error("N must be at least 1")
    pta = _pta()
    scene = pta.HostScene.load_isf(a.scene)
    cams = orbit(scene, a.n, a.axis)
    Path(a.output).write_text(json.dumps(cams, indent=1) + "\n")
    print(f"{a.output}: {len(cams)} cameras about the {a.axis} axis")


if __name__ == "__main__":
    main()
