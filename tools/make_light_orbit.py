"""A point light circling the scene, as keyframes for `path-tracer render --keyframes`:
    python tools/make_light_orbit.py SCENE.isf N [--light 0] [--axis y] [-o frames.json]
N frames: frame i replaces the scene's lights by the same list with light `--light` (a point light) rotated by 2 pi i / N about
the axis (x, y or z) through the centre of the scene's bounding box.  Frame 0 is the scene's own lighting ({}); colour and
size are kept.  Host only (libpthost.so)."""
import argparse
import json
import math
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))
from make_orbit import _pta, scene_box_centre  # noqa: E402


def isf_light(light):
    """The ISF form of a Light (f32 values as Python floats: they round-trip exactly)."""
    if light.kind == 0:   # PT_LIGHT_POINT
        return {"type": "Point", "position": list(light.vec), "color": list(light.color), "size": light.size}
    return {"type": "Directional", "direction": list(light.vec), "color": list(light.color)}


def light_orbit(host_scene, n, which=0, axis="y"):
    """List of n keyframes (dicts); [0] is {} (the scene's lights)."""
    import numpy as np
    lights = host_scene.lights
    if not 0 <= which < len(lights) or lights[which].kind != 0:
        raise ValueError(f"light {which} is not a point light of the scene")
    pivot = scene_box_centre(host_scene)
    p = np.array(list(lights[which].vec), np.float64) - pivot
    a = "xyz".index(axis)
    b, e = (a + 1) % 3, (a + 2) % 3   # right-handed rotation about axis a: b -> e
    frames = [{}]
    for i in range(1, n):
        t = 2.0 * math.pi * i / n
        c, s = math.cos(t), math.sin(t)
        q = p.copy()
        q[b], q[e] = c * p[b] - s * p[e], s * p[b] + c * p[e]
        ls = [isf_light(l) for l in lights]
        ls[which]["position"] = [float(np.float32(v)) for v in pivot + q]
        frames.append({"lights": ls})
    return frames


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("scene")
    ap.add_argument("n", type=int)
    ap.add_argument("--light", type=int, default=0)
    ap.add_argument("--axis", choices=("x", "y", "z"), default="y")
    ap.add_argument("-o", "--output", default="frames.json")
    a = ap.parse_args(argv)
    if a.n < 1:
        ap.error("N must be at least 1")
    pta = _pta()
    scene = pta.HostScene.load_isf(a.scene)
    try:
        frames = light_orbit(scene, a.n, a.light, a.axis)
    except ValueError as e:
        ap.error(str(e))
    Path(a.output).write_text(json.dumps(frames, indent=1) + "\n")
    print(f"{a.output}: {len(frames)} frames, light {a.light} about the {a.axis} axis")


if __name__ == "__main__":
    main()
