"""The `specks` family for the origin grids (host/og_raster.h sphere_footprint), next to the families of tests/escape_scenes.py:
spheres so small against their distance D from the grid's origin that r^2 drowns in the float32 rounding of the reference's
quadratic (c = |o - centre|^2 - r^2 and b^2 - 4ac are formed at magnitude D^2), set against a wall that faces the origin.

  walls    four squares of half-side 0.25 k that face the camera from D = 0.3, 3.1, 30 and 300 (k = D / |eye|, |eye| = 3.096), in
           four directions 0.23 rad off the view axis so that none hides another;
  specks   on every wall 5 radii x 7 placements: r = k x (3e-4, 1e-3, 3e-3, 1e-2, 3e-2) (r / D from 1e-4 to 1e-2), each in front
           of the wall and tangent to it, sunk halfway, and entirely behind it by gaps of k x (5e-5, 1e-4, 2e-4, 3e-4, 1e-3) - the
           wall at 3.1 with r = 1e-3 and the gap 2e-4 is the case in which the parent's distance bound let the walk return the wall;
  floor    8 x 8 quads of 0.1 beside the walls (as the camera sees them) with the same 35 specks on, in and under it: under the
           point light (2.9 away) and the directional light.
Instance 0 is flat, 1 is tilted by escape_scenes.TILT, 2 is translated by (1000, -2000, 500)."""
import numpy as np

import escape_scenes as es

EYE = 3.0 * np.array([0.35, 0.55, 0.8])     # where escape_scenes.build puts the camera for centre 0, extent 3
D0 = float(np.linalg.norm(EYE))
WALL_D = (0.3, D0, 30.0, 300.0)
RADII = (3e-4, 1e-3, 3e-3, 1e-2, 3e-2)      # x k
GAPS = (5e-5, 1e-4, 2e-4, 3e-4, 1e-3)       # x k
PLACEMENTS = ("front", "sunk") + GAPS
INSTANCES = (0, 1, 2)
SHIFT = (1000.0, -2000.0, 500.0)


def _frame():
    a = -EYE / D0
    u = np.cross(a, [0.0, 1.0, 0.0])
    u /= np.linalg.norm(u)
    return a, u, np.cross(u, a)


def _specks(models, info, prim, where, foot, normal, su, sw, k):
    """35 spheres around `foot` on the plane with unit `normal` (towards the origin), spread along su / sw."""
    for i, r in enumerate(RADII):
        for j, place in enumerate(PLACEMENTS):
            p = foot + su * (0.08 * k * (i - 2)) + sw * (0.065 * k * (j - 3))
            rr = r * k
            off = rr if place == "front" else (0.0 if place == "sunk" else -(rr + place * k))
            models.append(es.sphere(p + normal * off, rr))
            info.append(dict(where=where, prim=prim, r=r, place=place, k=k))
            prim += 1
    return prim


def layout():
    """(models, speck records) in the local frame: record = dict(where: wall number or 'floor', prim, r and place as in RADII /
    PLACEMENTS (unscaled), k)."""
    a, u, w = _frame()
    models, info, prim = [], [], 0
    for n, (D, (fu, fw)) in enumerate(zip(WALL_D, ((0.16, 0.16), (0.16, -0.16), (0.02, 0.16), (0.02, -0.16)))):
        d = a + fu * u + fw * w
        d /= np.linalg.norm(d)
        k = D / D0
        c = EYE + D * d
        pu = np.cross(d, w)
        pu /= np.linalg.norm(pu)
        pw = np.cross(pu, d)
        s = 0.25 * k
        q = [c - s * pu - s * pw, c + s * pu - s * pw, c + s * pu + s * pw, c - s * pu + s * pw]
        models.append(es.mesh([[q[0], q[1], q[2]], [q[0], q[2], q[3]]], floor=f"wall{n}"))
        prim += 2
        prim = _specks(models, info, prim, n, c, -d, pu, pw, k)
    # the floor: y = 0, where the direction a - 0.45 u from the eye meets it
    d = a - 0.45 * u
    f = EYE + d * (EYE[1] / -d[1])
    models.append(es.mesh(es.patch(f[0] - 0.4, f[2] - 0.4, 8, 8, 0.1), floor="floor"))
    prim += 128
    _specks(models, info, prim, "floor", f, np.array([0.0, 1.0, 0.0]), np.array([1.0, 0.0, 0.0]), np.array([0.0, 0.0, 1.0]), 1.0)
    return models, info


def make(pta, instance=0):
    """(BuiltScene, floors, speck records) of one instance."""
    models, info = layout()
    R = es.TILT if instance == 1 else np.eye(3)
    built, floors = es.build(pta, models, np.zeros(3), 3.0, R, 1.0, SHIFT if instance == 2 else (0, 0, 0))
    return built, floors, info


def speck_view(pta, built, rec, pixels_across=24, height=64):
    """A camera at the scene's eye that looks at speck `rec` with a field of view in which it is `pixels_across` of `height` pixels
    tall (scene_builder.make_camera with a narrow fov)."""
    import scene_builder as sb
    P = es.primitives(built)
    t = built.desc.contents.camera.transform
    eye = np.array([t[12], t[13], t[14]], np.float64)
    c, r = P["centre"][rec["prim"]].astype(np.float64), float(P["radius"][rec["prim"]])
    D = float(np.linalg.norm(c - eye))
    fov = 2.0 * np.arctan((r / D) * height / pixels_across)
    return sb.make_camera(pta, eye=eye, target=c, fov=float(fov))


def directed(pta, r=1e-3, gap=2e-4):
    """The directed scene: a 0.4 x 0.4 wall that faces the camera on the view axis and one sphere of radius r around the point the
    camera looks at (3.096 away), the wall `gap` in front of the sphere's nearest point.  (BuiltScene, the speck's record)."""
    a, u, w = _frame()
    c = -a * (r + gap)
    s = 0.2
    q = [c - s * u - s * w, c + s * u - s * w, c + s * u + s * w, c - s * u + s * w]
    built, _ = es.build(pta, [es.mesh([[q[0], q[1], q[2]], [q[0], q[2], q[3]]], floor="wall"), es.sphere((0, 0, 0), r)], np.zeros(3), 3.0)
    return built, dict(where="directed", prim=2, r=r, place=gap, k=1.0)
