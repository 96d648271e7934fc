"""The temporal history's model (tests/history_model.py) on synthetic frames: the literal properties of the reprojection
(include/ptgpu.h pt_history_advance).  No GPU: the GPU tests hold the kernel to this model bit for bit."""
import re

import numpy as np
import pytest

import history_model as hm
from conftest import ROOT

f32 = np.float32
N = 4
PARAMS = hm.DEFAULTS


def frame(camera, w, h, planes, seed):
    aov = hm.plane_records(camera, w, h, N, planes)
    a, m = hm.noise_planes(w * h, N, seed)
    return a, m, aov


def step(prev, cam_prev, cam_new, w, h, planes, seed, params=PARAMS):
    a, m, aov = frame(cam_new, w, h, planes, seed)
    vp = hm.view_constants(cam_prev, w, h) if cam_prev is not None else None
    return hm.advance(prev, vp, hm.view_constants(cam_new, w, h), N, a, m, aov, params, w, h), (a, m, aov)


WALL = [((0.0, 0.0, -4.0), (0.0, 0.0, 1.0), None)]
FRONT = hm.look_at((0.0, 0.0, 0.0), (0.0, 0.0, -1.0), fov=0.9)


def shifted(k, w, h, depth=4.0):
    """FRONT moved sideways by exactly k pixel footprints on the plane at `depth`."""
    V = hm.view_constants(FRONT, w, h)
    return hm.look_at((k * 2.0 * float(V.tx) * depth / w, 0.0, 0.0), (k * 2.0 * float(V.tx) * depth / w, 0.0, -1.0), fov=0.9)


def test_the_defaults_are_the_headers():
    text = (ROOT / "include" / "ptgpu.h").read_text()
    got = {k: re.search(rf"#define PT_HISTORY_DEFAULT_{k}\s+([0-9.]+)", text).group(1) for k in ("NORMAL_COS", "PLANE_TOL", "MAX_SAMPLES", "ROTATE")}
    assert (float(got["NORMAL_COS"]), float(got["PLANE_TOL"]), int(got["MAX_SAMPLES"]), int(got["ROTATE"])) == tuple(hm.DEFAULTS)


def test_view_constants_invert_a_rigid_camera():
    cam = hm.look_at((0.137, 1.371, 2.613), (0.02, 0.61, -0.52), fov=0.93)
    V = hm.view_constants(cam, 24, 16)
    t, _ = hm.camera_fields(cam)
    A = np.array([[t[4 * k + r] for k in range(3)] for r in range(3)], float)
    assert np.abs(V.M.astype(float) @ A - np.eye(3)).max() <= 1e-6
    assert V.tx == f32(V.ty * f32(f32(24) / f32(16))) and (V.c3 == t[12:15]).all()
    with pytest.raises(ValueError):
        hm.view_constants({"transform": [[1, 0, 0, 0], [2, 0, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]], "fov": 1.0}, 4, 4)


@pytest.mark.parametrize("size", [(1, 1), (3, 2), (64, 4), (37, 23)])
def test_the_same_camera_twice_maps_every_surface_pixel_to_itself(size):
    w, h = size
    planes = WALL + [((0.0, -1.0, 0.0), (0.0, 1.0, 0.0), lambda P: P[:, 2] > -3.0)]
    first, (a0, m0, _) = step(None, None, FRONT, w, h, planes, 1)
    assert (first["count"] == N).all() and (first["accum"].view(np.uint32) == a0.view(np.uint32)).all()
    assert (first["map"][first["surf"][:, 3] >= 0] == -3).all()           # an empty history: test 1
    second, (a1, m1, _) = step(first, FRONT, FRONT, w, h, planes, 2)
    surface = second["surf"][:, 3] >= 0
    assert surface.any() and (second["map"][surface] == np.arange(w * h)[surface]).all()
    assert (second["map"][~surface] == -1).all()
    assert (second["count"] == np.where(surface, 2 * N, N)).all()
    assert (second["accum"][surface] == (a0 + a1).astype(f32)[surface]).all() and (second["accum"][~surface] == a1[~surface]).all()
    assert (second["moments"][surface] == (m0 + m1).astype(f32)[surface]).all()


@pytest.mark.parametrize("k", [1, 3])
def test_a_sideways_shift_by_whole_pixels_shifts_the_map(k):
    w, h = 16, 8
    first, _ = step(None, None, FRONT, w, h, WALL, 1)
    second, _ = step(first, FRONT, shifted(k, w, h), w, h, WALL, 2)
    hmap = second["map"].reshape(h, w)
    xs, ys = np.meshgrid(np.arange(w), np.arange(h))
    assert (hmap[:, :w - k] == (xs + k + ys * w)[:, :w - k]).all()
    assert (hmap[:, w - k:] == hm.OUTSIDE).all()
    assert (second["count"].reshape(h, w)[:, w - k:] == N).all() and (second["count"].reshape(h, w)[:, :w - k] == 2 * N).all()


def test_revealed_wall_pixels_never_take_the_strips_history():
    w, h = 48, 6
    strip = ((0.0, 0.0, -1.5), (0.0, 0.0, 1.0), lambda P: np.abs(P[:, 0]) < 0.25)
    planes = [strip] + WALL
    first, _ = step(None, None, FRONT, w, h, planes, 1)
    moved = hm.look_at((0.3, 0.0, 0.0), (0.3, 0.0, -1.0), fov=0.9)
    second, _ = step(first, FRONT, moved, w, h, planes, 2)
    prim_new = second["surf"][:, 7].view(np.int32)
    prim_old = first["surf"][:, 7].view(np.int32)
    hmap = second["map"]
    got = hmap >= 0
    assert (prim_old[hmap[got]] == prim_new[got]).all()
    # the wall pixels whose primary tap lands on the strip: test 4 (the normals agree), and some of them exist
    V = hm.view_constants(FRONT, w, h)
    P = second["surf"][:, 0:3].astype(float)
    fx = (P[:, 0] / -P[:, 2] / float(V.tx) + 1.0) * 0.5 * w
    fy = (1.0 - P[:, 1] / -P[:, 2] / float(V.ty)) * 0.5 * h
    inside = (fx >= 0) & (fx < w) & (fy >= 0) & (fy < h)
    primary = np.where(inside, np.floor(fx) + np.floor(fy) * w, 0).astype(int)
    revealed = inside & (prim_new == 1) & (prim_old[primary] == 0)
    assert revealed.sum() >= h
    assert ((hmap[revealed] == -6) | ((hmap[revealed] >= 0) & (prim_old[np.where(hmap >= 0, hmap, 0)][revealed] == 1))).all()
    # ... and the strip's own pixels find the strip
    assert (hmap[prim_new == 0] >= 0).mean() > 0.5


def test_the_cap_scales_the_sums_and_bounds_the_counts():
    w, h = 16, 8
    params = PARAMS._replace(max_samples=6)
    hist, cam = None, None
    sums = []
    for k in range(4):
        hist, (a, m, _) = step(hist, cam, FRONT, w, h, WALL, 10 + k, params)
        cam = FRONT
        sums.append((a, m))
    # counts before each frame: 0, 4, 8 -> 6, 10 -> 6
    assert (hist["count"] == 6 + N).all()
    a2 = (sums[0][0] + sums[1][0]).astype(f32)
    f8 = f32(f32(6) / f32(8))
    a3 = ((a2 * f8).astype(f32) + sums[2][0]).astype(f32)
    f10 = f32(f32(6) / f32(10))
    a4 = ((a3 * f10).astype(f32) + sums[3][0]).astype(f32)
    assert (hist["accum"].view(np.uint32) == a4.view(np.uint32)).all()
    m2 = (sums[0][1] + sums[1][1]).astype(f32)
    m4 = (((((m2 * f8).astype(f32) + sums[2][1]).astype(f32)) * f10).astype(f32) + sums[3][1]).astype(f32)
    assert (hist["moments"].view(np.uint32) == m4.view(np.uint32)).all()


def test_points_behind_the_camera_and_wild_positions_are_outside():
    w, h = 8, 4
    first, _ = step(None, None, FRONT, w, h, WALL, 1)
    back = hm.look_at((0.0, 0.0, -8.0), (0.0, 0.0, -9.0), fov=0.9)        # the wall is behind this camera
    second, _ = step(first, back, FRONT, w, h, WALL, 2)
    assert (second["map"] == hm.OUTSIDE).all() and (second["count"] == N).all()
    a, m, aov = frame(FRONT, w, h, WALL, 3)
    wild = [(np.inf, 0.0, -1.0), (0.0, -np.inf, -1.0), (np.nan, 0.0, -1.0), (0.0, 0.0, np.nan), (1e30, 0.0, -1.0), (0.0, -1e30, -1.0),
            (np.inf, np.inf, -np.inf), (3e38, 3e38, -1e-30)]
    with np.errstate(over="ignore"):
        for k, p in enumerate(wild):
            aov[k, 8:11] = np.array(p, f32) * f32(N)
    V = hm.view_constants(FRONT, w, h)
    third = hm.advance(first, V, V, N, a, m, aov, PARAMS, w, h)
    assert (third["map"][:len(wild)] == hm.OUTSIDE).all()
    assert (third["map"][len(wild):] == np.arange(len(wild), w * h)).all()


@pytest.mark.parametrize("corner", [(0, 0), (1, 0), (0, 1), (1, 1)])
def test_a_primary_tap_in_a_corner_skips_the_taps_outside_the_image(corner):
    """The camera is turned so little that every primary tap is the pixel itself while the footprint's other taps of the corner
    pixel lie outside the image; the previous view's corner pixel holds no samples, so the fallbacks are asked for."""
    w, h = 3, 2
    cx, cy = corner[0] * (w - 1), corner[1] * (h - 1)
    first, _ = step(None, None, FRONT, w, h, WALL, 1)
    first["count"][cx + cy * w] = 0
    eps = 0.02 * (1 if corner[0] else -1), 0.02 * (1 if corner[1] else -1)     # the taps move towards the corner
    moved = hm.look_at((0.0, 0.0, 0.0), (eps[0], -eps[1], -1.0), fov=0.9)
    second, _ = step(first, FRONT, moved, w, h, WALL, 2)
    hmap = second["map"]
    assert hmap[cx + cy * w] == -3 and second["count"][cx + cy * w] == N
    others = np.arange(w * h) != cx + cy * w
    assert (hmap[others] >= 0).all()


def test_the_orbit_of_the_end_to_end_case_reprojects_half_of_the_surface_pixels(pta, oracle):
    """The frames of tests/test_history_gpu.py's end-to-end case from the CPU models: the oracle's samples and
    aov_model.records_f32's records.  From the second frame on at least half of the surface pixels find a source."""
    import aov_model as am
    import shading_model as sm
    w, h = hm.E2E_SIZE
    n = w * h
    hist, vprev = None, None
    for k in range(3):
        scene, camera, prof = hm.e2e_scene(pta, k)
        osc = oracle.OracleScene(scene.desc, oracle.PTO_BRUTE_FORCE, keepalive=scene)
        model = sm.ShadingModel(scene.desc, osc, oracle, max_hits=am.MAX_HITS)
        aov = am.reduce_records(am.records_f32(model, am.records_f64(model, prof)))
        _, acc, _ = osc.render(prof)
        lum = (f32(0.2126) * acc[:, 0] + f32(0.7152) * acc[:, 1]).astype(f32) + f32(0.0722) * acc[:, 2]
        mom = np.stack([lum, (lum * lum / f32(hm.E2E_SAMPLES)).astype(f32)], axis=1).astype(f32)   # (stand-in sums: the share ignores them)
        V = hm.view_constants(camera, w, h)
        hist = hm.advance(hist, vprev, V, hm.E2E_SAMPLES, acc.reshape(n, 3), mom, aov, hm.DEFAULTS, w, h)
        vprev = V
        if k:
            assert (hist["surf"][:, 3] >= 0).sum() > n // 4
            assert hm.share(hist["map"], hist["surf"]) >= 0.5, (k, hm.share(hist["map"], hist["surf"]))
