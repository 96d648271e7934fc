"""pt_scene_set_camera: a scene whose camera was replaced renders exactly what a scene created with that camera renders -
images, accumulators, grids, escape masks, debug planes, shards - and no state of an earlier camera survives (frame plans,
the cull table, the camera grid)."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
SCENES = ROOT / "tests" / "golden" / "scenes"
EXE = ROOT / "path-tracer_amd" / "path-tracer"
sys.path.insert(0, str(ROOT / "tools"))
import make_orbit  # noqa: E402
sys.path.pop(0)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def load(pta, name):
    if name == "ps5":
        return pta.HostScene.generate_ps5(30000, seed=1, flags=8)
    return pta.HostScene.load_isf(SCENES / name / "scene.isf")


def cameras(pta, scene):
    """An orbit step, a camera inside the scene box, one 4x farther out (delta_in grows) and one whose transform is scaled so
    that fro >= 64 (a fresh scene has no camera grid)."""
    base = scene.camera
    pivot = make_orbit.scene_box_centre(scene)
    orbit = pta.make_camera(make_orbit.orbit(scene, 8)[1])
    t = np.array(list(base.transform), np.float64)
    inside = t.copy()
    inside[12:15] = pivot
    far = t.copy()
    far[12:15] = pivot + 4.0 * (t[12:15] - pivot)
    scaled = t.copy()
    scaled[0:12] *= 40.0
    assert np.sqrt((scaled[[0, 1, 2, 4, 5, 6, 8, 9, 10]] ** 2).sum()) >= 64
    mk = lambda v: pta.Camera((pta.C.c_float * 16)(*[float(x) for x in np.float32(v)]), base.fov, base.zfar, base.znear)
    return {"orbit": orbit, "inside": mk(inside), "far": mk(far), "scaled": mk(scaled)}


def fresh(pta, name, cam, **kw):
    h = load(pta, name)
    h.set_camera(cam)
    return h, pta.GpuScene(h, **kw)


def same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1]))


@pytest.mark.parametrize("name", ["cube", "head", "spheres", "alpha_transparency", "white_furnace_direct", "ps5"])
def test_set_camera_equals_a_fresh_scene(pta, name):
    prof = pta.Profile.make(160, 120, 4, 0 if name == "white_furnace_direct" else 3)
    flag_sets = (0, pta.PT_FLAG_NO_GRIDS, pta.PT_FLAG_MEGAKERNEL)
    host = load(pta, name)
    g = pta.GpuScene(host)
    for f in flag_sets:   # (frames of the first camera: plans, masks, the cull table exist when the camera moves)
        g.render(prof, pta.Opts.make(flags=f))
    g.render(prof)
    for label, cam in cameras(pta, host).items():
        _, ref = fresh(pta, name, cam)
        g.set_camera(cam)
        assert g.info().cam_grid_res == ref.info().cam_grid_res, label
        if label == "scaled":
            assert ref.info().cam_grid_res == 0
        for f in flag_sets:
            got, want = g.render(prof, pta.Opts.make(flags=f)), ref.render(prof, pta.Opts.make(flags=f))
            assert same(got, want), (name, label, f)
        ref.close()


def test_no_stale_frame_plan(pta):
    prof = pta.Profile.make(160, 120, 4, 4)
    host = load(pta, "ps5")
    cams = cameras(pta, host)
    cam_a, cam_b = cams["far"], host.camera     # far out: the object is small, most camera rays miss
    _, ref_a = fresh(pta, "ps5", cam_a)
    _, ref_b = fresh(pta, "ps5", cam_b)
    segs = []
    for r in (ref_a, ref_b):
        r.render(prof, pta.Opts.make(flags=pta.PT_FLAG_COUNTERS))
        segs.append(r.counters().segments)
    assert segs[1] > segs[0], segs   # (what makes a plan of A overflow on B)
    want_a, want_b = ref_a.render(prof), ref_b.render(prof)
    g = pta.GpuScene(host)
    g.set_camera(cam_a)
    first_a = g.render(prof)
    assert same(first_a, want_a)
    assert same(g.render(prof), want_a) and g.info().frame_planned == 1
    g.set_camera(cam_b)
    assert same(g.render(prof), want_b) and g.info().frame_planned == 0
    assert same(g.render(prof), want_b) and g.info().frame_planned == 1
    g.set_camera(cam_a)
    assert same(g.render(prof), first_a)


def test_frame_in_flight_finishes_with_the_old_camera(pta):
    import torch
    prof = pta.Profile.make(160, 120, 8, 4)
    host = load(pta, "head")
    cam_a, cam_b = host.camera, cameras(pta, host)["orbit"]
    _, ref_b = fresh(pta, "head", cam_b)
    want_a, want_b = pta.GpuScene(host).render(prof), ref_b.render(prof)
    g = pta.GpuScene(host)
    n = 160 * 120
    outs = [(torch.empty(n * 3, dtype=torch.uint8, device="cuda"), torch.empty(n * 3, dtype=torch.float32, device="cuda")) for _ in range(2)]
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        g.render_device(prof, pta.Opts.make(), outs[0][0].data_ptr(), outs[0][1].data_ptr(), stream.cuda_stream)
        g.set_camera(cam_b)   # (no synchronisation by the caller)
        g.render_device(prof, pta.Opts.make(), outs[1][0].data_ptr(), outs[1][1].data_ptr(), stream.cuda_stream)
    stream.synchronize()
    for (rgb, acc), want in zip(outs, (want_a, want_b)):
        assert same((rgb.cpu().numpy().reshape(-1, 3), acc.cpu().numpy().reshape(-1, 3)), want)


def grid_arrays(grid):
    return (int(grid.c.res), int(grid.c.n_cells), int(grid.c.n_refs), int(grid.c.n_global), int(grid.c.enabled),
            int(grid.c.max_cell_refs), bits(np.array(list(grid.c.origin), np.float32)).tolist(), float(grid.c.ray_offset),
            int(grid.c.kind)), (grid.cell_off if grid.enabled else None), (grid.ref_prim if grid.enabled else None), \
        (bits(grid.ref_mindist) if grid.enabled else None)


def grid_bytes(grid):
    return (int(grid.c.n_cells) + 2) * 4 + 8 * max(1, grid.n_refs) if grid.enabled else 0


def assert_grids_equal(a, b, what):
    ha, *xa = grid_arrays(a)
    hb, *xb = grid_arrays(b)
    assert ha == hb, what
    for u, v in zip(xa, xb):
        assert (u is None and v is None) or np.array_equal(u, v), what


@pytest.mark.parametrize("name", ["head", "ps5"])
def test_camera_grid_equals_a_fresh_scene_and_the_host_builder(pta, name):
    host = load(pta, name)
    g = pta.GpuScene(host)
    lights_before = [pta.OriginGrid.from_device(g, 1 + i) for i in range(host.n_lights)]
    for label, cam in cameras(pta, host).items():
        h2, ref = fresh(pta, name, cam)
        before, old = g.info().device_bytes, pta.OriginGrid.from_device(g, 0)
        g.set_camera(cam)
        got, want = pta.OriginGrid.from_device(g, 0), pta.OriginGrid.from_device(ref, 0)
        assert_grids_equal(got, want, (name, label))
        # (device_bytes: only the camera grid's arrays change - the KD entry lists of a fresh scene may differ in length, their
        # eps takes the camera position into account, but they are not load-bearing: the images above are the same bits)
        assert g.info().grid_refs == ref.info().grid_refs, label
        assert g.info().device_bytes - before == grid_bytes(got) - grid_bytes(old), label
        if want.enabled:
            t = list(cam.transform)
            fro = float(np.sqrt(sum(float(t[4 * k + r]) ** 2 for k in range(3) for r in range(3))))
            hg = pta.OriginGrid(h2, origin=t[12:15], res=want.res, ray_offset=0.0, max_dir_len=np.float32(fro * 1.001))
            assert_grids_equal(got, hg, (name, label, "host"))
        for i, lb in enumerate(lights_before):
            assert_grids_equal(pta.OriginGrid.from_device(g, 1 + i), lb, (name, label, "light", i))
        ref.close()


def test_escape_masks_follow_the_camera(pta):
    from test_escape_masks import H_HI, H_LO, rays_through_clear_cells
    host = load(pta, "head")
    cams = cameras(pta, host)
    g = pta.GpuScene(host)
    m0 = g.escape_masks()
    # moving out: delta_in grows, the masks go and the schedule builds them again - as a fresh scene does
    g.set_camera(cams["far"])
    assert g.info().escape_prims == 0
    h_far, ref = fresh(pta, "head", cams["far"])
    m_far, m_ref = g.escape_masks(), ref.escape_masks()
    for u, v in zip(m_far, m_ref):
        assert np.array_equal(np.asarray(u).view(np.uint8), np.asarray(v).view(np.uint8))
    # moving in: the masks of the larger delta_in stay
    g.set_camera(cams["inside"])
    m_in = g.escape_masks()
    for u, v in zip(m_in, m_far):
        assert np.array_equal(np.asarray(u).view(np.uint8), np.asarray(v).view(np.uint8))
    assert g.info().escape_prims > 0 and m0 is not None
    for masks, seed in ((m_far, 3), (m_in, 4)):
        rays, prims = rays_through_clear_cells(host, masks, 20000, seed=seed)
        assert rays is not None
        h = ((rays[:, :3] - masks[1][prims]) * masks[0][prims]).sum(axis=1)
        ok = (h >= H_LO) & (h <= H_HI)
        _, counts = g.trace_all(rays[ok], 2)
        assert counts.sum() == 0


def test_moved_camera_matches_the_oracle(pta, oracle):
    prof = pta.Profile.make(160, 120, 4, 3)
    host = load(pta, "head")
    cam = cameras(pta, host)["orbit"]
    g = pta.GpuScene(host)
    g.render(prof)
    g.set_camera(cam)
    rgb, acc = g.render(prof)
    h2 = load(pta, "head")
    h2.set_camera(cam)
    o = oracle.OracleScene(h2.desc, oracle.PTO_BRUTE_FORCE)
    for row in (40, 77):
        o_rgb, o_acc, _ = o.render(prof, row * 160, (row + 1) * 160)
        assert np.array_equal(rgb[row * 160:(row + 1) * 160], o_rgb)
        assert np.array_equal(bits(acc[row * 160:(row + 1) * 160]), bits(o_acc))


def test_debug_render_shards_and_prep_after_a_move(pta):
    prof = pta.Profile.make(160, 120, 4, 3)
    host = load(pta, "alpha_transparency")
    cam = cameras(pta, host)["orbit"]
    _, ref = fresh(pta, "alpha_transparency", cam)
    want = ref.render(prof)
    g = pta.GpuScene(host)
    g.render(prof)
    g.set_camera(cam)
    d_got, d_want = g.debug_render(160, 120), ref.debug_render(160, 120)
    assert d_got.keys() == d_want.keys() and all(np.array_equal(d_got[k], d_want[k]) for k in d_want)
    rgb = np.zeros((160 * 120, 3), np.uint8)
    acc = np.zeros((160 * 120, 3), np.float32)
    for r in range(3):
        o = pta.Opts.make(shard_rank=r, shard_count=3, tile_w=32, tile_h=32)
        pr, pa = g.render(prof, o)
        m = pta.local_pixel_map(prof, o)
        rgb[m], acc[m] = pr, pa
    assert same((rgb, acc), want)
    prep = pta.Prep(host)
    scenes = [pta.GpuScene(host, prep=prep) for _ in range(2)]
    prep.close()
    for s in scenes:
        s.set_camera(cam)
        assert same(s.render(prof), want)


def test_set_camera_none_is_invalid_and_changes_nothing(pta):
    prof = pta.Profile.make(160, 120, 4, 3)
    g = pta.GpuScene(load(pta, "cube"))
    want = g.render(prof)
    with pytest.raises(pta.PtError) as e:
        g.set_camera(None)
    assert e.value.code == -1
    assert same(g.render(prof), want)


def test_cli_camera_path(pta, tmp_path):
    from PIL import Image
    scene_path = SCENES / "spheres" / "scene.isf"
    cams = tmp_path / "orbit.json"
    r = subprocess.run([sys.executable, str(ROOT / "tools" / "make_orbit.py"), str(scene_path), "3", "-o", str(cams)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    prof = tmp_path / "p.yml"
    prof.write_text("resolution:\n  width: 96\n  height: 64\nsamples: 4\nbounces: 2\n")
    host = pta.HostScene.load_isf(scene_path)
    g = pta.GpuScene(host)
    want = []
    for cam in pta.load_camera_path(cams):
        g.set_camera(cam)
        want.append(g.render(pta.Profile.make(96, 64, 4, 2))[0])
    for sub, extra in (("one", []), ("two", ["--devices", "0,0"])):
        out = tmp_path / sub
        out.mkdir()
        r = subprocess.run([str(EXE), "render", str(scene_path), "-q", "-p", str(prof), "--camera-path", str(cams),
                            "-o", str(out / "frame_%04d.png"), *extra], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        assert sorted(p.name for p in out.iterdir()) == [f"frame_{i:04d}.png" for i in range(3)]
        for i in range(3):
            assert np.array_equal(np.asarray(Image.open(out / f"frame_{i:04d}.png")).reshape(-1, 3), want[i]), (sub, i)
    assert not np.array_equal(want[0], want[1])
