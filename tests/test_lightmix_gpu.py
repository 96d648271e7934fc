"""The light mixer on the GPU: k_lightmix_apply against tests/lightmix_model.py bit for bit, the captured planes against the
accumulators of a second scene edited with set_lights, what a capture leaves behind in its scene, a mix against a real render
of the edited lights, and `render --keyframes --light-mixer`."""
import ctypes as C
import json
import subprocess

import numpy as np
import pytest

import lightmix_model as lm
from conftest import ROOT, SCENES

pytestmark = pytest.mark.gpu

f32 = np.float32
EXE = ROOT / "path-tracer_amd" / "path-tracer"
W, H, SAMPLES, BOUNCES = 70, 50, 4, 3   # 9 x 2 tiles of 8 x 32; neither side a multiple of a tile
PT_FLAG_NO_GRIDS = 4


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def same_bits(a, b):
    return bool(((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))).all())


def with_colors(lights, colors):
    out = []
    for l, c in zip(lights, np.asarray(colors, f32).reshape(-1, 3)):
        k = type(l).from_buffer_copy(l)
        k.color[0], k.color[1], k.color[2] = float(c[0]), float(c[1]), float(c[2])
        out.append(k)
    return out


def light_colors(lights):
    return np.array([[l.color[0], l.color[1], l.color[2]] for l in lights], f32).reshape(-1, 3)


def point_light(pta, vec, color):
    return pta.Light(pta.PT_LIGHT_POINT, (C.c_float * 3)(*[float(v) for v in vec]), (C.c_float * 3)(*[float(v) for v in color]), 0.1)


def load(pta, name):
    """(host scene, its lights) of the capture cases: golden scenes, `cube` given 6 lights, a scene set to 0 lights."""
    host = pta.HostScene.load_isf(SCENES / name.split("+")[0] / "scene.isf")
    if name == "cube+6":
        p = np.array(list(host.lights[0].vec), np.float64)
        offs = [(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (-1, 0.5, 0), (0.5, 0.5, -1)]
        cols = [(1000, 1000, 1000), (300, 0, 0), (0, 5, 0), (0.5, 0.25, 2), (0, 0, 0), (40, 80, 20)]   # (one black: unit 1)
        host.set_lights([point_light(pta, p + 0.5 * np.array(o), c) for o, c in zip(offs, cols)])
    elif name == "cube+0":
        host.set_lights([])
    return host, host.lights


# ------------------------------------------------------------------------------------------------ kernel against model
def device_apply(mix, colors, tm, n, want_rgb, want_acc):
    """pt_lightmix_apply_device on torch tensors with a guard tail behind each output: (rgb8, accum), either None."""
    import torch
    guard = 32
    d_rgb = torch.full((n * 3 + guard,), 0xA5, dtype=torch.uint8, device="cuda") if want_rgb else None
    d_acc = torch.full((n * 3 + guard,), -7.0, dtype=torch.float32, device="cuda") if want_acc else None
    mix.apply_device(colors, tm, d_rgb.data_ptr() if want_rgb else 0, d_acc.data_ptr() if want_acc else 0,
                     torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    rgb = acc = None
    if want_rgb:
        h = d_rgb.cpu().numpy()
        assert (h[n * 3:] == 0xA5).all(), "rgb8 written past the image"
        rgb = h[: n * 3].reshape(-1, 3)
    if want_acc:
        h = d_acc.cpu().numpy()
        assert (h[n * 3:] == f32(-7.0)).all(), "accum written past the image"
        acc = h[: n * 3].reshape(-1, 3)
    return rgb, acc


@pytest.mark.parametrize("n_local", (1, 2, 3, 35, 3072, 8710))
def test_apply_equals_the_model_bit_for_bit(pta, oracle, n_local):
    rng = np.random.default_rng(n_local)
    for n_lights in (0, 1, 3, 16):
        planes, unit, samples = lm.synthetic_planes(n_lights, n_local, 1000 * n_lights + n_local)
        mix = pta.LightMix.from_planes(planes, unit, samples)
        info = mix.info
        assert (info.n_lights, info.samples, info.n_local) == (n_lights, samples, n_local)
        assert np.array_equal(np.array(info.unit[:n_lights], f32), unit) and info.device_bytes >= planes.nbytes
        for i in range(n_lights + 1):
            assert same_bits(mix.basis(i), planes[i])
        colors = (rng.uniform(-0.5, 3.0, (n_lights, 3)) * unit[:, None]).astype(f32)
        if n_lights:
            colors[rng.integers(n_lights)] = 0   # a muted light
        want = lm.apply(planes, unit, colors)
        for tm in (0, 1, 2):
            want_rgb = oracle.post_process(pta.Profile.make(n_local, 1, samples, 1, tm), want)
            rgb, acc = mix.apply(colors, tm, want_accum=True)
            assert same_bits(acc, want), ("host", n_local, n_lights, tm)
            assert np.array_equal(rgb, want_rgb), ("host", n_local, n_lights, tm)
            assert np.array_equal(mix.apply(colors, tm), want_rgb), ("host rgb8 only", n_local, n_lights, tm)
            only = np.empty((n_local, 3), f32)
            pta.check_gpu(mix.lib.pt_lightmix_apply(mix.handle, colors.ctypes.data, tm, None, only.ctypes.data))
            assert same_bits(only, want), ("host accum only", n_local, n_lights, tm)
            for want_r, want_a in ((True, True), (True, False), (False, True)):
                rgb, acc = device_apply(mix, colors, tm, n_local, want_r, want_a)
                assert rgb is None or np.array_equal(rgb, want_rgb), ("device", n_local, n_lights, tm, want_r, want_a)
                assert acc is None or same_bits(acc, want), ("device", n_local, n_lights, tm, want_r, want_a)
        mix.close()


def test_apply_and_create_refuse_bad_arguments(pta):
    import torch
    planes, unit, samples = lm.synthetic_planes(2, 35, 5)
    mix = pta.LightMix.from_planes(planes, unit, samples)
    lib, INVALID = mix.lib, pta.PT_ERR_INVALID
    colors = np.ones((2, 3), f32)
    rgb, acc = np.empty((35, 3), np.uint8), np.empty((35, 3), f32)
    d_rgb = torch.empty(35 * 3 + 8, dtype=torch.uint8, device="cuda")
    d_acc = torch.empty(35 * 3 + 8, dtype=torch.float32, device="cuda")
    assert lib.pt_lightmix_apply(None, colors.ctypes.data, 1, rgb.ctypes.data, acc.ctypes.data) == INVALID
    assert lib.pt_lightmix_apply(mix.handle, None, 1, rgb.ctypes.data, acc.ctypes.data) == INVALID
    assert lib.pt_lightmix_apply(mix.handle, colors.ctypes.data, 1, None, None) == INVALID
    for tm in (-1, 3):
        assert lib.pt_lightmix_apply(mix.handle, colors.ctypes.data, tm, rgb.ctypes.data, None) == INVALID
        assert lib.pt_lightmix_apply_device(mix.handle, colors.ctypes.data, tm, d_rgb.data_ptr(), None, None) == INVALID
    for bad in (np.nan, np.inf, -np.inf):
        c = colors.copy()
        c[1, 2] = bad
        assert lib.pt_lightmix_apply(mix.handle, c.ctypes.data, 1, rgb.ctypes.data, acc.ctypes.data) == INVALID
        assert lib.pt_lightmix_apply_device(mix.handle, c.ctypes.data, 1, d_rgb.data_ptr(), d_acc.data_ptr(), None) == INVALID
    assert lib.pt_lightmix_apply_device(mix.handle, colors.ctypes.data, 1, d_rgb.data_ptr() + 1, None, None) == INVALID
    assert lib.pt_lightmix_apply_device(mix.handle, colors.ctypes.data, 1, None, d_acc.data_ptr() + 4, None) == INVALID
    assert lib.pt_lightmix_apply_device(None, colors.ctypes.data, 1, d_rgb.data_ptr(), None, None) == INVALID
    info = pta.LightMixInfo()
    assert lib.pt_lightmix_get_info(None, C.byref(info)) == INVALID and lib.pt_lightmix_get_info(mix.handle, None) == INVALID
    assert lib.pt_lightmix_basis(mix.handle, 3, acc.ctypes.data) == INVALID and lib.pt_lightmix_basis(mix.handle, 0, None) == INVALID
    out = C.c_void_p()
    create = lib.pt_lightmix_create_from_planes
    assert create(0, 2, samples, 35, unit.ctypes.data, None, C.byref(out)) == INVALID
    assert create(0, 2, samples, 35, None, planes.ctypes.data, C.byref(out)) == INVALID
    assert create(0, 2, samples, 35, unit.ctypes.data, planes.ctypes.data, None) == INVALID
    assert create(0, 2, 0, 35, unit.ctypes.data, planes.ctypes.data, C.byref(out)) == INVALID
    assert create(0, 2, samples, 0, unit.ctypes.data, planes.ctypes.data, C.byref(out)) == INVALID
    assert create(0, 2, samples, 35, np.array([1, 0], f32).ctypes.data, planes.ctypes.data, C.byref(out)) == INVALID
    assert create(0, 17, samples, 1, np.ones(17, f32).ctypes.data, np.zeros((18, 1, 3), f32).ctypes.data, C.byref(out)) == pta.PT_ERR_UNSUPPORTED
    assert not out.value
    lib.pt_lightmix_destroy(None)
    # the refusals left the object as it was
    assert same_bits(mix.apply(colors, 1, want_accum=True)[1], lm.apply(planes, unit, colors))


# ------------------------------------------------------------------------------------------------ capture
def conditions(pta):
    yield "unsharded", [pta.Opts.make()], 0
    yield "3 shards of 8x32 tiles", [pta.Opts.make(shard_rank=r, shard_count=3, tile_w=8, tile_h=32) for r in range(3)], 0
    yield "PT_FLAG_NO_GRIDS", [pta.Opts.make(flags=PT_FLAG_NO_GRIDS)], 0
    yield "planned scene with keyed caches", [pta.Opts.make()], 3


@pytest.mark.parametrize("name", ("cube", "head", "spheres", "cube+6", "cube+0"))
def test_capture_equals_frames_of_a_scene_edited_with_set_lights(pta, name):
    prof = pta.Profile.make(W, H, SAMPLES, BOUNCES)
    host, lights = load(pta, name)
    base = light_colors(lights)
    g, ref = pta.GpuScene(host), pta.GpuScene(host)
    for label, opts_list, warm in conditions(pta):
        for opts in opts_list:
            for _ in range(warm):   # the frames that plan the configuration and key and fill the scene's caches
                g.render(prof, opts)
            mix = g.lightmix_capture(prof, opts)
            info = mix.info
            n_local = int(pta.gpu_lib().pt_local_pixel_count(C.byref(prof), C.byref(opts)))
            assert (info.n_lights, info.samples, info.n_local) == (len(lights), SAMPLES, n_local), (name, label)
            assert np.array_equal(np.array(info.unit[:len(lights)], f32), lm.units(base)), (name, label)
            frames = []
            for i in range(len(lights) + 1):
                ref.set_lights(with_colors(lights, lm.basis_colors(base, i)))
                frames.append(ref.render(prof, opts)[1])
            want = lm.capture(np.stack(frames))
            for i in range(len(lights) + 1):
                assert same_bits(mix.basis(i), want[i]), (name, label, opts.shard_rank, i)
            if len(lights):
                assert np.abs(want[1:]).max() > 0, (name, label)   # (the lights do reach the image)
            mix.close()


def test_capture_leaves_the_scene_as_it_was(pta):
    import torch
    prof = pta.Profile.make(W, H, SAMPLES, BOUNCES)
    host, lights = load(pta, "spheres")
    g = pta.GpuScene(host)
    for warm in (0, 3):   # a fresh scene, then one with a frame plan and keyed caches
        for _ in range(warm):
            g.render(prof)
        before = g.render(prof)
        mix = g.lightmix_capture(prof)
        mix.close()
        after = g.render(prof)
        assert np.array_equal(before[0], after[0]) and same_bits(before[1], after[1]), warm
    fresh = pta.GpuScene(host)
    want = fresh.render(prof)
    assert np.array_equal(before[0], want[0]) and same_bits(before[1], want[1])
    torch.cuda.synchronize()   # no HIP error is pending on the device the scene renders on
    assert torch.cuda.is_available() and float(torch.ones(4, device="cuda").sum().item()) == 4.0
    # the object outlives its scene
    mix = g.lightmix_capture(prof)
    colors = light_colors(lights)
    first = mix.apply(colors, want_accum=True)
    g.close()
    again = mix.apply(colors, want_accum=True)
    assert np.array_equal(first[0], again[0]) and same_bits(first[1], again[1])
    mix.close()


def test_capture_failures_return_no_object_and_change_nothing(pta):
    prof = pta.Profile.make(W, H, SAMPLES, BOUNCES)
    host, lights = load(pta, "cube")
    p = np.array(list(lights[0].vec), np.float64)
    host.set_lights([point_light(pta, p + 0.05 * np.array([k % 3, k % 5, k % 7]), (10, 20, 30)) for k in range(17)])
    g = pta.GpuScene(host)
    lib = g.lib
    before = g.render(prof)
    out = C.c_void_p()
    assert lib.pt_lightmix_capture(g.handle, C.byref(prof), None, C.byref(out)) == pta.PT_ERR_UNSUPPORTED
    assert not out.value
    assert lib.pt_lightmix_capture(None, C.byref(prof), None, C.byref(out)) == pta.PT_ERR_INVALID
    assert lib.pt_lightmix_capture(g.handle, None, None, C.byref(out)) == pta.PT_ERR_INVALID
    assert lib.pt_lightmix_capture(g.handle, C.byref(prof), None, None) == pta.PT_ERR_INVALID
    assert lib.pt_lightmix_capture(g.handle, C.byref(pta.Profile.make(W, H, 0, BOUNCES)), None, C.byref(out)) == pta.PT_ERR_INVALID
    bad = pta.Opts.make(shard_rank=3, shard_count=3)
    assert lib.pt_lightmix_capture(g.handle, C.byref(prof), C.byref(bad), C.byref(out)) == pta.PT_ERR_INVALID
    assert not out.value
    after = g.render(prof)
    assert np.array_equal(before[0], after[0]) and same_bits(before[1], after[1])
    # 16 lights are taken
    g.set_lights(host.lights[:16])
    mix = g.lightmix_capture(prof)
    assert mix.info.n_lights == 16
    mix.close()


# ------------------------------------------------------------------------------------------------ against a real render
@pytest.mark.parametrize("name", ("cube", "head", "spheres"))
def test_mix_against_a_render_of_the_edited_lights(pta, name):
    prof = pta.Profile.make(W, H, SAMPLES, BOUNCES)
    host, lights = load(pta, name)
    base = light_colors(lights)
    g = pta.GpuScene(host)
    mix = g.lightmix_capture(prof)
    rng = np.random.default_rng(len(name))
    solo = np.zeros_like(base)
    solo[-1] = base[-1]
    sets = {"same": base, "random a": lm.random_colors(rng, base), "random b": lm.random_colors(rng, base),
            "mute": lm.random_colors(rng, base, mute=0), "solo": solo, "black": np.zeros_like(base)}
    for label, colors in sets.items():
        host.set_lights(with_colors(lights, colors))
        fresh = pta.GpuScene(host)
        ref_rgb, ref = fresh.render(prof)
        fresh.close()
        rgb, acc = mix.apply(colors, want_accum=True)
        ratio = float((np.abs(acc.astype(np.float64) - ref) / (1e-4 * SAMPLES + 1e-3 * np.abs(ref))).max())
        lsb = int(np.abs(rgb.astype(int) - ref_rgb.astype(int)).max())
        print(f"{name} {label}: {ratio:.3e} of the tolerance, {lsb} LSB")
        assert ratio <= 1.0 and lsb <= 1, (name, label, ratio, lsb)
    mix.close()


# ------------------------------------------------------------------------------------------------ CLI
def test_cli_light_mixer(pta, tmp_path):
    from PIL import Image
    scene_path = SCENES / "head" / "scene.isf"
    cam = json.loads(scene_path.read_text())["camera"]
    cam["transform"][3][0] += 0.3

    def lights(p, c0, c1):
        return [{"type": "Point", "position": p, "color": c0, "size": 0.1},
                {"type": "Directional", "direction": [0.2, -1.0, -0.3], "color": c1}]
    frames = [{"lights": lights([2.0, 3.0, 2.5], [30.0, 25.0, 20.0], [1.5, 1.5, 1.5])},      # lights moved
              {"lights": lights([2.0, 3.0, 2.5], [10.0, 40.0, 5.0], [0.5, 1.0, 2.5])},       # colour
              {"lights": lights([2.0, 3.0, 2.5], [0.0, 0.0, 0.0], [3.0, 2.0, 1.0])},         # colour (the point light muted)
              {"camera": cam},
              {"lights": lights([2.0, 3.0, 2.5], [60.0, 20.0, 20.0], [0.2, 0.2, 0.9])}]      # colour
    path = tmp_path / "frames.json"
    path.write_text(json.dumps(frames))
    prof = tmp_path / "p.yml"
    prof.write_text("resolution:\n  width: 64\n  height: 48\nsamples: 4\nbounces: 2\n")
    images = {}
    for sub, extra in (("plain", []), ("mixer", ["--light-mixer"])):
        out = tmp_path / sub
        out.mkdir()
        r = subprocess.run([str(EXE), "render", str(scene_path), "-q", "-p", str(prof), "--keyframes", str(path),
                            "-o", str(out / "frame_%02d.png"), *extra], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        assert ("light mixer:" in r.stderr) == bool(extra)
        if extra:
            assert r.stderr.strip().splitlines()[-1] == "light mixer: 2 captures, 5 mixed frames, 0 rendered frames", r.stderr
        images[sub] = [np.asarray(Image.open(out / f"frame_{i:02d}.png")).astype(int) for i in range(5)]
    for i in range(5):
        assert np.abs(images["plain"][i] - images["mixer"][i]).max() <= 1, i
    assert not np.array_equal(images["plain"][1], images["plain"][2])
    cams = tmp_path / "cams.json"
    cams.write_text(json.dumps([cam]))
    misuse = {"no keyframes": ["--camera-path", str(cams), "--light-mixer"],
              "denoise": ["--keyframes", str(path), "--light-mixer", "--denoise"],
              "two devices": ["--keyframes", str(path), "--light-mixer", "--devices", "0,0"]}
    for sub, args in misuse.items():
        out = tmp_path / sub.replace(" ", "_")
        out.mkdir()
        r = subprocess.run([str(EXE), "render", str(scene_path), "-q", "-p", str(prof), *args, "-o", str(out / "f_%d.png")],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 2, (sub, r.stderr)
        assert not list(out.iterdir())
