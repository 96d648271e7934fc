"""The light mixer's premise on the CPU: a frame rebuilt from the planes E, D_l (tests/lightmix_model.py) of ORACLE frames equals
the oracle's real frame of the scene with the edited light colours, within the project's smoke tolerance and 1 LSB."""
import numpy as np
import pytest

import lightmix_model as lm
from conftest import SCENES

f32 = np.float32
GOLDEN = ("cube", "head", "spheres", "reflection", "alpha_transparency")
W, H, SAMPLES, BOUNCES = 64, 48, 8, 4


def with_colors(lights, colors):
    """Copies of `lights` with colours [n, 3]."""
    out = []
    for l, c in zip(lights, np.asarray(colors, f32).reshape(-1, 3)):
        k = type(l).from_buffer_copy(l)
        k.color[0], k.color[1], k.color[2] = float(c[0]), float(c[1]), float(c[2])
        out.append(k)
    return out


def light_colors(lights):
    return np.array([[l.color[0], l.color[1], l.color[2]] for l in lights], f32).reshape(-1, 3)


def oracle_frame(oracle, host, lights, colors, prof):
    host.set_lights(with_colors(lights, colors))
    rgb, acc, _ = oracle.OracleScene(host.desc, oracle.PTO_BVH).render(prof)
    return rgb, acc


def test_the_colour_only_comparison_of_light_tables(pta):
    """pth_lights_differ_in_color_only: count, kind, vec and size bit for bit; colours are free."""
    import ctypes as C
    fn = pta.host_lib().pth_lights_differ_in_color_only
    base = pta.HostScene.load_isf(SCENES / "head" / "scene.isf").lights
    assert len(base) == 2

    def table(ls):
        return (pta.Light * max(1, len(ls)))(*ls), len(ls)

    def edited(i, field, value):
        ls = [type(l).from_buffer_copy(l) for l in base]
        if field == "vec":
            ls[i].vec[1] = value
        else:
            setattr(ls[i], field, value)
        return ls
    a, n = table(base)
    assert fn(a, n, *table(with_colors(base, [[0, 0, 0], [9, 8, 7]]))) == 1
    assert fn(a, n, *table(edited(0, "kind", 1 - base[0].kind))) == 0
    assert fn(a, n, *table(edited(1, "vec", base[1].vec[1] + 1.0))) == 0
    assert fn(a, n, *table(edited(0, "size", base[0].size + 0.5))) == 0
    assert fn(a, n, *table(base[:1])) == 0 and fn(a, n, a, 1) == 0
    zero, minus = edited(0, "vec", 0.0), edited(0, "vec", -0.0)
    assert fn(*table(zero), *table(minus)) == 0 and fn(*table(zero), *table(zero)) == 1
    assert fn(None, 0, None, 0) == 1 and fn(None, 2, a, n) == 0
    assert C.sizeof(pta.LightMixInfo) == 24 + 4 * pta.PT_LIGHTMIX_MAX_LIGHTS


@pytest.mark.parametrize("name", GOLDEN)
def test_mix_of_oracle_planes_equals_the_oracle_frame_of_the_edited_scene(pta, oracle, name):
    host = pta.HostScene.load_isf(SCENES / name / "scene.isf")
    prof = pta.Profile.make(W, H, SAMPLES, BOUNCES)
    lights = host.lights
    base = light_colors(lights)
    unit = lm.units(base)
    frames = [oracle_frame(oracle, host, lights, lm.basis_colors(base, i), prof)[1] for i in range(len(lights) + 1)]
    planes = lm.capture(np.stack(frames))
    rng = np.random.default_rng(7 + len(name))
    worst32 = worst64 = 0.0
    for k in range(3):
        colors = lm.random_colors(rng, base, mute=k if k == 2 else None)
        ref_rgb, ref = oracle_frame(oracle, host, lights, colors, prof)
        tol = 1e-4 * SAMPLES + 1e-3 * np.abs(ref)
        mix = lm.apply(planes, unit, colors)
        r32 = float((np.abs(mix.astype(np.float64) - ref) / tol).max())
        r64 = float((np.abs(lm.apply_f64(planes, unit, colors) - ref) / tol).max())
        worst32, worst64 = max(worst32, r32), max(worst64, r64)
        rgb = oracle.post_process(prof, mix)
        lsb = int(np.abs(rgb.astype(int) - ref_rgb.astype(int)).max())
        print(f"{name} set {k}: f32 mix {r32:.3e} of the tolerance, f64 mix {r64:.3e}, rgb8 {lsb} LSB")
        assert r32 <= 1.0 and r64 <= 1.0, (name, k, r32, r64)
        assert lsb <= 1, (name, k, lsb)
    print(f"{name}: worst ratio f32 {worst32:.3e}, f64 {worst64:.3e}")
