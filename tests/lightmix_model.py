"""The light mixer's arithmetic in numpy float32, written from include/ptgpu.h (pt_lightmix_capture, pt_lightmix_apply): one
IEEE f32 operation per step in the order the header writes them.  numpy rounds every elementwise float32 operation on its own,
so `a + f * d` below is a product rounded to f32 followed by a sum rounded to f32 - the uncontracted form the kernel is
compiled to."""
import numpy as np

f32 = np.float32
MAX_LIGHTS = 16


def units(colors):
    """m_l: the largest channel of light l's colour, or 1.0 if that is 0.  colors: [n, 3]."""
    c = np.asarray(colors, f32).reshape(-1, 3)
    m = c.max(axis=1) if len(c) else np.zeros(0, f32)
    return np.where(m == 0, f32(1), m).astype(f32)


def basis_colors(colors, plane):
    """The light colours of the frame behind plane `plane`: 0 = every light black (E), 1 + l = light l at (m_l, m_l, m_l) and the
    others black (F_l)."""
    c = np.zeros_like(np.asarray(colors, f32).reshape(-1, 3))
    if plane > 0:
        c[plane - 1, :] = units(colors)[plane - 1]
    return c


def capture(frames):
    """frames: [n + 1, n_local, 3] accumulators E, F_0 .. F_{n-1}.  Returns the planes E, D_l = F_l - E."""
    frames = np.asarray(frames, f32)
    planes = frames.copy()
    planes[1:] = frames[1:] - frames[0]
    return planes


def factors(colors, unit):
    """f[l][ch] = colors[l][ch] / unit[l]"""
    c = np.asarray(colors, f32).reshape(-1, 3)
    return (c / np.asarray(unit, f32).reshape(-1, 1)).astype(f32)


def apply(planes, unit, colors):
    """accum [n_local, 3]: a = E; for l in order: a = a + f[l][ch] * D_l."""
    planes = np.asarray(planes, f32)
    f = factors(colors, unit)
    a = planes[0].copy()
    with np.errstate(all="ignore"):
        for l in range(len(f)):
            a = a + f[l][None, :] * planes[1 + l]
    return a.astype(f32)


def apply_f64(planes, unit, colors):
    """The same mix summed in float64 (the reconstruction the issue's CPU measurement used)."""
    planes = np.asarray(planes, np.float64)
    f = np.asarray(colors, np.float64).reshape(-1, 3) / np.asarray(unit, np.float64).reshape(-1, 1)
    return planes[0] + (f[:, None, :] * planes[1:]).sum(axis=0) if len(f) else planes[0].copy()


def synthetic_planes(n_lights, n_local, seed):
    """Planes that exercise the mix: ordinary radiance, fireflies, exact zeros, negative differences, a few denormals.
    Returns (planes [n_lights + 1, n_local, 3], unit [n_lights], samples)."""
    rng = np.random.default_rng(seed)
    shape = (n_lights + 1, n_local, 3)
    p = rng.gamma(0.6, 2.0, shape).astype(f32)
    p[rng.random(shape) < 0.02] *= f32(3.0e4)           # fireflies
    p[rng.random(shape) < 0.10] = f32(0)                # black
    neg = rng.random(shape) < 0.25
    neg[0] = False
    p[neg] = -p[neg] * f32(0.01)                        # D_l may be negative by rounding; E is not
    p[rng.random(shape) < 0.01] = f32(1e-41)
    unit = rng.choice(np.array([1.0, 0.25, 1000.0, 37.5, 3.0], f32), n_lights).astype(f32)
    return p, unit, int(rng.integers(1, 9))


def random_colors(rng, base, mute=None):
    """base colours times per-channel factors in [0.2, 3); light `mute` black."""
    base = np.asarray(base, f32).reshape(-1, 3)
    c = (base * rng.uniform(0.2, 3.0, base.shape).astype(f32)).astype(f32)
    if mute is not None and len(c):
        c[mute % len(c)] = 0
    return c
