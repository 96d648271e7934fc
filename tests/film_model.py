"""The progressive film of include/ptgpu.h (pt_film_*) restated in numpy: merge, noise (per pixel in float32, the
block tree in float32, the statistics in float64), resolve and the schedule of pt_film_render_until.  Written from the
header's definition, one IEEE operation per step; the GPU tests hold the kernels to it bit for bit."""
import numpy as np

f32 = np.float32
BLOCK = 256
MAX_SAMPLES = 1 << 24
DEFAULT_LUM_FLOOR = 0.01


def merge(film, frame):
    """film = film + pass, one f32 addition per float (accum and moments alike)."""
    return (np.asarray(film, f32) + np.asarray(frame, f32)).astype(f32)


def pixel_error(moments, n, lum_floor=DEFAULT_LUM_FLOOR):
    """err [n_local] float32 of moments [n_local, 2] = (m1, m2) for a total of n >= 2 samples."""
    m = np.asarray(moments, f32).reshape(-1, 2)
    N = f32(n)
    with np.errstate(all="ignore"):
        mu = (m[:, 0] / N).astype(f32)
        e2 = (m[:, 1] / N).astype(f32)
        sq = (mu * mu).astype(f32)
        s2 = np.maximum(f32(0), (e2 - sq).astype(f32)).astype(f32)
        vL = (s2 / f32(n - 1)).astype(f32)
        se = np.sqrt(vL).astype(f32)
        den = np.maximum(mu, f32(lum_floor)).astype(f32)
        return (se / den).astype(f32)


def blocks(err):
    """(block_sum, block_max) float32 of the blocks of 256 packed pixels: v padded with 0.f, then for stride = 128 .. 1:
    v[i] = v[i] + v[i + stride] for i < stride."""
    err = np.asarray(err, f32).reshape(-1)
    nb = (len(err) + BLOCK - 1) // BLOCK
    v = np.zeros((nb, BLOCK), f32)
    v.reshape(-1)[:len(err)] = err
    bmax = v.max(axis=1).astype(f32)   # (err >= 0: the padding never wins over a pixel)
    stride = BLOCK // 2
    while stride >= 1:
        v[:, :stride] = (v[:, :stride] + v[:, stride:2 * stride]).astype(f32)
        stride //= 2
    return v[:, 0].copy(), bmax


def statistics(block_sum, n_local, target, samples):
    """The fields of pt_film_noise_stats, in float64, b ascending."""
    S, worst, over = 0.0, 0.0, 0
    nb = len(block_sum)
    for b in range(nb):
        pixels = min(BLOCK, n_local - BLOCK * b)
        s = float(block_sum[b])
        mean_b = s / float(pixels)
        S = S + s
        if b == 0 or mean_b > worst:
            worst = mean_b
        if mean_b > target:
            over += 1
    mean = S / float(n_local)
    return {"mean_error": mean, "max_block_error": worst, "fraction_over": over / nb, "samples": samples, "n_blocks": nb,
            "converged": int(mean <= target)}


def noise(moments, n, target, lum_floor=DEFAULT_LUM_FLOOR):
    """(statistics, err, block_sum, block_max) of a film's moments with a total of n samples."""
    err = pixel_error(moments, n, lum_floor)
    bsum, bmax = blocks(err)
    return statistics(bsum, len(err), target, n), err, bsum, bmax


def resolve_color(accum, n):
    return (np.asarray(accum, f32) / f32(n)).astype(f32)


def schedule(first, max_samples, last=0, total=0):
    """The passes pt_film_render_until can add with a target that is never met: first (or 2 * last on a film that has
    passes), doubling, while the total stays <= min(max_samples, 2^24)."""
    cap = min(max_samples, MAX_SAMPLES)
    out = []
    while True:
        nxt = 2 * last if last else first
        if total + nxt > cap:
            return out
        out.append(nxt)
        total += nxt
        last = nxt


def render_until(noise_after, first, max_samples, target, last=0, total=0):
    """The schedule stopped by the noise: noise_after(k, total) -> mean_error of the film after pass k.  Returns the passes
    made and whether the last one converged."""
    made = []
    for k, n in enumerate(schedule(first, max_samples, last, total)):
        total += n
        made.append(n)
        if noise_after(k, total) <= target:
            return made, True
    return made, False


def synthetic_planes(n_local, n, seed):
    """Seeded (accum [n_local, 3], moments [n_local, 2]) of a film of n samples: m2/n >= (m1/n)^2 for most pixels, and the edge
    cases planted where the plane has room: zero variance, a mean below the floor, e2 < mu*mu (clamped to 0), a black pixel."""
    rng = np.random.default_rng(seed)
    mu = rng.uniform(0.02, 4.0, n_local)
    rel = rng.uniform(0.0, 1.5, n_local)
    m1 = (mu * n).astype(f32)
    m2 = ((mu * mu) * (1.0 + rel * rel) * n).astype(f32)
    if n_local > 0:   # zero variance: every sample the same luminance L (m1 = n L, m2 = n L^2, both exact for these values)
        m1[0], m2[0] = f32(0.5 * n), f32(0.25 * n)
    if n_local > 1:   # a mean below the floor
        m1[1], m2[1] = f32(0.001 * n), f32(0.00001 * n)
    if n_local > 2:   # e2 < mu*mu: a negative s2 is clamped
        m1[2], m2[2] = f32(2.0 * n), f32(3.0 * n)
    if n_local > 3:   # a black pixel
        m1[3], m2[3] = f32(0), f32(0)
    if n_local > 300:
        m1[-1], m2[-1] = f32(1.0 * n), f32(0.5 * n)   # clamped, in the last (partial) block
    accum = rng.uniform(0.0, 4.0 * n, (n_local, 3)).astype(f32)
    return accum, np.stack([m1, m2], axis=1).astype(f32)
