"""The adaptive film of include/ptgpu.h (tile-list frames and pt_film_*tile*) restated in numpy: the tile map and
the packed order of a tile list, the scatter-merge with its counts, the tile-noise tree (float32) and its statistics (float64),
candidates and dilation, and the schedule of pt_film_render_until_adaptive.  Written from the header's text, one IEEE operation
per step; the GPU tests hold the kernels to it bit for bit."""
import numpy as np

import film_model as fm

f32 = np.float32
MAX_SAMPLES = fm.MAX_SAMPLES


class Tiling:
    """The tiling of a width x height image: tile k = ty * tiles_x + tx, clipped to the image."""

    def __init__(self, width, height, tile_w=32, tile_h=32):
        self.width, self.height, self.tile_w, self.tile_h = width, height, tile_w, tile_h
        self.tiles_x = (width + tile_w - 1) // tile_w
        self.tiles_y = (height + tile_h - 1) // tile_h
        self.n_tiles = self.tiles_x * self.tiles_y
        self.n_pixels = width * height

    def rect(self, k):
        """(x0, y0, cw, ch) of tile k."""
        x0, y0 = (k % self.tiles_x) * self.tile_w, (k // self.tiles_x) * self.tile_h
        return x0, y0, min(self.tile_w, self.width - x0), min(self.tile_h, self.height - y0)

    def pixels(self, k):
        """Global indices x + y * width of tile k's pixels in the order j = y * cw + x."""
        x0, y0, cw, ch = self.rect(k)
        ys, xs = np.mgrid[y0:y0 + ch, x0:x0 + cw]
        return (xs + ys * self.width).reshape(-1).astype(np.uint32)

    def check_list(self, tiles):
        """What a tile list must be: not empty, strictly ascending, every number below n_tiles."""
        t = [int(k) for k in tiles]
        return bool(t) and all(0 <= k < self.n_tiles for k in t) and all(a < b for a, b in zip(t, t[1:]))

    def pixel_map(self, tiles):
        """pt_tiles_pixel_map: the global index of every packed pixel - the tiles one after the other in list order."""
        assert self.check_list(tiles)
        return np.concatenate([self.pixels(int(k)) for k in tiles])


def merge_tiles(tiling, film_accum, film_mom, counts, tiles, pass_accum, pass_mom, samples):
    """The scatter-merge: film = film + pass on the pixels of the listed tiles (the pass planes packed), count += samples; every
    other pixel keeps its bits.  Returns new (accum, moments, counts)."""
    where = tiling.pixel_map(tiles)
    acc, mom, cnt = np.array(film_accum, f32), np.array(film_mom, f32), np.array(counts, np.uint32)
    acc[where] = (acc[where] + np.asarray(pass_accum, f32)).astype(f32)
    mom[where] = (mom[where] + np.asarray(pass_mom, f32)).astype(f32)
    cnt[where] += np.uint32(samples)
    return acc, mom, cnt


def pixel_error(moments, counts, lum_floor=fm.DEFAULT_LUM_FLOOR):
    """pt_film_noise's err with n = the pixel's own count (every count >= 2)."""
    m = np.asarray(moments, f32).reshape(-1, 2)
    n = np.asarray(counts, np.uint32).reshape(-1)
    N = n.astype(f32)
    with np.errstate(all="ignore"):
        mu = (m[:, 0] / N).astype(f32)
        e2 = (m[:, 1] / N).astype(f32)
        sq = (mu * mu).astype(f32)
        s2 = np.maximum(f32(0), (e2 - sq).astype(f32)).astype(f32)
        vL = (s2 / (n - np.uint32(1)).astype(f32)).astype(f32)
        se = np.sqrt(vL).astype(f32)
        den = np.maximum(mu, f32(lum_floor)).astype(f32)
        return (se / den).astype(f32)


def tile_tree(err_tile):
    """(sum, max) float32 of one tile's errors in the order j: v[i] = 0.f, then v[i] = v[i] + err_j for j = i, i + 256, ...;
    then for stride = 128 .. 1: v[i] = v[i] + v[i + stride] for i < stride.  The maximum goes down the same steps."""
    e = np.asarray(err_tile, f32).reshape(-1)
    v, w = np.zeros(256, f32), np.zeros(256, f32)
    for j0 in range(0, len(e), 256):
        part = e[j0:j0 + 256]
        v[:len(part)] = (v[:len(part)] + part).astype(f32)
        w[:len(part)] = np.maximum(w[:len(part)], part).astype(f32)
    stride = 128
    while stride >= 1:
        v[:stride] = (v[:stride] + v[stride:2 * stride]).astype(f32)
        w[:stride] = np.maximum(w[:stride], w[stride:2 * stride]).astype(f32)
        stride //= 2
    return v[0], w[0]


def tile_arrays(tiling, err):
    """(tile_sum, tile_max) float32 [n_tiles] of an err plane in image order."""
    out = [tile_tree(np.asarray(err, f32)[tiling.pixels(k)]) for k in range(tiling.n_tiles)]
    return np.array([o[0] for o in out], f32), np.array([o[1] for o in out], f32)


def statistics(tiling, tile_sum, counts, target, active_tiles=0):
    """The fields of pt_film_tile_stats, in float64, t ascending."""
    S, worst, over = 0.0, 0.0, 0
    for t in range(tiling.n_tiles):
        _, _, cw, ch = tiling.rect(t)
        s = float(tile_sum[t])
        mean_t = s / float(cw * ch)
        S = S + s
        if t == 0 or mean_t > worst:
            worst = mean_t
        if mean_t > target:
            over += 1
    counts = np.asarray(counts, np.uint64)
    return {"mean_error": S / float(tiling.n_pixels), "max_tile_error": worst, "samples": int(counts.max()),
            "pixel_samples": int(counts.sum()), "n_tiles": tiling.n_tiles, "over_tiles": over, "active_tiles": active_tiles,
            "converged": int(over == 0)}


def tile_noise(tiling, moments, counts, target, lum_floor=fm.DEFAULT_LUM_FLOOR, active_tiles=0):
    """(statistics, err, tile_sum, tile_max) of a film's moments and per-pixel counts."""
    err = pixel_error(moments, counts, lum_floor)
    tsum, tmax = tile_arrays(tiling, err)
    return statistics(tiling, tsum, counts, target, active_tiles), err, tsum, tmax


def candidates(tiling, tile_sum, target):
    """The tiles whose mean error (float64) exceeds the target, ascending."""
    return [t for t in range(tiling.n_tiles) if float(tile_sum[t]) / float(tiling.rect(t)[2] * tiling.rect(t)[3]) > target]


def dilate(tiling, tiles, radius=1):
    """The tiles and - radius 1 - their 8 neighbours inside the image, ascending."""
    on = set()
    for t in tiles:
        tx, ty = t % tiling.tiles_x, t // tiling.tiles_x
        for y in range(max(0, ty - radius), min(tiling.tiles_y - 1, ty + radius) + 1):
            for x in range(max(0, tx - radius), min(tiling.tiles_x - 1, tx + radius) + 1):
                on.add(y * tiling.tiles_x + x)
    return sorted(on)


def next_active(tiling, tile_sum, target, dilate_by):
    return dilate(tiling, candidates(tiling, tile_sum, target), dilate_by)


def render_until_adaptive(tiling, noise_after, first, uniform_samples, dilate_by, target, max_samples, last=0, total=0):
    """The loop of pt_film_render_until_adaptive on an empty film (or one of uniform passes below uniform_samples):
    noise_after(k, samples, tiles) -> tile_sum of the film after pass k of `samples` samples over `tiles` (a list; every tile
    while the film is empty or its largest count is below uniform_samples).  Returns ([(samples, tiles)], reason) with reason
    "converged" (no candidate) or "budget" (the next pass would take the largest count above min(max_samples, 2^24)).
    `total` is the largest count: some pixel takes every pass as long as the active sets shrink."""
    cap = min(max_samples, MAX_SAMPLES)
    every = list(range(tiling.n_tiles))
    made, active = [], every
    while True:
        nxt = 2 * last if last else first
        if total + nxt > cap:
            return made, "budget"
        tiles = every if (not made and not last) or total < uniform_samples else active
        tsum = noise_after(len(made), nxt, tiles)
        made.append((nxt, tiles))
        total += nxt
        last = nxt
        if not candidates(tiling, tsum, target):
            return made, "converged"
        active = next_active(tiling, tsum, target, dilate_by)
