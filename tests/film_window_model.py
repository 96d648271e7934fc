"""Windowed films of include/ptgpu.h (pt_film_*window*) restated in numpy and driven by the sample planes of
pt_render_samples for the N-sample profile: the carry of a window frame (the additions of k_accumulate_moments, sample by
sample), the gather / carry / scatter of a tile window grouped by count, and the loop of pt_film_render_until_windowed.  Noise
and selection are film_adaptive_model's.  Written from the header's text; the GPU tests hold the library to it bit for bit."""
import numpy as np

import denoise_var_model as dvm
import film_adaptive_model as am
import film_model as fm

f32 = np.float32


def carry(accum, moments, planes, s0, s1):
    """A window frame on packed buffers: (accum [n, 3], moments [n, 2]) hold the sums of planes[:s0] (ignored when s0 == 0);
    returns them continued over planes[s0:s1] ([N, n, 3]), one f32 operation per step, in sample order."""
    planes = np.asarray(planes, f32)
    assert 0 <= s0 < s1 <= len(planes)
    if s0 == 0:
        acc, m1, m2 = np.zeros(planes.shape[1:], f32), np.zeros(planes.shape[1], f32), np.zeros(planes.shape[1], f32)
    else:
        acc, m1, m2 = np.array(accum, f32), np.array(moments, f32)[:, 0], np.array(moments, f32)[:, 1]
    with np.errstate(all="ignore"):
        for c in planes[s0:s1]:
            L = dvm.lum(c)
            acc = acc + c
            m1 = m1 + L
            m2 = m2 + L * L
    return acc.astype(f32), np.stack([m1, m2], axis=1).astype(f32)


def groups_by_count(tile_count, tiles):
    """The tile-list frames of one tile window: [(count, tiles at that count)], counts ascending, tiles ascending."""
    out = {}
    for t in tiles:
        out.setdefault(int(tile_count[t]), []).append(int(t))
    return [(c, sorted(out[c])) for c in sorted(out)]


class WindowFilm:
    """A windowed film of the enumeration planes [N, n_pixels, 3] (image order) over `tiling`."""

    def __init__(self, tiling, planes):
        self.tiling, self.planes, self.N = tiling, np.asarray(planes, f32), len(planes)
        assert self.planes.shape[1] == tiling.n_pixels
        self.reset()

    def reset(self):
        n = self.tiling.n_pixels
        self.accum, self.moments = np.zeros((n, 3), f32), np.zeros((n, 2), f32)
        self.counts = np.zeros(n, np.uint32)
        self.tile_count = [0] * self.tiling.n_tiles
        self.frames = []   # (s0, s1, tiles) of every tile-list window frame, in the order they are rendered

    @property
    def samples(self):
        return max(self.tile_count)

    def add_tile_window(self, samples, tiles):
        """Every listed tile from its own count; False (nothing changed) where the call is refused."""
        tiles = [int(t) for t in tiles]
        if samples < 1 or not self.tiling.check_list(tiles) or any(self.tile_count[t] + samples > self.N for t in tiles):
            return False
        acc, mom = self.accum.copy(), self.moments.copy()
        for c, group in groups_by_count(self.tile_count, tiles):
            where = self.tiling.pixel_map(group)                      # gather: the packed order of the group's frame
            a, m = carry(self.accum[where], self.moments[where], self.planes[:, where], c, c + samples)
            acc[where], mom[where] = a, m                             # scatter, once every frame is done
            self.frames.append((c, c + samples, group))
        self.accum, self.moments = acc, mom
        for t in tiles:
            self.tile_count[t] += samples
            self.counts[self.tiling.pixels(t)] += np.uint32(samples)
        return True

    def add_window(self, samples):
        return self.add_tile_window(samples, range(self.tiling.n_tiles))

    def tile_sums(self, target, lum_floor=fm.DEFAULT_LUM_FLOOR, active_tiles=0):
        st, _, tsum, _ = am.tile_noise(self.tiling, self.moments, self.counts, target, lum_floor, active_tiles)
        return st, tsum


def next_window(tile_count, tiles, window_samples, N):
    """Step 1 of the loop: (the listed tiles that are not full, the window clipped so that none of them passes N)."""
    todo = [t for t in tiles if tile_count[t] < N]
    if not todo:
        return [], 0
    return todo, min(window_samples, N - max(tile_count[t] for t in todo))


def render_until_windowed(film, window_samples, adaptive, uniform_samples, dilate_by, target, lum_floor=fm.DEFAULT_LUM_FLOOR):
    """pt_film_render_until_windowed on an EMPTY WindowFilm.  Returns ([(samples, tiles, statistics)], reason): the windows
    in order and "converged" (no candidate) or "budget" (no active tile has a sample left)."""
    assert film.samples == 0 and window_samples >= 2
    every = list(range(film.tiling.n_tiles))
    made, active, measured = [], every, False
    while True:
        everything = (not measured) or adaptive == 0 or film.samples < uniform_samples
        todo, w = next_window(film.tile_count, every if everything else active, window_samples, film.N)
        if not todo:
            return made, "budget"
        assert film.add_tile_window(w, todo)
        st, tsum = film.tile_sums(target, lum_floor, len(todo))
        measured = True
        made.append((w, todo, st))
        if not am.candidates(film.tiling, tsum, target):
            return made, "converged"
        active = am.next_active(film.tiling, tsum, target, dilate_by)
