"""Sharded films of include/ptgpu.h (pt_film_*shard*) restated in numpy: which rank holds a tile, the packed order of
a shard film's planes, the merge and the tile noise in that order - by mapping through the pixel map into film_adaptive_model,
which is what "the same arithmetic on pixels found elsewhere" means - and the loop of N ranks in lock-step.  Written from the
header's text; the GPU tests hold the library to it bit for bit."""
import numpy as np

import film_adaptive_model as am
import film_model as fm

f32 = np.float32


def rank_stride(count):
    """s of the rule (tx + ty * s) % count: the smallest odd number >= 3 coprime to count, 1 for one or two ranks."""
    if count <= 2:
        return 1
    s = 3
    while np.gcd(s, count) != 1:
        s += 2
    return s


def tile_rank(tiling, k, count):
    """The rank that holds tile k of `tiling` among `count` ranks."""
    return (k % tiling.tiles_x + (k // tiling.tiles_x) * rank_stride(count)) % count if count > 1 else 0


class Shard:
    """Rank `rank` of `count` over `tiling`: its tiles ascending, their packed offsets, the global index of every packed pixel.
    One rank holds the image in image order (pt_local_pixel_map with shard_count <= 1)."""

    def __init__(self, tiling, rank, count):
        self.tiling, self.rank, self.count = tiling, rank, max(1, count)
        self.tiles = [k for k in range(tiling.n_tiles) if tile_rank(tiling, k, self.count) == rank]
        sizes = [tiling.rect(k)[2] * tiling.rect(k)[3] for k in self.tiles]
        self.offsets = [int(o) for o in np.concatenate([[0], np.cumsum(sizes)])]
        if self.count == 1:
            self.map = np.arange(tiling.n_pixels, dtype=np.uint32)
        else:
            self.map = tiling.pixel_map(self.tiles) if self.tiles else np.zeros(0, np.uint32)
        self.n_local = len(self.map)
        self.local_of = np.full(tiling.n_pixels, -1, np.int64)   # global pixel -> packed local pixel
        self.local_of[self.map] = np.arange(self.n_local)

    def base(self, k):
        """The first packed pixel of tile k (None: another rank's); packed films only."""
        return self.offsets[self.tiles.index(k)] if k in self.tiles else None

    def own(self, tiles):
        """The listed tiles this rank holds, in list order."""
        return [int(k) for k in tiles if tile_rank(self.tiling, int(k), self.count) == self.rank]

    def list_pixels(self, tiles):
        """The global pixels of the rank's listed tiles, packed in list order: the order of the host planes of
        pt_film_add_tile_planes on a shard film, and of the tile-list frame a tile pass renders."""
        own = self.own(tiles)
        return self.tiling.pixel_map(own) if own else np.zeros(0, np.uint32)

    def to_image(self, local, fill=0):
        """A packed local plane in image order, `fill` where other ranks' pixels are."""
        local = np.asarray(local)
        out = np.full((self.tiling.n_pixels,) + local.shape[1:], fill, local.dtype)
        out[self.map] = local
        return out


def merge_tiles(shard, accum, moments, counts, tiles, pass_accum, pass_mom, samples):
    """film = film + pass on the rank's listed tiles (the pass planes: shard.list_pixels(tiles) order), count += samples there;
    packed local planes in, new ones out.  A list with none of the rank's tiles changes no plane."""
    own = shard.own(tiles)
    if not own:
        return np.array(accum, f32), np.array(moments, f32), np.array(counts, np.uint32)
    a, m, c = am.merge_tiles(shard.tiling, shard.to_image(np.asarray(accum, f32)), shard.to_image(np.asarray(moments, f32)),
                             shard.to_image(np.asarray(counts, np.uint32)), own, pass_accum, pass_mom, samples)
    return a[shard.map], m[shard.map], c[shard.map]


def tile_noise(shard, moments, counts, lum_floor=fm.DEFAULT_LUM_FLOOR):
    """pt_film_shard_tile_noise: (err [n_local] packed, tile_sum, tile_max [n_tiles]) - a tile's figures from its own pixels,
    +0.f for the tiles of other ranks."""
    t = shard.tiling
    err = am.pixel_error(moments, counts, lum_floor)
    tsum, tmax = np.zeros(t.n_tiles, f32), np.zeros(t.n_tiles, f32)
    for k in shard.tiles:
        tsum[k], tmax[k] = am.tile_tree(err[shard.local_of[t.pixels(k)]])
    return err, tsum, tmax


def combine(arrays):
    """The exchange: element-wise over the ranks' arrays.  Unowned entries are +0.f and errors are not negative, so the sum, the
    maximum and the owner's value are the same bits; this is the sum."""
    out = np.zeros_like(arrays[0])
    for a in arrays:
        out = (out + a).astype(f32)
    return out


class ModelFilm:
    """Planes and counts of one holder of a film: a Shard's packed part, or the whole image (Shard(tiling, 0, 1))."""

    def __init__(self, shard):
        self.shard = shard
        n = shard.n_local
        self.accum, self.moments, self.counts = np.zeros((n, 3), f32), np.zeros((n, 2), f32), np.zeros(n, np.uint32)
        self.tile_count = [0] * shard.tiling.n_tiles   # of every tile of the image: tile lists are global

    def add_tile_pass(self, tiles, frame_accum, frame_mom, samples):
        """A pass over `tiles` whose whole frame (image order) is (frame_accum, frame_mom)."""
        where = self.shard.list_pixels(tiles)
        self.accum, self.moments, self.counts = merge_tiles(self.shard, self.accum, self.moments, self.counts, tiles,
                                                            frame_accum[where], frame_mom[where], samples)
        for k in tiles:
            self.tile_count[k] += samples

    def sums(self, lum_floor):
        return tile_noise(self.shard, self.moments, self.counts, lum_floor)[1]


def render_until_adaptive_lockstep(tiling, n_ranks, frame, first, uniform_samples, dilate_by, target, max_samples,
                                   lum_floor=fm.DEFAULT_LUM_FLOOR):
    """pt_film_render_until_adaptive_sharded on n_ranks empty model ranks, in lock-step: frame(samples) -> the whole frame
    (accum, moments) in image order of a pass of `samples` samples.  Every rank takes the pass over the same global list, measures
    its own tiles, and the combined sums drive am.render_until_adaptive's schedule - the unsharded loop's own code.  Returns
    (films, [(samples, tiles)], reason, the combined tile sums after the last pass)."""
    films = [ModelFilm(Shard(tiling, r, n_ranks)) for r in range(n_ranks)]
    last = {}

    def noise_after(_k, samples, tiles):
        fa, fm_ = frame(samples)
        for f in films:
            f.add_tile_pass(tiles, fa, fm_, samples)
        last["sums"] = combine([f.sums(lum_floor) for f in films])
        return last["sums"]
    made, why = am.render_until_adaptive(tiling, noise_after, first, uniform_samples, dilate_by, target, max_samples)
    return films, made, why, last.get("sums")


def assemble(films):
    """The shards' planes and counts in image order: (accum, moments, counts)."""
    t = films[0].shard.tiling
    acc, mom, cnt = np.zeros((t.n_pixels, 3), f32), np.zeros((t.n_pixels, 2), f32), np.zeros(t.n_pixels, np.uint32)
    for f in films:
        acc[f.shard.map], mom[f.shard.map], cnt[f.shard.map] = f.accum, f.moments, f.counts
    return acc, mom, cnt
