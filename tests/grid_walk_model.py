"""The three list walks of csrc/pt_grid.h restated in numpy on top of OriginGrid.cells() / the grid's arrays, for host-built grids
and OriginGrid.from_device ones alike.  The per-primitive intersections come from the brute-force oracle's trace_all (the sorted
hit list of every ray): the model does not restate the intersection code, it tests the LISTS and the STOP RULES.

    closest(grid, rays, trace)                     og_next_hit for rays that start at the grid's origin (camera rays)
    blocked_point(grid, srays, trace, pos, ldist)  og_blocker<RANGED = true>  (the cell is looked up with pos - origin, as
                                                   og_light_radiance does)
    blocked_ortho(grid, srays, trace)              og_blocker<RANGED = false> with the scan limit -depth(ray origin)

trace = (hits, counts) of oracle.OracleScene.trace_all(rays, K).  A ray with more than K hits is not modelled (`truncated`).

How a sequential walk is evaluated without a loop: a cell's list ascends in its distance word (lists_sorted checks that), and
best.key only shrinks while the walk goes on.  So entry e is tested iff  m_e <= kmax * min{key of the hits of entries before e}
(globals count as before everything): if that holds for e it holds for every entry before e, and if an entry before e ended
the walk it fails for e.  The float32 product is monotone, so taking the minimum first is the same comparison the device
makes against best.key * kmax."""
import numpy as np

F32 = np.float32
INDEX = 0x7fffffff


def mag3(a):
    """mag3 (csrc/pt_math.h) in float32: sqrtf(x x + y y + z z), summed left to right."""
    a = a.astype(F32)
    return np.sqrt(((a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]).astype(F32) + a[:, 2] * a[:, 2]).astype(F32)).astype(F32)


def camera_kmax(d):
    """kmax of a camera ray of direction d (pt_wf_shade_body.h:176, pt_grid_kernels.h:30), float32."""
    dlen = mag3(d)
    return (np.where(dlen > F32(1.0), dlen, F32(1.0)).astype(F32) * F32(1.00002)).astype(F32)


class Lists:
    """(cell, primitive) -> entry of a grid's lists."""

    def __init__(self, grid, n_prims):
        self.grid, self.n_prims = grid, int(n_prims)
        n, ng = grid.n_refs, grid.n_global
        self.prim = (grid.ref_prim[:n] & INDEX).astype(np.int64)
        self.word = grid.ref_mindist[:n].astype(F32)
        self.global_rank = np.full(self.n_prims, -1, np.int64)
        self.global_rank[self.prim[:ng]] = np.arange(ng)
        off = grid.cell_off.astype(np.int64)
        self.first, self.last = int(off[0]), int(off[-1])
        idx = np.arange(self.first, self.last)
        self.owner = np.repeat(np.arange(len(off) - 1, dtype=np.int64), np.diff(off))
        key = self.owner * self.n_prims + self.prim[self.first:self.last]
        order = np.argsort(key, kind="stable")
        self.keys, self.refs = key[order], idx[order]

    def lists_sorted(self):
        """Every cell's list ascends in its distance word (what the walks' `break` relies on)."""
        w = self.word[self.first:self.last]
        same = self.owner[1:] == self.owner[:-1]
        return bool(np.all(~same | (w[1:] >= w[:-1])))

    def lookup(self, cells, prims):
        """cells [n], prims [n, K] (-1: none) -> (rank [n, K], word [n, K], is_global [n, K], found [n, K]).  rank orders the
        entries as the walks meet them: the global block first, then the cell's entries."""
        p = np.where(prims >= 0, prims, 0).astype(np.int64)
        g = self.global_rank[p]
        key = cells.astype(np.int64)[:, None] * self.n_prims + p
        at = np.minimum(np.searchsorted(self.keys, key), max(len(self.keys) - 1, 0))
        in_cell = (self.keys[at] == key) if len(self.keys) else np.zeros(key.shape, bool)
        ref = self.refs[at] if len(self.keys) else np.zeros(key.shape, np.int64)
        is_global = (g >= 0) & (prims >= 0)
        found = is_global | (in_cell & (prims >= 0))
        rank = np.where(is_global, g, ref)
        word = np.where(is_global, F32(-np.inf), self.word[ref] if len(self.word) else F32(0)).astype(F32)
        return rank, word, is_global, found


def _valid(hits, counts):
    K = hits.shape[1]
    return np.arange(K)[None, :] < np.minimum(counts, K)[:, None], counts > K


def _closest(lists, rays, trace):
    hits, counts = trace
    valid, truncated = _valid(hits, counts)
    d = rays[:, 3:].astype(F32)
    cells = lists.grid.cells(d)
    kmax = camera_kmax(d)
    rank, word, is_global, found = lists.lookup(cells, np.where(valid, hits["prim"], -1))
    key = hits["dist"].astype(F32)
    usable = valid & found
    # smallest key among the hits of entries met earlier
    earlier = usable[:, None, :] & (rank[:, None, :] < rank[:, :, None])          # [n, h, g]: g is met before h
    prev = np.where(earlier, key[:, None, :], F32(np.inf)).min(axis=2).astype(F32)
    with np.errstate(invalid="ignore", over="ignore"):
        limit = (prev * kmax[:, None]).astype(F32)
    tested = usable & (is_global | ~(word > limit))
    order = hits["prim"].astype(np.int64) * 2 + ((hits["flags"] & 4) != 0)
    k = np.where(tested, key, F32(np.inf))
    best = k.min(axis=1)
    tie = tested & (k == best[:, None])
    pick = np.where(tie, order, np.iinfo(np.int64).max).argmin(axis=1)
    hit = tested.any(axis=1)
    i = np.arange(len(rays))
    return dict(prim=np.where(hit, hits["prim"][i, pick], -1), flags=np.where(hit, hits["flags"][i, pick], 0),
                key=np.where(hit, key[i, pick], F32(0)).astype(F32), truncated=truncated)


def closest(lists, rays, trace, block=8192):
    """og_next_hit from t_prev = -inf, cutoff = inf.  Returns dict(prim [n] (-1: miss), flags [n], key [n] float32, truncated [n]):
    the entry the walk returns, to be compared with trace's first hit.  (In blocks of rows: the [n, K, K] tables stay small.)"""
    parts = [_closest(lists, rays[i:i + block], (trace[0][i:i + block], trace[1][i:i + block])) for i in range(0, len(rays), block)]
    if not parts:
        return dict(prim=np.zeros(0, np.int64), flags=np.zeros(0, np.int64), key=np.zeros(0, F32), truncated=np.zeros(0, bool))
    return {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}


def first_of(trace):
    """trace's first hit in closest()'s form."""
    hits, counts = trace
    hit = counts > 0
    return dict(prim=np.where(hit, hits["prim"][:, 0], -1), flags=np.where(hit, hits["flags"][:, 0], 0),
                key=np.where(hit, hits["dist"][:, 0], F32(0)).astype(F32))


def same_hit(a, b):
    return (a["prim"] == b["prim"]) & (a["flags"] == b["flags"]) & (a["key"].view(np.uint32) == b["key"].view(np.uint32))


def passes_range(srays, hits, pos, ldist):
    """The range test of get_light_info (mod.rs:319-321) as og_blocker forms it: mag3((so + sd t) - pos) <= ldist in float32.
    trace_all reports a triangle's ray parameter and a sphere's Euclidean distance from the ray's origin; a sphere's parameter is
    that distance over |sd| (sd is a float32-normalised vector: the two differ by rounding only)."""
    so, sd = srays[:, None, :3].astype(F32), srays[:, None, 3:].astype(F32)
    sphere = (hits["flags"] & 2) != 0
    t = np.where(sphere, (hits["dist"] / mag3(srays[:, 3:])[:, None]).astype(F32), hits["dist"]).astype(F32)
    x = ((so + (sd * t[:, :, None]).astype(F32)).astype(F32) - pos[:, None, :].astype(F32)).astype(F32)
    m = np.sqrt(((x[..., 0] * x[..., 0] + x[..., 1] * x[..., 1]).astype(F32) + x[..., 2] * x[..., 2]).astype(F32)).astype(F32)
    return ~(m > ldist[:, None])


def blocked_point(lists, srays, trace, pos, ldist):
    """og_blocker<RANGED = true> for the shadow rays `srays` of the surface points `pos`, ldist = mag3(pos - origin): the cell of
    pos - origin, the global block, then the cell's entries up to the first whose distance word exceeds ldist; a hit counts if it
    passes the range test.  Returns dict(blocked [n], expected [n], needed [n, K], ...): expected = trace holds a hit that passes."""
    hits, counts = trace
    valid, truncated = _valid(hits, counts)
    origin = np.array(list(lists.grid.c.origin), F32)
    direction = (pos.astype(F32) - origin).astype(F32)
    cells = lists.grid.cells(direction)
    rank, word, is_global, found = lists.lookup(cells, np.where(valid, hits["prim"], -1))
    needed = valid & passes_range(srays, hits, pos, ldist)
    tested = valid & found & (is_global | ~(word > ldist[:, None]))
    return dict(blocked=(tested & needed).any(axis=1), expected=needed.any(axis=1), needed=needed, tested=tested, found=found,
                word=word, is_global=is_global, truncated=truncated, cells=cells)


def blocked_ortho(lists, srays, trace):
    """og_blocker<RANGED = false>: the cell of the ray's origin, the global block, then the cell's entries up to the first whose
    key exceeds -depth(origin); any hit counts."""
    hits, counts = trace
    valid, truncated = _valid(hits, counts)
    so = srays[:, :3].astype(F32)
    cells = lists.grid.cells(so)
    limit = (-lists.grid.depth(so)).astype(F32)
    rank, word, is_global, found = lists.lookup(cells, np.where(valid, hits["prim"], -1))
    tested = valid & found & (is_global | ~(word > limit[:, None]))
    return dict(blocked=tested.any(axis=1), expected=valid.any(axis=1), needed=valid, tested=tested, found=found, word=word,
                is_global=is_global, truncated=truncated, cells=cells, limit=limit)
