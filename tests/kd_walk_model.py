"""What a ray REACHES in the builder's KD-tree, never what it hits: the scalar walk of tests/test_abi_and_kd.py
(visited_prims: csrc/pt_integrator.h kd_traverse) restated over many rays at once, with the bookkeeping the walkers' stacks are
about - the height of the stack of pending far children.  tests/test_kd_tree_shapes.py uses it to CERTIFY that its scenes and
rays drive the device walkers into the parts of their code that shallow trees leave unexecuted (the overflow halves of
stack_push / stack_get behind WF_LDS_STACK and WF_EXACT_LDS_STACK, entry lists of several WF_ENTRY_BATCH batches, trees around
WF_LDS_NODES slots).  Expected values never come from here: they come from tests/geometry_model.py (brute force) and the oracle.

The device walkers place planes with v_rcp_f32 and carry slacks of their own (exit_rel), so their heights may differ from
these by a step or two: every condition built on this model keeps a margin of 2 from the constant it is about.
"""
import ctypes as C
import re

import numpy as np

from conftest import ROOT

F32 = np.float32
CSRC = ROOT / "path-tracer_amd" / "csrc"


def _define(path, name):
    m = re.search(r"^\s*#\s*define\s+" + name + r"\s+(\d+)u?\b", path.read_text(), re.M)
    assert m, (name, "not defined as a number in", path.name)
    return int(m.group(1))


WF_LDS_STACK = _define(CSRC / "pt_wavefront.h", "WF_LDS_STACK")
WF_EXACT_LDS_STACK = _define(CSRC / "pt_wavefront.h", "WF_EXACT_LDS_STACK")
WF_ENTRY_BATCH = _define(CSRC / "pt_wavefront.h", "WF_ENTRY_BATCH")
WF_LDS_NODES = _define(CSRC / "pt_wavefront.h", "WF_LDS_NODES")
PT_KD_STACK = _define(CSRC / "pt_device.h", "PT_KD_STACK")
_m = re.search(r'env_float\("PT_KD_MAX_LEAF",\s*(\d+)', (ROOT / "path-tracer_amd" / "host" / "kd_build.cpp").read_text())
PT_KD_MAX_LEAF = int(_m.group(1))      # the builder's default leaf size
ENTRY_LIST_CAP = 63                    # prep_entry_lists cuts the descent at depth >= 63 (6 bits of the entry word)


class Tree:
    """pth_kd_build's output for a built scene: nodes [n, 2] (builder layout: below child = node + 1), refs, bounds."""

    def __init__(self, pta, built):
        kd = pta.KdTree()
        pta.check_host(pta.host_lib().pth_kd_build(built.desc, C.byref(kd)))   # (built: a BuiltScene, alive during the call)
        self.nodes = np.ctypeslib.as_array(C.cast(kd.nodes, C.POINTER(C.c_uint32)), (max(1, kd.n_nodes), 2)).copy()[: kd.n_nodes]
        self.refs = np.ctypeslib.as_array(kd.refs, (max(1, kd.n_refs),)).copy()[: kd.n_refs]
        self.n_nodes, self.n_refs, self.n_leaves, self.depth = int(kd.n_nodes), int(kd.n_refs), int(kd.n_leaves), int(kd.depth)
        self.bmin, self.bmax = np.array(kd.bounds_min, F32), np.array(kd.bounds_max, F32)
        pta.host_lib().pth_kd_free(C.byref(kd))
        self.info = dict(n_nodes=self.n_nodes, n_refs=self.n_refs, n_leaves=self.n_leaves, depth=self.depth, bmin=self.bmin,
                         bmax=self.bmax)
        self.axis = (self.nodes[:, 1] & 3).astype(np.int64)
        self.split = self.nodes[:, 0].copy().view(F32)
        self.above = (self.nodes[:, 1] >> 2).astype(np.int64)      # interior: the above child; leaf: its reference count

    def leaf_has(self, n_prims):
        """bool [n_nodes, n_prims]: the primitives a leaf references."""
        has = np.zeros((self.n_nodes, max(1, n_prims)), bool)
        for k in np.nonzero(self.axis == 3)[0]:
            has[k, self.refs[int(self.nodes[k, 0]): int(self.nodes[k, 0]) + int(self.above[k])]] = True
        return has


def walk(tree, rays, n_prims, accepted=None, stop_t=None):
    """The walk of every ray (rays [n, 6] f32), all rays stepping together.  accepted [n]: the primitive of the ray's accepted
    hit (-1: none; from gm.ray_cast, never from here).  stop_t [n]: the ray parameter of that hit (inf: none) - the walk ends,
    as the closest-hit walkers do, at the first popped segment that starts behind it (without the walkers' slack: the model
    stops no later than they do, so its heights are floors of theirs).  -> dict of [n] arrays:
      height       the highest number of pending far children
      hit_height   the height the stack had when the entry was popped that led to the first visited leaf referencing
                   `accepted` (0: that leaf was reached without a pop; -1: no such leaf visited) - the popped entry is the one
                   at index hit_height - 1
      visits       nodes visited."""
    rays = np.ascontiguousarray(rays, F32).reshape(-1, 6)
    n = len(rays)
    o, d = rays[:, :3], rays[:, 3:]
    has = tree.leaf_has(n_prims)
    accepted = np.full(n, -1, np.int64) if accepted is None else np.asarray(accepted, np.int64)
    stop_t = np.full(n, np.inf, F32) if stop_t is None else np.asarray(stop_t, F32)
    REL, ABS = F32(1.00001), F32(1e-6)
    with np.errstate(all="ignore"):
        inv = F32(1) / d
        t0, t1 = (tree.bmin[None] - o) * inv, (tree.bmax[None] - o) * inv
        swap = t0 > t1
        tn, tf = np.where(swap, t1, t0), np.where(swap, t0, t1)
        tmin, tmax = np.zeros(n, F32), np.full(n, np.inf, F32)
        for a in range(3):
            tmin = np.where(tn[:, a] > tmin, tn[:, a], tmin)
            tmax = np.where(tf[:, a] < tmax, tf[:, a], tmax)
        alive = ~(tmin > tmax * F32(1.0001) + F32(1e-4)) & (tree.n_nodes > 0)
        node = np.zeros(n, np.int64)
        sp = np.zeros(n, np.int64)
        st_node = np.zeros((n, PT_KD_STACK + 2), np.int64)
        st_tmax = np.zeros((n, PT_KD_STACK + 2), F32)
        height, visits = np.zeros(n, np.int64), np.zeros(n, np.int64)
        popped_from, hit_height = np.zeros(n, np.int64), np.full(n, -1, np.int64)
        while alive.any():
            i = np.nonzero(alive)[0]
            k = node[i]
            visits[i] += 1
            ax = tree.axis[k]
            inner = ax != 3
            # ---- interior nodes
            j, kj, axj = i[inner], k[inner], ax[inner]
            if len(j):
                split = tree.split[kj]
                oa, da, ia = o[j, axj], d[j, axj], inv[j, axj]
                tp = (split - oa) * ia
                below_first = (oa < split) | ((oa == split) & (da <= 0))
                below, above = kj + 1, tree.above[kj]
                first, second = np.where(below_first, below, above), np.where(below_first, above, below)
                only_first = (tp > tmax[j] * REL + ABS) | (tp <= 0)
                only_second = ~only_first & (tp < tmin[j] * (F32(2) - REL) - ABS)
                both = ~(only_first | only_second)
                jb = j[both]
                assert (sp[jb] <= PT_KD_STACK).all(), "the model's stack is deeper than PT_KD_STACK"
                st_node[jb, sp[jb]] = second[both]
                st_tmax[jb, sp[jb]] = tmax[jb]
                sp[jb] += 1
                height[jb] = np.maximum(height[jb], sp[jb])
                tmax[jb] = tp[both]
                node[j] = np.where(only_second, second, first)
            # ---- leaves
            j, kj = i[~inner], k[~inner]
            if len(j):
                acc = accepted[j]
                found = (acc >= 0) & (hit_height[j] < 0) & has[kj, np.maximum(acc, 0)]
                hit_height[j[found]] = popped_from[j[found]]
                empty = sp[j] == 0
                alive[j[empty]] = False
                j = j[~empty]
                popped_from[j] = sp[j]
                sp[j] -= 1
                tmin[j] = tmax[j]
                node[j] = st_node[j, sp[j]]
                tmax[j] = st_tmax[j, sp[j]]
                alive[j[tmin[j] > stop_t[j]]] = False
    return dict(height=height, hit_height=hit_height, visits=visits)


def stop_parameters(rays, first_hits, gm):
    """The ray parameter of each ray's accepted hit (records [n] of gm.HIT_DTYPE: the first of gm.ray_cast's list): a triangle's
    dist is the parameter itself, a sphere's is a length, |d| times the parameter.  inf where there is no hit."""
    rays = np.ascontiguousarray(rays, F32).reshape(-1, 6)
    dlen = np.sqrt((rays[:, 3:].astype(np.float64) ** 2).sum(axis=1))
    t = np.where((first_hits["flags"] & gm.FLAG_SPHERE) != 0, first_hits["dist"] / np.maximum(dlen, 1e-300), first_hits["dist"])
    return np.where(first_hits["prim"] >= 0, t, np.inf).astype(F32)


def home_depths(tree, models, camera_position):
    """Per primitive the depth of its HOME NODE, as the comment above prep_entry_lists (csrc/pt_gpu.hip) defines it: the deepest
    node whose box holds every origin a hit on the primitive can produce - its bounds pushed 1.05e-5 along the normals (a
    sphere: the radius grown by that) and by eps = 2.5e-7 x the largest coordinate of the tree's bounds or the camera.  The
    descent stops at a leaf, at a plane the padded box straddles or touches, and at depth ENTRY_LIST_CAP.  That depth is the
    length of the primitive's entry list.  models: the geometry_model form, normals flat (tests/test_geometry_model.py built)."""
    ext = max(float(np.abs(tree.bmin).max()), float(np.abs(tree.bmax).max()), float(np.abs(np.asarray(camera_position)).max()))
    eps = F32(2.5e-7 * max(ext, 1e-3))
    k105 = F32(1.05e-5)
    lo, hi = [], []
    for m in models:
        if m[0] == "mesh":
            t = np.asarray(m[1], F32).reshape(-1, 3, 3)
            t64 = t.astype(np.float64)
            nrm = np.cross(t64[:, 1] - t64[:, 0], t64[:, 2] - t64[:, 0])
            nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(F32)
            lo.append(t.min(axis=1) + k105 * nrm - eps)     # (flat normals: the three vertex normals are the same)
            hi.append(t.max(axis=1) + k105 * nrm + eps)
        else:
            c, r = np.asarray(m[1], F32), F32(m[2])
            lo.append((c - r - k105 - eps)[None])
            hi.append((c + r + k105 + eps)[None])
    lo, hi = np.concatenate(lo).astype(F32), np.concatenate(hi).astype(F32)
    out = np.zeros(len(lo), np.int64)
    for p in range(len(lo)):
        node, depth = 0, 0
        while tree.n_nodes and tree.axis[node] != 3 and depth < ENTRY_LIST_CAP and np.isfinite(lo[p, 0]) and np.isfinite(hi[p, 0]):
            a, s = tree.axis[node], tree.split[node]
            if hi[p, a] < s:
                node = node + 1
            elif lo[p, a] > s:
                node = int(tree.above[node])
            else:
                break
            depth += 1
        out[p] = depth
    return out


def check_structure(tree, n_prims):
    """The structure checks of test_kd_tree_structure_and_coverage: DFS layout, every child index valid, every leaf range
    valid, every primitive referenced, the depth within the walkers' stacks."""
    nodes = tree.nodes
    interior = tree.axis != 3
    assert tree.n_nodes == len(nodes) and interior.sum() + tree.n_leaves == len(nodes)
    above = tree.above[interior]
    assert (above > np.nonzero(interior)[0] + 1).all() and (above < len(nodes)).all()
    leaf = ~interior
    assert ((nodes[leaf, 0].astype(np.int64) + tree.above[leaf]) <= tree.n_refs).all()
    assert set(tree.refs.tolist()) == set(range(n_prims))
    assert tree.depth < PT_KD_STACK
    # (the depth the builder reports is the deepest leaf's)
    depth = np.zeros(len(nodes), np.int64)
    for k in np.nonzero(interior)[0]:
        depth[k + 1] = depth[tree.above[k]] = depth[k] + 1
    assert len(nodes) == 0 or int(depth.max()) == tree.depth
    return depth
