// Origin grids on the device: ray casts for rays through one point (host/origin_grid.cpp builds them).
//
// The reference filters every ray_cast() (renderer/utils.rs:11-21) through kdtree-ray.  Camera rays
// (renderer/mod.rs:114-124: every sample of every pixel starts at camera column 3) and the shadow rays of a
// point light (renderer/mod.rs:301-331: they all pass within 1e-5 |n| of the light) are looked up here instead:
// the ray's direction selects ONE cell of a cube map around the common point, and the cell's list - sorted by
// distance from that point, conservative by construction - holds every primitive the ray can hit.  One table
// lookup and a few Möller–Trumbore tests that neighbouring lanes share, instead of ~20 dependent node fetches at
// ~44 scattered addresses per wavefront; the arithmetic of the accepted hit is the same instruction sequence.
//
// This header holds the lookups; the kernels that use them are k_wf_shade (pt_wavefront.h: camera cast and
// shadow casts inline) and k_og_primary / k_og_shadow / k_og_shadow_offgrid (pt_grid_kernels.h).
#pragma once
#include "pt_integrator.h"

// Cell of direction w (host mirror: path-tracer_amd/__init__.py OriginGrid.cells, tests/test_origin_grid.py).
PT_D void og_cell_coords(const DevGrid& G, f3 w, uint32_t& face, uint32_t& cu_out, uint32_t& cv_out) {
    const float ax = fabsf(w.x), ay = fabsf(w.y), az = fabsf(w.z);
    const bool fx = ax >= ay && ax >= az, fy = !fx && ay >= az;
    const float wa = fx ? w.x : (fy ? w.y : w.z);
    const float wb = fx ? w.y : (fy ? w.z : w.x);
    const float wc = fx ? w.z : (fy ? w.x : w.y);
    const float inv = 1.0f / fabsf(wa);
    const float fu = (wb * inv + 1.0f) * G.half_res, fv = (wc * inv + 1.0f) * G.half_res;
    const float top = (float)(G.res - 1u);
    const float cu = fu >= 0.f ? fminf(floorf(fu), top) : 0.f;   // (NaN -> cell 0: such a ray hits nothing anyway)
    const float cv = fv >= 0.f ? fminf(floorf(fv), top) : 0.f;
    face = (fx ? 0u : (fy ? 2u : 4u)) + (wa < 0.f ? 1u : 0u);
    cu_out = (uint32_t)cu;
    cv_out = (uint32_t)cv;
}
PT_D uint32_t og_cell(const DevGrid& G, f3 w) {
    uint32_t face, cu, cv;
    og_cell_coords(G, w, face, cu, cv);
    return (face * G.res + cv) * G.res + cu;
}

// Orthographic grid: cell of the ray ORIGIN p (host mirror: OriginGrid.cells), and the scan limit -depth(p).
PT_D uint32_t og_cell_ortho(const DevGrid& G, f3 p) {
    const float fu = (dot3(p, ld3(G.axis_u)) - G.u0) * G.cells_per_unit, fv = (dot3(p, ld3(G.axis_v)) - G.v0) * G.cells_per_unit;
    const float top = (float)(G.res - 1u);
    const float cu = fu >= 0.f ? fminf(floorf(fu), top) : 0.f;
    const float cv = fv >= 0.f ? fminf(floorf(fv), top) : 0.f;
    return (uint32_t)cv * G.res + (uint32_t)cu;
}

// Candidate update with one primitive record (v0 | id, e1 | e2.x, e2.yz): the acceptance rule of next_hit().
template <bool COUNT>
PT_D void og_test_closest(f3 o, f3 d, float4 q0, float4 q1, float4 q2, float t_prev, uint32_t ord_prev, RawHit& best,
                          LocalCtr& lc) {
    const uint32_t pid = __float_as_uint(q0.w);
    if (COUNT) lc.tris++;
    if (!(pid & PT_PRIM_SPHERE)) {
        float dist, u, v;
        bool bf;
        if (!isect_triangle(o, d, mk3(q0.x, q0.y, q0.z), mk3(q1.x, q1.y, q1.z), mk3(q1.w, q2.x, q2.y), dist, u, v, bf)) return;
        const uint32_t ord = PT_PRIM_INDEX(pid) * 2u;
        if (key_less(t_prev, ord_prev, dist, ord) && key_less(dist, ord, best.key, best.ord)) {
            best.key = dist;
            best.ord = ord;
            best.pid = pid;
            best.u = u;
            best.v = v;
            best.flags = bf ? 1u : 0u;
        }
    } else {
        float t[2], key[2];
        bool ex[2];
        const int nh = isect_sphere(o, d, mk3(q0.x, q0.y, q0.z), q1.x, t, key, ex);
        for (int k = 0; k < nh; ++k) {
            const uint32_t ord = PT_PRIM_INDEX(pid) * 2u + (ex[k] ? 1u : 0u);
            if (key[k] == key[k] && key_less(t_prev, ord_prev, key[k], ord) && key_less(key[k], ord, best.key, best.ord)) {
                best.key = key[k];
                best.ord = ord;
                best.pid = pid;
                best.u = t[k];
                best.v = 0.f;
                best.flags = 2u | (ex[k] ? 4u : 0u);
            }
        }
    }
}

// The entry of ray_cast()'s sorted list that follows (t_prev, ord_prev), among the candidates of `cell`.
// Rays that START at the grid's origin (camera): kmax >= max(1, |d|) (with rounding slack) - a primitive whose
// distance bound exceeds best.key * kmax cannot give a smaller key (triangle keys are ray parameters, sphere keys
// Euclidean distances).  Rays that END there (shadow rays) pass kmax = INFINITY: their keys grow towards the
// FRONT of the list, every candidate up to `cutoff` (the distance of the ray's start from the origin) is tested.
template <bool COUNT>
PT_D bool og_next_hit(const DevScene& S, const DevGrid& G, uint32_t cell, f3 o, f3 d, float kmax, float cutoff,
                      float t_prev, uint32_t ord_prev, RawHit& best, LocalCtr& lc) {
    best.key = INFINITY;
    best.ord = 0xffffffffu;
    best.pid = 0xffffffffu;
    for (uint32_t k = 0; k < G.n_global; ++k) {
        const float4* pp = S.prim_pos + (size_t)(G.refs[k].x & ~PT_PRIM_SPHERE) * 3;
        og_test_closest<COUNT>(o, d, pp[0], pp[1], pp[2], t_prev, ord_prev, best, lc);
    }
    const uint32_t first = G.cell_off[cell], last = G.cell_off[cell + 1u];   // (one entry more than cells)
    for (uint32_t k = first; k < last; ++k) {
        const uint2 r = G.refs[k];
        const float m = __uint_as_float(r.y);
        if (m > cutoff || m > best.key * kmax) break;
        const float4* pp = S.prim_pos + (size_t)(r.x & ~PT_PRIM_SPHERE) * 3;
        og_test_closest<COUNT>(o, d, pp[0], pp[1], pp[2], t_prev, ord_prev, best, lc);
    }
    // kdtree-ray's box test (scene_slab): a ray it rejects has no hits at all
    if (best.pid != 0xffffffffu && !hit_passes_slab(S, o, d)) best.pid = 0xffffffffu;
    return best.pid != 0xffffffffu;
}

// Opaque scenes: is there any hit - RANGED (point light): with |hit - pos| <= ldist (mod.rs:319-321 with every
// opacity exactly 1); otherwise (directional light, mod.rs:291-297) any hit at all?  `ldist` is also the scan limit
// of the list (point light: distance surface - light; directional: minus the depth of the ray's origin).
template <bool COUNT, bool RANGED>
PT_D uint32_t og_blocker(const DevScene& S, const DevGrid& G, uint32_t cell, f3 so, f3 sd, f3 pos, float ldist, LocalCtr& lc) {
    const uint32_t first = G.cell_off[cell], last = G.cell_off[cell + 1u];
    const uint32_t n_all = G.n_global + (last - first);
    for (uint32_t j = 0; j < n_all; ++j) {
        const uint32_t k = j < G.n_global ? j : first + (j - G.n_global);
        const uint2 r = G.refs[k];
        if (j >= G.n_global && __uint_as_float(r.y) > ldist) break;
        const float4* pp = S.prim_pos + (size_t)(r.x & ~PT_PRIM_SPHERE) * 3;
        const float4 q0 = pp[0], q1 = pp[1], q2 = pp[2];
        if (COUNT) lc.tris++;
        if (!(r.x & PT_PRIM_SPHERE)) {
            float t, u, v;
            bool bf;
            if (!isect_triangle(so, sd, mk3(q0.x, q0.y, q0.z), mk3(q1.x, q1.y, q1.z), mk3(q1.w, q2.x, q2.y), t, u, v, bf))
                continue;
            if (RANGED && mag3((so + sd * t) - pos) > ldist) continue;
            return __float_as_uint(q0.w);
        } else {
            float t[2], key[2];
            bool ex[2];
            const int nh = isect_sphere(so, sd, mk3(q0.x, q0.y, q0.z), q1.x, t, key, ex);
            for (int h = 0; h < nh; ++h) {
                if (!(key[h] == key[h])) continue;
                if (RANGED && mag3((so + sd * t[h]) - pos) > ldist) continue;
                return __float_as_uint(q0.w);
            }
        }
    }
    return 0xffffffffu;
}
// (the id word of the first occluder found, 0xffffffff = none; kdtree-ray's box test once, after the scan: a ray the
// scene box rejects has no hits at all)
template <bool COUNT, bool RANGED>
PT_D bool og_blocked(const DevScene& S, const DevGrid& G, uint32_t cell, f3 so, f3 sd, f3 pos, float ldist, LocalCtr& lc) {
    const uint32_t pid = og_blocker<COUNT, RANGED>(S, G, cell, so, sd, pos, ldist, lc);
    return pid != 0xffffffffu && hit_passes_slab(S, so, sd);
}


// get_light_info (mod.rs:281-333) for light `li` through its grid: the radiance that reaches the surface (pos,
// normal gn, uv, kind).  Point light: cube map around the light, looked up with (pos - light); the caller has checked
// that |gn| is within the grid's margin.  Directional light: orthographic grid, looked up with the ray's origin.
// DIRL: the scene has directional lights (a compile-time switch: the orthographic branch compiled into the fused
// bounce-0 kernel costs it 112 B more scratch per lane and 3.5 ms on config 3, which has none).
template <bool ALPHA, bool COUNT, bool DIRL>
PT_D f3 og_light_radiance(const DevScene& S, uint32_t li, f3 pos, f3 gn, f2 uv, bool sphere, LocalCtr& lc) {
    const DevLight& L = S.lights[li];
    const DevGrid& G = S.light_grids[li];
    const f3 so = pos + gn * 0.00001f;   // NORMAL_BIAS (mod.rs:58)
    if (COUNT) lc.shadow_rays++;
    if (DIRL && L.kind != PT_LIGHT_POINT) {   // mod.rs:283-299: every hit of the whole ray counts, sampled at ITS surface
        const f3 sd = -1.f * ld3(L.vec);
        f3 rad = ld3(L.color);
        const uint32_t cell = og_cell_ortho(G, so);
        const float limit = -dot3(so, ld3(G.axis_w));
        if (!ALPHA) {
            if (og_blocked<COUNT, false>(S, G, cell, so, sd, pos, limit, lc)) rad = rad * 0.0f;
            return rad;
        }
        float t_prev = -INFINITY;
        uint32_t ord_prev = 0;
        RawHit h;
        bool first = true;
        while (og_next_hit<COUNT>(S, G, cell, so, sd, INFINITY, limit, t_prev, ord_prev, h, lc)) {
            if (COUNT && !first) lc.restarts++;
            first = false;
            rad = rad * (1.f - hit_opacity(S, so, sd, h));
            if (sum3(rad) == 0.f) break;
            t_prev = h.key;
            ord_prev = h.ord;
        }
        return rad;
    }
    f3 direction = pos - ld3(L.vec);
    const uint32_t cell = og_cell(G, direction);
    const float ldist = mag3(direction);
    direction = normalize3(direction);
    f3 rad = ld3(L.color) / (4.f * PT_PI * ldist * ldist);
    const f3 sd = -1.f * direction;
    if (!ALPHA) {
        if (og_blocked<COUNT, true>(S, G, cell, so, sd, pos, ldist, lc)) rad = rad * 0.0f;
        return rad;
    }
    // walk the sorted list, attenuating by (1 - opacity) (mod.rs:319-329)
    float t_prev = -INFINITY;
    uint32_t ord_prev = 0;
    RawHit h;
    bool first = true;
    while (og_next_hit<COUNT>(S, G, cell, so, sd, INFINITY, ldist, t_prev, ord_prev, h, lc)) {
        if (COUNT && !first) lc.restarts++;
        first = false;
        const f3 sp = so + sd * ((h.flags & 2u) ? h.u : h.key);
        if (mag3(sp - pos) > ldist) break;
        // the SHADED hit's kind / uv with the occluder's material (mod.rs:324)
        const uint32_t smodel = __float_as_uint(S.prim_attr[(size_t)PT_PRIM_INDEX(h.pid) * 4 + 3].w);
        rad = rad * (1.f - material_opacity(S, smodel, sphere, uv));
        if (sum3(rad) == 0.f) break;
        t_prev = h.key;
        ord_prev = h.ord;
    }
    return rad;
}

// og_light_radiance of an OPAQUE scene in its two halves, for the caller that keeps the visibility (the shadow-visibility
// cache of the bounce-0 kernel, pt_wavefront.h VIS): the radiance before the visibility factor - the expressions of
// og_light_radiance, operand for operand - and the cast whose answer is that factor.  rad * 0.0f where blocked stays the
// caller's, as there.
template <bool DIRL>
PT_D f3 og_light_unshadowed(const DevScene& S, uint32_t li, f3 pos) {
    const DevLight& L = S.lights[li];
    if (DIRL && L.kind != PT_LIGHT_POINT) return ld3(L.color);
    const f3 direction = pos - ld3(L.vec);
    const float ldist = mag3(direction);
    return ld3(L.color) / (4.f * PT_PI * ldist * ldist);
}
template <bool DIRL>
PT_D bool og_light_blocked(const DevScene& S, uint32_t li, f3 pos, f3 gn, LocalCtr& lc) {
    const DevLight& L = S.lights[li];
    const DevGrid& G = S.light_grids[li];
    const f3 so = pos + gn * 0.00001f;   // NORMAL_BIAS (mod.rs:58)
    if (DIRL && L.kind != PT_LIGHT_POINT) {
        const f3 sd = -1.f * ld3(L.vec);
        const uint32_t cell = og_cell_ortho(G, so);
        const float limit = -dot3(so, ld3(G.axis_w));
        return og_blocked<false, false>(S, G, cell, so, sd, pos, limit, lc);
    }
    f3 direction = pos - ld3(L.vec);
    const uint32_t cell = og_cell(G, direction);
    const float ldist = mag3(direction);
    direction = normalize3(direction);
    const f3 sd = -1.f * direction;
    return og_blocked<false, true>(S, G, cell, so, sd, pos, ldist, lc);
}
