// The body of k_wf_shade and of k_wf_shade_hits (pt_wavefront.h), included inside both kernels: a function the two call would
// be the plainer form, but inlined it compiles the existing variants to other code than the kernel's own text does (scratch
// of eight variants moved by 4-8 B; profiles/r09_experiments.txt item 0), and those variants are tuned to the byte.
// In scope: the template parameters ALPHA, COUNT, PRIMARY, GRIDX (bits SB_*; constants in k_wf_shade_hits) and the kernel's
// parameters - S, W, tile_offsets, queue_in, hits, rng_planes, draws, queue_out, shadow_q, contrib, staging, index_list,
// exact_list, chunk_hits, exact_next, block_empty, ctr, gctr - and hit_plane, vis_plane, next_plane, next_hits, next_ctr,
// cont_plane, cont_stride, cont_flags.
    // index_list (bounces >= 1): null - the whole queue, entries marked WF_HIT_PENDING left out; else the entries to shade:
    // the hand-over list of k_wf_trace, whose casts k_wf_trace_wide has finished by now - `hits` is then that list's
    // own plane (W.list_cap records, by list position).  The pass over the queue runs WHILE k_wf_trace_wide walks
    // those few long casts (WF_WIDE_LANES = 32 lanes each, a launch bound by its longest cast).  Behind that list, in the same launch, the
    // exact list (k_wf_trace_exact, pt_wavefront.h wf_exact_words): word by list position, the rest of the hit in the chunk's
    // own plane (chunk_hits) at the queue index.  exact_next: the exact list of the NEXT bounce - a survivor whose new ray the
    // wavefront walker will not take (slack_is_capped) is listed here, where the ray is made, so that k_wf_trace_exact can
    // walk it while k_wf_trace is busy with the rest of the queue.
    constexpr int GRID = GRIDX & SB_GRID_MASK;
    constexpr bool DIRL = (GRIDX & SB_DIRL) != 0;
    constexpr bool CACHED = (GRIDX & SB_CACHED) != 0;
    constexpr bool STORE = (GRIDX & SB_STORE) != 0, LOAD = (GRIDX & SB_LOAD) != 0;
    static_assert(GRIDX != SB_DIRL, "DIRL needs a grid mode");
    static_assert(!(STORE || LOAD) || (CACHED && !ALPHA && !COUNT && PRIMARY), "the camera-hit cache serves the cached opaque bounce-0 kernel");
    static_assert(!(STORE && LOAD), "a launch stores the camera hits or loads them");
    constexpr bool VIS = (GRIDX & SB_VIS) != 0;
    static_assert(!VIS || LOAD, "the shadow-visibility cache serves the launches that load their camera hits");
    // NEXT: the launch reads the bounce-1 hit cache as well (next_plane: the chunk's records there) - a survivor whose record
    // says miss and whose colour is final ends here, the others get the word and the hit k_wf_hits_load would have copied
    constexpr bool NEXT = (GRIDX & SB_NEXT) != 0;
    static_assert(!NEXT || (LOAD && VIS), "the bounce-1 hits are consumed by the launches that load camera hits and visibility");
    static_assert(!CACHED || (GRID == 3 && !COUNT), "the word cache serves the fused bounce-0 kernel");
    // VIS1, NEXT1 (k_wf_shade_fused: the opaque bounce-1 pass of a scene without the orthographic branch).  VIS1: the launch reads
    // the bounce-1 shadow-visibility bytes (vis_plane, by out_slot, never written here) - a hit whose live lights all have
    // known bits gets them added here, in light order, with the operands of k_og_shadow_vis, and writes no shadow record;
    // any other goes to the shadow queue whole.  NEXT1: the launch reads the bounce-2 hit cache as well (next_plane, by item),
    // as NEXT does one bounce earlier.
    constexpr bool VIS1 = (GRIDX & SB_VIS1) != 0, NEXT1 = (GRIDX & SB_NEXT1) != 0;
    static_assert(!VIS1 || ((GRIDX & (SB_VIS1 - 1)) == 0 && !ALPHA && !COUNT && !PRIMARY), "the bounce-1 visibility is read by the plain opaque later-bounce pass");
    static_assert(!NEXT1 || VIS1, "the bounce-2 hits are consumed by the launch that adds the lights itself");
    // CONT_STORE, CONT_LOAD (k_wf_shade_hits: the scene's cache of bounce-0 continuations, pt_gpu.hip FrameCache cont_cache;
    // cont_plane points at the chunk's first item of plane 0, plane 1 lies cont_stride records behind it).  Plane 0: the raw
    // bits of next_d and a state word (0: never written - the planes are zeroed when they are keyed; bit 0: written; bit 1:
    // escape_proves_miss was evaluated for the item with the masks that existed then; bit 2: its answer), plane 1: the raw bits of next_thr.  CONT_STORE: every hit lane writes
    // its two records behind ct_eval_indirect.  CONT_LOAD: the records are read at the top of the step, beside cam_rec, vis
    // and next_rec, and the launch contains no ct_sample, no ct_eval_indirect and no use of words 2 and 3.
    constexpr bool CONT_STORE = (GRIDX & SB_CONT_STORE) != 0, CONT_LOAD = (GRIDX & SB_CONT_LOAD) != 0;
    static_assert(!CONT_STORE || ((STORE || (LOAD && VIS)) && !NEXT), "the continuation is stored by the launch that runs while the bounce-1 hits are stored");
    static_assert(!CONT_LOAD || NEXT, "the continuation is loaded by the launches that read the bounce-1 hits themselves");
    static_assert(!(CONT_STORE && CONT_LOAD), "a launch stores the continuation or loads it");
    // LEAN (k_wf_shade_hits<.. | SB_LEAN>, 6379: the steady frame of a scene without the orthographic branch).  A frame whose caches
    // answer everything makes no shadow cast, runs no escape test and writes no shadow record: this variant contains none of
    // that - no og_light_blocked, no parking, no escape_proves_miss, no shadow-queue stores - and so needs neither the
    // registers nor the LDS that hold the general variant at four waves per SIMD.  The host launches it only for a
    // configuration whose last counted frame met no such lane (pt_gpu.hip, "lean"); a lane that would need any of it all the
    // same - a COLD lane - writes nothing and raises bit 1 of ctr[0].overflow, which fails the configuration's next call.
    // The records that are consumed behind the lights only (next_rec, cont_d, cont_thr: 48 of the step's 81 dense bytes per
    // item) are fetched at the top of the step, as in the general variant, but wait in LDS, not in registers (sh_late).
    constexpr bool LEAN = (GRIDX & SB_LEAN) != 0;
    static_assert(!LEAN || (CONT_LOAD && !DIRL && PRIMARY), "the lean variant is a loading bounce-0 launch without the orthographic branch");
    // LEAN1 (k_wf_shade_fused<SB_VIS1 | SB_LEAN1>, 8448: bounces 1 and 2 of a steady frame).  A frame whose visibility bytes are all known
    // writes no shadow record at these bounces, sorts nothing, lists no ray for k_wf_trace_exact, plays no roulette and draws
    // words 4-7 of the staged plane only: this variant contains none of the rest - no shadow or contribution record with its
    // second lights loop, no second colour (a known light is added to `color` at once, with the operands `lit` receives in the
    // general variant), no sorting option, no exact_shade_lists branch, no ChaCha block - and so runs at WF_SHADE_LEAN1_WAVES
    // waves per SIMD.  A lane that needs any of it - a live light of unknown visibility, a normal too long for the grids, a
    // draw beyond the staged words: a COLD lane - writes nothing and counts nothing; it appends its queue index to the
    // hand-over list (one wf_reserve per wave on the list's own counter), and a launch of HAND, the general body over exactly
    // those entries, follows on the same stream and shades the record whole.
    // The list (`index_list` of both launches; the lean one writes it): sixteen count words by bounce, zeroed once per chunk,
    // then the queue indices - as long as the bounce's queue, so it cannot overflow.  HAND reads the word and the hit of an
    // entry from the chunk's own planes at the queue index.
    constexpr bool LEAN1 = (GRIDX & SB_LEAN1) != 0, HAND = (GRIDX & SB_HAND) != 0;
    static_assert(!(LEAN1 || HAND) || (VIS1 && !NEXT1), "the lean later-bounce variant and its list pass read the visibility bytes alone");
    static_assert(!(LEAN1 && HAND), "a launch hands over or shades what was handed over");
    uint32_t* const handover = (LEAN1 || HAND) ? const_cast<uint32_t*>(index_list) : nullptr;
    uint4* rng_planes_out = const_cast<uint4*>(rng_planes);   // GRID == 3 writes plane 1 (nobody reads it before bounce 1)
    static_assert(GRID < 2 || PRIMARY, "the camera grid serves bounce 0");
    const bool list_pass = !PRIMARY && !LEAN1 && index_list != nullptr;
    const uint32_t n_def = HAND ? min(handover[W.bounce], W.qcap_in) : list_pass ? ctr[W.bounce].deferred_count : 0u;
    // (HAND: the hand-over list alone - the bounce's exact list was shaded with the queue, by the launch that handed over)
    const uint32_t n = PRIMARY ? W.n_items : list_pass ? n_def + ((!HAND && exact_list) ? min(ctr[W.bounce].exact_count, W.ecap) : 0u) : min(ctr[W.bounce].queue_count, W.qcap_in);
    // entry e of this launch: its queue record, the word of its hit, the hit
    auto entry_index = [&](uint32_t e) -> uint32_t {
        if constexpr (HAND) return handover[WF_HANDOVER_HEAD + e];
        return !list_pass ? e : e < n_def ? index_list[e] : exact_list[e - n_def];
    };
    auto entry_word = [&](uint32_t e) -> uint32_t {
        if constexpr (HAND) return wf_hit_word(hits, handover[WF_HANDOVER_HEAD + e]);
        return (!list_pass || e < n_def) ? wf_hit_word(hits, e) : wf_exact_words(exact_list, W.ecap)[e - n_def];
    };
    auto entry_hit = [&](uint32_t e, uint32_t i, RawHit& h) -> bool {
        if constexpr (HAND) return wf_load_hit(hits, W.hcap, i, h);
        if (!list_pass) return wf_load_hit(hits, W.hcap, e, h);
        if (e < n_def) return wf_load_hit(hits, W.list_cap, e, h);
        const uint32_t x = wf_exact_words(exact_list, W.ecap)[e - n_def];
        if (x == 0xffffffffu) return false;
        const uint4 k = ((const uint4*)((const uint32_t*)chunk_hits + W.hcap))[i];
        return unpack_hit(make_uint4(x, k.x, k.y, k.z), h);
    };
    uint32_t n_draws = 0, n_new = 0, n_moot = 0, n_hits = 0, n_cam_tris = 0, n_masked = 0;
    LocalCtr lc = {0, 0, 0, 0, 0, 0};   // (GRID: casts made here)
    // (NEXT: [2] the elided of a step; [3][0], [3][2] what threads 0 and 2 counted over the launch's steps - records written,
    // records elided -, each its own thread's word, added to the device's counters once, at the end: an atomic per step
    // would stand, with its round trip, in front of the compaction's barrier)
    __shared__ uint32_t sh_cnt[NEXT ? 4 : 2][WF_SHADE_THREADS / 64];
    if (NEXT && threadIdx.x < WF_SHADE_THREADS / 64) sh_cnt[NEXT ? 3 : 0][threadIdx.x] = 0u;
    // ([3][1], the general loading variants: set by any lane that casts for a light of unknown visibility - a word other
    // threads write, so its zero must be there before the first of them can get that far)
    if constexpr (CONT_LOAD && !LEAN) __syncthreads();
    __shared__ uint32_t sh_base[2];
    __shared__ uint32_t sh_oct[8][WF_SHADE_THREADS / 64], sh_oct_off[8][WF_SHADE_THREADS / 64];
    // (VIS1: what threads 0-3 counted over the launch's steps, each its own word - next-bounce records written, shadow records
    // written, survivors ended or elided here, records whose lights were added here -, added to the device's counters once,
    // at the end.  The kernel has no LDS to spare and a register more is scratch: the words are sh_oct_off's last row, which
    // only the sorting options write - render_chunk takes this kernel for unsorted frames, PT_WF_SORT=0, only.)
    uint32_t* const fused_acc = &sh_oct_off[7][0];
    if (VIS1 && threadIdx.x < WF_SHADE_THREADS / 64) fused_acc[threadIdx.x] = 0u;
    const uint32_t wave = threadIdx.x >> 6;
    // LDS parking (PARK: the cached opaque bounce-0 variant at four waves per SIMD): per-lane state that is cold across an
    // inline shadow cast waits in LDS, slot-major (sh_park[slot][thread]: conflict-free dwords, every slot private to its
    // thread - no barrier).  The accesses are volatile: a plain store would be forwarded to its load and the register kept.
    constexpr bool PARK = CACHED && !ALPHA && WF_SHADE_PARK;
    // (wf_opaque_arg reads S at offset 0 of the kernarg segment and W right behind it: the kernels below check that)
    __shared__ uint32_t sh_park[(PARK && !LEAN) ? WF_PARK_SLOTS + (VIS ? 1u : 0u) + (NEXT ? 4u : 0u) : 1][WF_SHADE_THREADS];   // (VIS: + PK_VIS; NEXT: + PK_NEXT)
    // (LEAN) the late records of the step, [plane][thread]: 0 next_rec, 1 cont_d, 2 cont_thr - every slot private to its thread,
    // so no barrier; volatile, as the parking slots are: a plain store would be forwarded to its load and the registers kept
    typedef uint32_t WfLateRec __attribute__((ext_vector_type(4)));
    __shared__ WfLateRec sh_late[LEAN ? 3 : 1][LEAN ? WF_SHADE_THREADS : 1];
    volatile __attribute__((address_space(3))) WfLateRec* const late = (volatile __attribute__((address_space(3))) WfLateRec*)&sh_late[0][LEAN ? threadIdx.x : 0u];
    auto late_get = [&](uint32_t plane) -> uint4 { const WfLateRec v = late[plane * WF_SHADE_THREADS]; return make_uint4(v.x, v.y, v.z, v.w); };
    // (an LDS pointer by type: a volatile access through a generic pointer stays a flat access, one 64-bit address per slot)
    volatile __attribute__((address_space(3))) uint32_t* const park = (volatile __attribute__((address_space(3))) uint32_t*)&sh_park[0][threadIdx.x];
    auto park_u = [&](uint32_t slot, uint32_t v) { park[slot * WF_SHADE_THREADS] = v; };
    auto park_f = [&](uint32_t slot, float v) { park[slot * WF_SHADE_THREADS] = __float_as_uint(v); };
    auto park_3 = [&](uint32_t slot, f3 v) { park_f(slot, v.x), park_f(slot + 1u, v.y), park_f(slot + 2u, v.z); };
    auto unpark_u = [&](uint32_t slot) -> uint32_t { return park[slot * WF_SHADE_THREADS]; };
    auto unpark_f = [&](uint32_t slot) -> float { return __uint_as_float(park[slot * WF_SHADE_THREADS]); };
    auto unpark_3 = [&](uint32_t slot) -> f3 { const float x = unpark_f(slot), y = unpark_f(slot + 1u); return mk3(x, y, unpark_f(slot + 2u)); };
    // (LEAN1) what the BRDF sample does not touch - out_slot, item, the colour, final by then, the new ray's origin and the
    // primitive - waits in LDS across ct_sample and ct_eval_indirect, [slot][thread]: every slot private to its thread, so no
    // barrier; volatile, as the slots above are.  These nine registers are what stands between the variant and
    // WF_SHADE_LEAN1_WAVES waves without scratch (the first five alone: 12 B, profiles/r22_experiments.txt item 1).
    constexpr uint32_t PARK1_SLOTS = 9u;
    __shared__ uint32_t sh_park1[LEAN1 ? PARK1_SLOTS : 1][LEAN1 ? WF_SHADE_THREADS : 1];
    volatile __attribute__((address_space(3))) uint32_t* const park1 = (volatile __attribute__((address_space(3))) uint32_t*)&sh_park1[0][LEAN1 ? threadIdx.x : 0u];
    // (Bounce 0 needs no hit aggregation like the later bounces' below: a wavefront is one 8x8 pixel block of one sample,
    // so its camera rays hit or miss together - collecting the hits of 256 items in LDS and shading them 256 at a time left
    // the instruction count and the 52 active lanes per instruction unchanged, profiles/r02_experiments.txt item 13.)
    // One workgroup-wide step: thread t shades queue entry i (live = it has one).  Every thread of the workgroup
    // calls this together: the compaction at the end has barriers.
    // (PARK) The arguments again, read through a kernarg pointer made opaque inside the grid-stride loop: what is derived from
    // them (float copies of scalars, item-decoding terms, addresses) can then not be hoisted out of that loop into vector
    // registers that stay occupied - and spilled - through every cast; the fields are fetched by scalar loads where they are used.
    auto scene_arg = [&]() -> const DevScene& { return PARK ? wf_opaque_arg<DevScene>(0u) : S; };
    auto params_arg = [&]() -> const WfParams& { return PARK ? wf_opaque_arg<WfParams>(WF_ARG_OFFSET_W) : W; };
    auto shade_one = [&](const uint32_t e, bool live) {   // e: position in the queue / in the lists
    const DevScene& S = scene_arg();
    const WfParams& W = params_arg();
    const uint32_t i = (list_pass && live) ? entry_index(e) : e;
    f3 o = mk3(0, 0, 0), d = mk3(0, 0, 1), thr = mk3(0, 0, 0), color = mk3(0, 0, 0);
    uint32_t item = i, draw = 0, out_slot = 0;
    RawHit h;
    bool hit = false;
    WfRng rng;
    rng.block = 0xffffffffu;
    uint32_t word2 = 0, word3 = 0;                      // GRID == 3: words 2 and 3 of the item's ChaCha block
    uint4 later_words = make_uint4(0u, 0u, 0u, 0u);     //            words 4-7 (bounces 1 and 2; the alpha walk of bounce 0)
    // rng.gen::<f32>() number idx (>= 2) of the path at bounce 0, GRID == 3: from the block in registers; beyond
    // word 7 (more than three alpha draws) the block is derived again by wf_rng_draw
    auto draw_b0 = [&](uint32_t idx) -> float {
        if (idx >= (CACHED ? 4u : WF_RNG_STAGED)) return wf_rng_draw(rng, W, tile_offsets, rng_planes, item, idx);   // (CACHED: plane 1 of the cache)
        uint32_t word = word2;
        word = idx == 3u ? word3 : word;
        word = idx == 4u ? later_words.x : word;
        word = idx == 5u ? later_words.y : word;
        word = idx == 6u ? later_words.z : word;
        word = idx == 7u ? later_words.w : word;
        return wf_rng_float(word);
    };
    // (LOAD) the item's camera hit: a dense load that depends on nothing - its latency runs under decode_item and the ray set-up
    // (LEAN) the three late records first: loads return in order, so when the step's last dense load - the item's words - is
    // there, so are they, and the stores that put them into LDS (behind the ray set-up) wait for nothing of their own
    uint4 late_next = make_uint4(0u, 0u, 0u, 0u), late_d = make_uint4(0u, 0u, 0u, 0u), late_thr = make_uint4(0u, 0u, 0u, 0u);
    if constexpr (LEAN) {
        if (live) late_next = next_plane[i], late_d = cont_plane[i], late_thr = cont_plane[cont_stride + i];
    }
    uint4 cam_rec = make_uint4(0xffffffffu, 0u, 0u, 0u);
    if (LOAD && PRIMARY && live) cam_rec = hit_plane[i];
    // (VIS) the item's visibility byte, as dense and as independent: two bits per light - 0 unknown, 1 not blocked, 2 blocked
    // (og_blocked of the item's surface and that light).  Bit 8, in the register only: this launch found one of them out.
    uint32_t vis = 0u;
    if constexpr (VIS) {
        if (live) vis = vis_plane[i];
    }
    // (NEXT) the record of the item's bounce-1 cast, as dense and as independent: read for every item, used by the survivors.
    // (Issued behind the lights, where only the survivors would load it, its latency stood in front of the compaction's
    // barriers in every step: the launch took 13.9 ms for the 8.1 ms of the kernel without it.)
    // NEXT_WORD (the variant with the orthographic branch): the word alone, (key, u, v) read again where a hit is written - the
    // whole record held through the lights is 20 B of scratch there (8 B this way); without that branch it is none, and the
    // second read cost the launch 0.16 ms (8.29 against 8.13 ms).
    constexpr bool NEXT_WORD = NEXT && DIRL;
    uint4 next_rec = make_uint4(0u, 0u, 0u, 0u);
    if constexpr (LEAN) {
        // (read from sh_late where it is used)
    } else if constexpr (NEXT_WORD) {
        if (live) next_rec.x = ((const uint32_t*)next_plane)[4u * (size_t)i];
    } else if constexpr (NEXT) {
        if (live) next_rec = next_plane[i];
    }
    // (CONT_LOAD) the item's continuation, as dense and as independent: read for every item, used by the hit lanes.  (For the
    // lanes whose camera record is a hit only, and with nontemporal loads: 0.04 and 0.09 ms of a 12.2 ms frame, inside the
    // spread of the runs, the second at 8 B of scratch - profiles/r19_experiments.txt item 3.)
    uint4 cont_d = make_uint4(0u, 0u, 0u, 0u), cont_thr = make_uint4(0u, 0u, 0u, 0u);
    if constexpr (CONT_LOAD && !LEAN) {
        if (live) cont_d = cont_plane[i], cont_thr = cont_plane[cont_stride + i];
    }
    if (PRIMARY && live) {  // entry i is work item i: the initial path state, built in place
        ItemRef it = decode_item(W.P, tile_offsets, W.item_base + i);
        if (!it.valid) {
            live = false;
        } else {
            thr = mk3(1.f, 1.f, 1.f);
            color = mk3(0.f, 0.f, 0.f);
            out_slot = (it.sample - 1u - W.P.sample_begin) * W.P.n_local + it.out_index;
            if (GRID >= 2) {   // ray_cast + alpha walk of the camera ray (mod.rs:182-205) through the camera grid
                if constexpr (LEAN) {   // words 0 and 1 alone: the continuation is loaded, nothing draws from words 2 and 3
                    const uint2 w01 = *(const uint2*)(rng_planes + i);
                    float sx, sy;
                    primary_screen(S, it.x, it.y, W.P.width, W.P.height, wf_rng_float(w01.x), wf_rng_float(w01.y), sx, sy);
                    primary_from_screen(S, sx, sy, o, d);
                } else
                if (GRID == 3 && CACHED) {   // the same words, made once per item enumeration: one dense 16-byte load
                    const uint4 w03 = rng_planes[i];
                    float sx, sy;
                    primary_screen(S, it.x, it.y, W.P.width, W.P.height, wf_rng_float(w03.x), wf_rng_float(w03.y), sx, sy);
                    primary_from_screen(S, sx, sy, o, d);
                    word2 = w03.z;
                    word3 = w03.w;
                } else if (GRID == 3) {   // StdRng::seed_from_u64(sample + i * samples), jitter x then y (mod.rs:110-120)
                    uint32_t w[16];
                    pt_chacha12_block((uint64_t)it.sample + (uint64_t)it.global_index * (uint64_t)W.P.samples, 0u, w);
                    float sx, sy;
                    primary_screen(S, it.x, it.y, W.P.width, W.P.height, wf_rng_float(w[0]), wf_rng_float(w[1]), sx, sy);
                    primary_from_screen(S, sx, sy, o, d);
                    word2 = w[2];
                    word3 = w[3];
                    later_words = make_uint4(w[4], w[5], w[6], w[7]);
                } else {
                    const uint2 sc = *(const uint2*)(rng_planes + i);  // jittered screen position (k_wf_rng)
                    primary_from_screen(S, __uint_as_float(sc.x), __uint_as_float(sc.y), o, d);
                }
                if (LOAD) {   // the cast's result as an earlier frame of this view stored it
                    draw = 2u;
                    hit = unpack_hit(cam_rec, h);
                } else {
                    const uint32_t cell = og_cell(S.cam_grid, d);
                    const float dlen = mag3(d);
                    const float kmax = (dlen > 1.0f ? dlen : 1.0f) * 1.00002f;
                    draw = 2u;   // the pixel jitter
                    if (COUNT) lc.segments++;
                    const uint32_t tris_before = lc.tris;
                    hit = og_next_hit<COUNT>(S, S.cam_grid, cell, o, d, kmax, INFINITY, -INFINITY, 0u, h, lc);
                    if (STORE) hit_plane[i] = pack_hit(h, hit);
                    if (ALPHA) {
                        RawHit kept = h;
                        bool have_kept = false;
                        while (hit) {
                            const float opacity = hit_opacity(S, o, d, h);
                            if (COUNT) lc.shaded++;
                            bool stop = opacity >= 1.f;
                            if (!stop && opacity > 0.001f)
                                stop = (GRID == 3 ? draw_b0(draw++) : wf_rng_draw(rng, W, tile_offsets, rng_planes, item, draw++)) < opacity;
                            if (stop) break;
                            kept = h;   // skipped: remember it, look for the next entry of the list
                            have_kept = true;
                            if (COUNT) lc.restarts++;
                            hit = og_next_hit<COUNT>(S, S.cam_grid, cell, o, d, kmax, INFINITY, kept.key, kept.ord, h, lc);
                        }
                        if (!hit && have_kept) {   // every hit skipped: the last one is shaded
                            h = kept;
                            hit = true;
                        }
                    }
                    if (COUNT) n_cam_tris += lc.tris - tris_before;
                }
            } else {
                draw = ALPHA ? draws[i] : 2u;   // 2 = the pixel jitter (+ the draws of the alpha walk)
                hit = wf_load_hit(hits, W.hcap, i, h);
                if (hit) {  // (a missed cast only adds the background: no ray, no normalisation)
                    const uint2 sc = *(const uint2*)(rng_planes + i);  // jittered screen position (k_wf_rng)
                    primary_from_screen(S, __uint_as_float(sc.x), __uint_as_float(sc.y), o, d);
                }
            }
            if (COUNT) n_new++;
        }
    }
    if constexpr (LEAN) {   // (a lane reads its slots only where it is live and hit: those lanes stored them here)
        if (live) {
            late[0] = (WfLateRec){late_next.x, late_next.y, late_next.z, late_next.w};
            late[WF_SHADE_THREADS] = (WfLateRec){late_d.x, late_d.y, late_d.z, late_d.w};
            late[2u * WF_SHADE_THREADS] = (WfLateRec){late_thr.x, late_thr.y, late_thr.z, late_thr.w};
        }
    }
    if (!PRIMARY && live) {
        const float4* qr = wf_ray_rec(queue_in, i);
        const float4* qp = wf_path_rec(queue_in, W.qcap_in, i);
        float4 q0 = qr[0], q1 = qr[1], q2 = qp[0], q3 = qp[1];
        o = mk3(q0.x, q0.y, q0.z);
        d = mk3(q0.w, q1.x, q1.y);
        thr = mk3(q2.x, q2.y, q2.z);
        color = mk3(q3.x, q3.y, q3.z);
        item = __float_as_uint(q1.z);
        draw = ALPHA ? draws[i] : (__float_as_uint(q1.w) & 0xffffu);
        out_slot = __float_as_uint(q2.w);
        hit = entry_hit(e, i, h);
        if (out_slot == 0xffffffffu) live = false;  // (records of items outside the image; none since bounce 0 is fused)
        // (VIS1) the record's visibility byte, as soon as its slot is there, and (NEXT1) the item's bounce-2 record, as soon as
        // the item is: their latency runs under make_surface and material_sample
        if constexpr (VIS1) {
            if (live) vis = vis_plane[out_slot];
        }
        if constexpr (NEXT1) {
            if (live && item < W.n_items) next_rec = next_plane[item];
        }
    }
    const uint32_t bounce = PRIMARY ? 0u : W.bounce, bounces = W.P.bounces;   // (PRIMARY: no Russian roulette code at all)
    bool to_shadow = false, survive = false;
    bool cold = false;   // (LEAN) the lane needs what this variant does not contain
    bool inlined = false, ended_inline = false;   // (VIS1: the lights were added here; ... and the path ended for it)
    f3 term0 = mk3(0.f, 0.f, 0.f);
    Surface surf;
    f3 next_o = o, next_d = d, next_thr = thr;
    // background (mod.rs:184-186): the path ends here.  Bounce 0 only: a miss of a later bounce never gets here - its
    // result was staged by the kernel that finished the record's colour (wf_prestage_miss)
    if (PRIMARY && live && !hit) {
        color = color + mul_ew(thr, ld3(S.background));
        float* out = staging + (size_t)out_slot * 3;
        out[0] = color.x;
        out[1] = color.y;
        out[2] = color.z;
    }
    Brdf brdf;
    f3 normal = mk3(0, 0, 0), view = mk3(0, 0, 0);
    if (live && hit) {
        if (COUNT) n_hits++;
        make_surface(S, o, d, h, surf);
        MatSample ms;
        material_sample(S, surf.model, surf.sphere, surf.uv, ms);
        normal = shading_normal(S, surf);
        if (COUNT && !ALPHA) atomicAdd(&gctr->shaded_hits, 1ull);
        view = -1.f * d;
        ct_init(brdf, ms);
        color = color + mul_ew(thr, ms.emissive);
        f3 lit = color;   // (VIS1: ... with the lights)
        // (thr ⊙ eval_direct) per light.  GRID: the light's visibility is looked up here and the light added at
        // once, in light order (mod.rs:248-262).  Otherwise (and for a normal too long for the grids' margin) the
        // visibility factor is applied by the shadow kernel: the first light's term stays in registers, the others
        // are recomputed when the record is written.
        const bool inline_lights = GRID != 0 && dot3(surf.normal, surf.normal) <= S.light_grid_max_normal2;
        // (PARK) what no cast changes is parked once, what a light changes right before its cast; all of it comes back after
        auto park_fixed = [&] {
            park_f(PK_BRDF, brdf.metalness), park_f(PK_BRDF + 1u, brdf.roughness);
            park_3(PK_BRDF + 2u, brdf.albedo), park_3(PK_BRDF + 5u, brdf.emissive), park_3(PK_BRDF + 8u, brdf.f0);
            park_3(PK_NORMAL, normal), park_3(PK_VIEW, view);
            park_f(PK_UV, surf.uv.x), park_f(PK_UV + 1u, surf.uv.y);
            park_u(PK_PID, h.pid), park_u(PK_OUT_SLOT, out_slot), park_u(PK_WORD2, word2), park_u(PK_WORD2 + 1u, word3);
        };
        auto unpark_fixed = [&] {
            brdf.metalness = unpark_f(PK_BRDF), brdf.roughness = unpark_f(PK_BRDF + 1u);
            brdf.albedo = unpark_3(PK_BRDF + 2u), brdf.emissive = unpark_3(PK_BRDF + 5u), brdf.f0 = unpark_3(PK_BRDF + 8u);
            normal = unpark_3(PK_NORMAL), view = unpark_3(PK_VIEW);
            surf.uv.x = unpark_f(PK_UV), surf.uv.y = unpark_f(PK_UV + 1u);
            h.pid = unpark_u(PK_PID), out_slot = unpark_u(PK_OUT_SLOT), word2 = unpark_u(PK_WORD2), word3 = unpark_u(PK_WORD2 + 1u);
        };
        if (PARK && !VIS) park_fixed();   // (VIS: around the casts that are still made)
        for (uint32_t li = 0; li < S.n_lights; ++li) {
            const DevLight& L = S.lights[li];
            f3 ldir = L.kind == PT_LIGHT_POINT ? normalize3(surf.pos - ld3(L.vec)) : ld3(L.vec);
            f3 c = mul_ew(thr, ct_eval_direct(brdf, normal, view, -1.f * ldir));
            if (li == 0) term0 = c;
            const bool moot = wf_light_is_moot(L, c, surf.pos);
            if (GRID != 0 && inline_lights) {
                if (moot) {
                    if (COUNT) n_moot++;
                } else if constexpr (VIS) {
                    // og_light_radiance with the cast's answer kept: a light whose bits are known costs the radiance alone - no
                    // grid cell, no list, no primitive, no slab test.  The cast and all the parking around it sit behind
                    // this branch: a wavefront none of whose lanes has an unknown light skips it, and once the plane is
                    // full no LDS parking instruction is issued at all.
                    const uint32_t known = (vis >> (2u * li)) & 3u;
                    bool blocked = known == 2u;
                    if constexpr (LEAN) {   // an unknown light: the lane is cold
                        if (known == 0u) cold = true;
                    } else
                    if (known == 0u) {
                        if (PARK) park_fixed(), park_3(PK_C, c), park_3(PK_COLOR, color), park_3(PK_TERM0, term0), park_u(PK_VIS, vis);
                        if (PARK && NEXT) park_u(PK_NEXT, next_rec.x), park_u(PK_NEXT + 1u, next_rec.y), park_u(PK_NEXT + 2u, next_rec.z), park_u(PK_NEXT + 3u, next_rec.w);
                        blocked = og_light_blocked<DIRL>(S, li, surf.pos, surf.normal, lc);
                        if (PARK) {
                            c = unpark_3(PK_C), color = unpark_3(PK_COLOR), term0 = unpark_3(PK_TERM0), vis = unpark_u(PK_VIS);
                            if (NEXT) next_rec = make_uint4(unpark_u(PK_NEXT), unpark_u(PK_NEXT + 1u), unpark_u(PK_NEXT + 2u), unpark_u(PK_NEXT + 3u));
                            unpark_fixed();
                        }
                        if constexpr (CONT_LOAD) {
                            // the continuation across the cast: six slots more would cost the fourth workgroup per CU, and the
                            // planes are read-only in this launch - the lanes that cast read their records again
                            // (volatile: a plain load is merged with the one at the top of the step, and the records held)
                            const volatile uint32_t* again = (const volatile uint32_t*)(cont_plane + i);
                            cont_d = make_uint4(again[0], again[1], again[2], again[3]);
                            again = (const volatile uint32_t*)(cont_plane + cont_stride + i);
                            cont_thr.x = again[0], cont_thr.y = again[1], cont_thr.z = again[2];
                            // ... and leave a mark: a frame that made no such cast may take the lean variant next.  One word
                            // of LDS per workgroup (sh_cnt[3][1]: nobody else's), added to the device's counter once, at the
                            // end - an atomic per wave and cast on the one word made the frame that fills the visibility
                            // plane 16 ms longer (157.9 -> 173.9 ms, profiles/r21_experiments.txt item 2)
                            sh_cnt[NEXT ? 3 : 0][1] = 1u;
                        }
                        vis |= ((blocked ? 2u : 1u) << (2u * li)) | 0x100u;
                    }
                    f3 rad = og_light_unshadowed<DIRL>(S, li, surf.pos);
                    if (blocked) rad = rad * 0.0f;
                    if (!(rad.x == 0.f && rad.y == 0.f && rad.z == 0.f)) color = color + mul_ew(c, rad);
                } else {
                    if (PARK) park_3(PK_C, c), park_3(PK_COLOR, color), park_3(PK_TERM0, term0);
                    const f3 rad = og_light_radiance<ALPHA, COUNT, DIRL>(S, li, surf.pos, surf.normal, surf.uv, surf.sphere, lc);
                    if (PARK) {
                        c = unpark_3(PK_C), color = unpark_3(PK_COLOR), term0 = unpark_3(PK_TERM0);
                        unpark_fixed();
                    }
                    if (!(rad.x == 0.f && rad.y == 0.f && rad.z == 0.f)) color = color + mul_ew(c, rad);
                }
            } else if (!moot) {
                if constexpr (LEAN) cold = true;   // (a normal too long for the grids' margin: the lane would write a shadow record)
                else if constexpr (!LEAN1) to_shadow = true;
                if constexpr (LEAN1) {
                    // the light as the general variant adds it to `lit` - which starts as this colour -, added here: unknown
                    // bits make the lane cold, and a cold lane's colour goes nowhere
                    const uint32_t known = (vis >> (2u * li)) & 3u;
                    if (known == 0u) cold = true;
                    inlined = true;
                    f3 rad = og_light_unshadowed<false>(S, li, surf.pos);
                    if (known == 2u) rad = rad * 0.0f;
                    if (!(rad.x == 0.f && rad.y == 0.f && rad.z == 0.f)) color = color + mul_ew(c, rad);
                } else
                if constexpr (VIS1) {
                    // the light as k_og_shadow_vis would add it, should every live light of the record turn out known (bit 8,
                    // in the register only: one of them is not)
                    const uint32_t known = (vis >> (2u * li)) & 3u;
                    if (known == 0u) vis |= 0x100u;
                    f3 rad = og_light_unshadowed<false>(S, li, surf.pos);
                    if (known == 2u) rad = rad * 0.0f;
                    if (!(rad.x == 0.f && rad.y == 0.f && rad.z == 0.f)) lit = lit + mul_ew(c, rad);
                }
            }
        }
        if constexpr (LEAN1) {
            // all of the record's lights, or none, here too: the general variant would send this record to the shadow queue for
            // a normal too long for the grids' margin, so the lane is cold; so is one whose two draws are not both staged words
            if (inlined && !(dot3(surf.normal, surf.normal) <= S.light_grid_max_normal2)) cold = true;
            if (bounce < bounces && draw + 1u >= WF_RNG_STAGED) cold = true;
            if (cold) inlined = false;
        } else
        if constexpr (VIS1) {
            // all of the record's lights, or none: a partly added record would change the order of the additions.  A normal too
            // long for the grids' margin, or an unknown bit: the record goes to the shadow queue whole, as in k_wf_shade.
            if (to_shadow && !(vis & 0x100u) && dot3(surf.normal, surf.normal) <= S.light_grid_max_normal2) {
                color = lit;
                to_shadow = false;
                inlined = true;
            }
        }
        if (COUNT && !inline_lights && !to_shadow) n_moot += S.n_lights;
        if constexpr (VIS && !LEAN) {   // what this launch found out: one byte store per lane that cast; none once the plane is full
            if (vis & 0x100u) vis_plane[i] = (uint8_t)vis;
        }
        bool ended = false;
        uint32_t esc_state = 0u;   // (CONT_STORE) bits 1 and 2 of the record's state word
        if constexpr (CONT_LOAD) {
            if (bounce < bounces) {   // what the storing launch computed here, bit for bit
                next_o = surf.pos + surf.normal * 0.00001f;
                draw += 2u;
                if constexpr (LEAN) cont_d = late_get(1u), cont_thr = late_get(2u);   // (the thread's own slots, stored above)
                next_d = mk3(__uint_as_float(cont_d.x), __uint_as_float(cont_d.y), __uint_as_float(cont_d.z));
                next_thr = mk3(__uint_as_float(cont_thr.x), __uint_as_float(cont_thr.y), __uint_as_float(cont_thr.z));
                // a hit lane without a record cannot occur below the mark: counted (next_ctr[6]; its zero throughput ends the path)
                const bool missing = (cont_d.w & 1u) == 0u;
                if constexpr (LEAN) {   // ... and cold
                    if (missing) cold = true;
                } else
                if (wf_any(missing)) {
                    const unsigned long long m = __ballot(missing);
                    if (missing && wf_lane_rank(m) == 0u) atomicAdd(next_ctr + 6, (unsigned long long)__popcll(m));
                }
            }
        } else if (bounce < bounces && !(LEAN1 && cold)) {
            next_o = surf.pos + surf.normal * 0.00001f;
            float r1, r2;
            if constexpr (LEAN1) {   // draws 2b+2 and 2b+3 of an opaque path: words 4-7 of the staged plane (any other lane is cold)
                r1 = wf_rng_float(wf_rng_staged(rng_planes, W.cap, W.rng_first_plane, item, draw));
                r2 = wf_rng_float(wf_rng_staged(rng_planes, W.cap, W.rng_first_plane, item, draw + 1u));
                draw += 2u;
            } else
            if (GRID == 3 && ALPHA) {
                r1 = draw_b0(draw++);
                r2 = draw_b0(draw++);
            } else if (GRID == 3) {
                r1 = wf_rng_float(word2);
                r2 = wf_rng_float(word3);
                draw += 2u;
            } else if (PRIMARY && !ALPHA) {   // draws 2 and 3 of the item: staged next to the screen position (k_wf_rng)
                const uint2 w23 = *(const uint2*)((const uint32_t*)(rng_planes + item) + 2);
                r1 = wf_rng_float(w23.x);
                r2 = wf_rng_float(w23.y);
                draw += 2u;
            } else {
                r1 = wf_rng_draw(rng, W, tile_offsets, rng_planes, item, draw++);
                r2 = wf_rng_draw(rng, W, tile_offsets, rng_planes, item, draw++);
            }
            if constexpr (LEAN1) {
                park1[0] = out_slot, park1[WF_SHADE_THREADS] = item;
                park1[2u * WF_SHADE_THREADS] = __float_as_uint(color.x), park1[3u * WF_SHADE_THREADS] = __float_as_uint(color.y);
                park1[4u * WF_SHADE_THREADS] = __float_as_uint(color.z);
                park1[5u * WF_SHADE_THREADS] = __float_as_uint(next_o.x), park1[6u * WF_SHADE_THREADS] = __float_as_uint(next_o.y);
                park1[7u * WF_SHADE_THREADS] = __float_as_uint(next_o.z), park1[8u * WF_SHADE_THREADS] = h.pid;
            }
            next_d = ct_sample(brdf, normal, view, r1, r2);
            f3 wgt = ct_eval_indirect(brdf, normal, view, next_d) / 1.0f;
            next_thr = mul_ew(thr, wgt);
            if constexpr (LEAN1) {
                out_slot = park1[0], item = park1[WF_SHADE_THREADS];
                next_o.x = __uint_as_float(park1[5u * WF_SHADE_THREADS]), next_o.y = __uint_as_float(park1[6u * WF_SHADE_THREADS]);
                next_o.z = __uint_as_float(park1[7u * WF_SHADE_THREADS]), h.pid = park1[8u * WF_SHADE_THREADS];
                color.x = __uint_as_float(park1[2u * WF_SHADE_THREADS]), color.y = __uint_as_float(park1[3u * WF_SHADE_THREADS]);
                color.z = __uint_as_float(park1[4u * WF_SHADE_THREADS]);
            }
            if constexpr (CONT_STORE) {
                // the escape test's answer for the lanes that will ask for it (not ended, a triangle, masks there): bit 1 - it
                // was evaluated, with the masks that exist now -, bit 2 - the answer; the test below reads it from here
                if (!(dot3(next_thr, next_thr) < 0.00001f) && S.escape != nullptr && !surf.sphere)
                    esc_state = 2u | (escape_proves_miss(S, PT_PRIM_INDEX(h.pid), next_o, next_d) ? 4u : 0u);
                cont_plane[i] = make_uint4(__float_as_uint(next_d.x), __float_as_uint(next_d.y), __float_as_uint(next_d.z), 1u | esc_state);
                cont_plane[cont_stride + i] = make_uint4(__float_as_uint(next_thr.x), __float_as_uint(next_thr.y), __float_as_uint(next_thr.z), 0u);
            }
        }
        if (dot3(next_thr, next_thr) < 0.00001f) ended = true;
        if constexpr (LEAN1) {   // (nothing of a cold lane's is asked of the masks)
            if (cold) ended = true;
        }
        if (!LEAN1 && !ended && bounce > 3) {   // (LEAN1: bounces 1 and 2)
            float p = max_rs(max_rs(next_thr.x, next_thr.y), next_thr.z);
            next_thr = next_thr * (1.f / p);
            if (wf_rng_draw(rng, W, tile_offsets, rng_planes, item, draw++) > p) ended = true;
        }
        survive = !ended && bounce + 1 <= bounces;
        // Escape mask of the primitive the ray leaves (pt_escape.h): a clear bit proves that the next ray_cast is empty, i.e.
        // that the path ends with `colour + throughput x background` (mod.rs:184-186) - no record, no cast.  The background
        // term must be added AFTER this bounce's lights (mod.rs:248-262 come first): here if the lights are added here
        // (inline) or none can contribute; through the shadow queue only if the term is exactly zero (a black background).
        if constexpr (CONT_LOAD || CONT_STORE) {
            // The same with the answer from the record (the statement below is kept as it is for every other kernel: written
            // as one, the two forms changed the code of 57 of them).  CONT_STORE: evaluated above, where it was recorded.
            // CONT_LOAD: the recorded answer where the launch was told that the scene's masks are those the records were made
            // with - cont_flags bit 0 - and the record has one; any other lane runs the test itself, behind a branch that a
            // wavefront with no such lane skips.
            bool proven = false;
            if (survive && S.escape != nullptr && !surf.sphere) {
                if constexpr (CONT_STORE) {
                    proven = (esc_state & 4u) != 0u;
                } else {
                    const bool known = (cont_flags & 1u) != 0u && (cont_d.w & 2u) != 0u;
                    proven = known && (cont_d.w & 4u) != 0u;
                    if constexpr (LEAN) {   // the test is needed and the record has no answer for these masks: cold
                        if (!known) cold = true;
                    } else
                    if (wf_any(!known)) {
                        if (!known) proven = escape_proves_miss(S, PT_PRIM_INDEX(h.pid), next_o, next_d);
                        // the lanes that ran the test although the launch was told the records have answers: counted
                        // (next_ctr[7]; none once k_cont_escape_fill has been over the records)
                        if ((cont_flags & 1u) != 0u) {
                            const unsigned long long m = __ballot(!known);
                            if (!known && wf_lane_rank(m) == 0u) atomicAdd(next_ctr + 7, (unsigned long long)__popcll(m));
                        }
                    }
                }
            }
            if (proven) {
                const f3 bg = mul_ew(next_thr, ld3(S.background));
                const bool zero = bg.x == 0.f && bg.y == 0.f && bg.z == 0.f;
                if (zero || !to_shadow) {
                    if (!zero) color = color + bg;
                    survive = false;
                }
            }
        } else
        if (survive && S.escape != nullptr && !surf.sphere && escape_proves_miss(S, PT_PRIM_INDEX(h.pid), next_o, next_d)) {
            const f3 bg = mul_ew(next_thr, ld3(S.background));
            const bool zero = bg.x == 0.f && bg.y == 0.f && bg.z == 0.f;
            if (zero || !to_shadow) {
                if (!zero) color = color + bg;
                survive = false;
                if (COUNT) n_masked++;
                // (VIS1: k_wf_shade would have kept this path - a record of the next queue whose cast misses)
                if (VIS1 && !zero && inlined) ended_inline = true;
            }
        }
    }
    // (NEXT) A survivor whose next cast is known to miss, behind a colour that is final: what wf_prestage_miss stages for it
    // (below, with the other stores) IS the sample - no record, no slot, nothing for bounce 1 to read.  A to_shadow survivor
    // keeps its record whatever the cast found: the shadow kernel patches the colour and stages the miss.
    bool elided = false;
    if constexpr (LEAN) {
        // a cold lane writes nothing - no record, no sample, no count - and flags the frame (bit 1 of the word a full queue
        // sets: the configuration's next call fails, pt_gpu.hip frame_plan)
        if (cold) {
            survive = false;
            atomicOr(&ctr[0].overflow, 2u);
        }
        // (the word alone; the rest where the hit is written, behind the barriers)
        if (survive) next_rec.x = *(volatile __attribute__((address_space(3))) uint32_t*)late;
    }
    if constexpr (LEAN1) {
        // a cold lane writes nothing - no record, no sample, no count - and hands its queue entry over.  (An entry is handed
        // over once at most and the list is as long as the queue: the bound holds by construction and is checked all the same.)
        if (cold) survive = false, inlined = false, ended_inline = false;
        if (wf_any(cold)) {
            const uint32_t slot = wf_reserve(handover + W.bounce, cold);
            if (cold && slot < W.qcap_in) handover[WF_HANDOVER_HEAD + slot] = i;
            else if (cold) ctr[0].overflow = 1u;
            const unsigned long long m = __ballot(cold);
            if (cold && wf_lane_rank(m) == 0u) atomicAdd(next_ctr + 6, (unsigned long long)__popcll(m));   // (pt_get_b1_lean_stats)
        }
    }
    if constexpr (NEXT) {
        elided = survive && !to_shadow && next_rec.x == (0xffffffffu ^ WF_HIT1_FLIP);
        if (elided) survive = false;
    }
    if constexpr (NEXT1) {   // the same one bounce later
        elided = survive && !to_shadow && next_rec.x == (0xffffffffu ^ WF_HIT1_FLIP);
        if (elided) survive = false;
    }
    // ---- compaction: survivors -> queue[b+1], surface hits -> shadow queue.  One atomic per
    // workgroup and queue (wave ballots -> LDS -> one lane), not one per wavefront: the counter
    // word would otherwise cap the kernel at ~88 M wave-atomics per second.
    // Coherence sorting (W.sort_octants): the survivors of a workgroup step - paths that started in the same few
    // 8x8 pixel blocks - are placed in the workgroup's slice of the queue by the OCTANT of their new direction
    // (ballot per octant, mbcnt rank, prefix over octants and waves in LDS), so that the 64 consecutive records a
    // wavefront of the next k_wf_trace launch fetches walk the tree in the same child order.  The position of a
    // record in a queue is free (results are keyed by out_slot), so no bit of the image changes.
    unsigned long long m_next = __ballot(survive), m_sh = __ballot(to_shadow);
    const unsigned long long m_elided = NEXT ? __ballot(elided) : 0ull;
    const unsigned long long m_gone = VIS1 ? __ballot(elided || ended_inline) : 0ull, m_inlined = VIS1 ? __ballot(inlined) : 0ull;
    uint32_t oct = 0, oct_rank = 0;
    if (!LEAN1 && (W.sort_octants & 1u)) {
        oct = (next_d.x < 0.f ? 1u : 0u) | (next_d.y < 0.f ? 2u : 0u) | (next_d.z < 0.f ? 4u : 0u);
#pragma unroll
        for (uint32_t k = 0; k < 8u; ++k) {
            const unsigned long long m = __ballot(survive && oct == k);
            if ((threadIdx.x & 63u) == 0) sh_oct[k][wave] = (uint32_t)__popcll(m);
            if (oct == k) oct_rank = wf_lane_rank(m);
        }
    }
    if ((threadIdx.x & 63u) == 0) {
        sh_cnt[0][wave] = (uint32_t)__popcll(m_next);
        sh_cnt[1][wave] = (uint32_t)__popcll(m_sh);
        if constexpr (NEXT) sh_cnt[2][wave] = (uint32_t)__popcll(m_elided);
        // (VIS1: three counts of at most 64 in the one word - the sum over the waves stays below 10 bits a field)
        if constexpr (VIS1) sh_cnt[1][wave] = (uint32_t)__popcll(m_sh) | ((uint32_t)__popcll(m_gone) << 10) | ((uint32_t)__popcll(m_inlined) << 20);
    }
    __syncthreads();
    if (NEXT && threadIdx.x == 2) {
        uint32_t total = 0;
        for (uint32_t k = 0; k < WF_SHADE_THREADS / 64; ++k) total += sh_cnt[2][k];
        sh_cnt[NEXT ? 3 : 0][2] += total;
    } else if (threadIdx.x < 2) {
        uint32_t total = 0;
        for (uint32_t k = 0; k < WF_SHADE_THREADS / 64; ++k) total += sh_cnt[threadIdx.x][k];
        if (VIS1 && threadIdx.x == 1) total &= 0x3ffu;
        uint32_t* counter = threadIdx.x == 0 ? &ctr[bounce + 1].queue_count : &ctr[bounce].shadow_count;
        sh_base[threadIdx.x] = total ? atomicAdd(counter, total) : 0u;
        if (NEXT && threadIdx.x == 0) sh_cnt[NEXT ? 3 : 0][0] += total;
        if (VIS1) fused_acc[threadIdx.x] += total;
    } else if (VIS1 && threadIdx.x < 4) {   // thread 2: the ended and the elided, thread 3: the records with their lights added here
        uint32_t total = 0;
        for (uint32_t k = 0; k < WF_SHADE_THREADS / 64; ++k) total += sh_cnt[1][k];
        fused_acc[threadIdx.x] += (total >> (10u * (threadIdx.x - 1u))) & 0x3ffu;
    } else if (!LEAN1 && (W.sort_octants & 1u) && threadIdx.x >= 64u && threadIdx.x < 64u + 8u * (WF_SHADE_THREADS / 64)) {
        // exclusive prefix of the (octant, wave) counts, octant-major
        const uint32_t e = threadIdx.x - 64u;
        uint32_t before = 0;
        for (uint32_t j = 0; j < e; ++j) before += sh_oct[j / (WF_SHADE_THREADS / 64)][j % (WF_SHADE_THREADS / 64)];
        sh_oct_off[e / (WF_SHADE_THREADS / 64)][e % (WF_SHADE_THREADS / 64)] = before;
    }
    __syncthreads();
    uint32_t next_idx = sh_base[0] + wf_lane_rank(m_next), sh_idx = sh_base[1] + wf_lane_rank(m_sh);
    for (uint32_t k = 0; k < wave; ++k) {
        next_idx += sh_cnt[0][k];
        sh_idx += VIS1 ? (sh_cnt[1][k] & 0x3ffu) : sh_cnt[1][k];
    }
    if (!LEAN1 && (W.sort_octants & 1u)) next_idx = sh_base[0] + sh_oct_off[oct][wave] + oct_rank;
    __syncthreads();  // sh_cnt / sh_base are rewritten by the next step
    // (the queues are sized by the records this very frame is known to produce, pt_gpu.hip FramePlan: a record beyond its
    // queue's end means that knowledge was wrong - nothing is written, the frame is flagged and rendered again with room)
    if ((survive && next_idx >= W.qcap_out) || (to_shadow && sh_idx >= W.scap)) {
        ctr[0].overflow = 1u;
        survive = false;
        to_shadow = false;
    }
    if (GRID == 3 && !CACHED && survive) rng_planes_out[(size_t)(1u - W.rng_first_plane) * W.cap + item] = later_words;   // draws 4-7 of the path
    if constexpr (NEXT || NEXT1) {
        // as k_wf_hits_load: the word and the hit to the chunk's hit plane at the record's queue position; an item without a
        // record to the next bounce's exact list (whose pass over the queue is unsplit: no WF_HIT_PENDING), and counted
        // (NEXT1: this launch is still reading the chunk's hit plane - next_hits is a plane of the next queue's own, as long
        // as that queue)
        const uint32_t next_hcap = NEXT1 ? W.qcap_out : W.hcap;
        const bool unknown = survive && next_rec.x == 0u;
        if (survive && !unknown) {
            const uint32_t word = next_rec.x ^ WF_HIT1_FLIP;
            ((uint32_t*)next_hits)[next_idx] = word;
            if constexpr (LEAN) {
                if (word != 0xffffffffu) next_rec = late_get(0u);
            }
            if (NEXT_WORD && word != 0xffffffffu) {   // (volatile: a plain load is merged with the word's, and the record held)
                const volatile uint32_t* rest = (const volatile uint32_t*)next_plane + 4u * (size_t)i;
                next_rec.y = rest[1], next_rec.z = rest[2], next_rec.w = rest[3];
            }
            if (word != 0xffffffffu) ((uint4*)((uint32_t*)next_hits + next_hcap))[next_idx] = make_uint4(next_rec.y, next_rec.z, next_rec.w, 0u);
        }
        if (wf_any(unknown)) {
            const uint32_t slot = wf_reserve(&ctr[bounce + 1].exact_count, unknown);
            if (unknown && slot < W.ecap) exact_next[slot] = next_idx;
            else if (unknown) ctr[0].overflow = 1u;
            const unsigned long long m = __ballot(unknown);
            if (unknown && wf_lane_rank(m) == 0u) {
                atomicAdd(next_ctr, (unsigned long long)__popcll(m));
                atomicAdd(next_ctr + 3, (unsigned long long)__popcll(m));
            }
        }
    } else if (!LEAN1 && W.exact_shade_lists) {   // (wave-uniform; 0.24 % of random directions)
        const bool listed = survive && slack_is_capped(__builtin_amdgcn_rcpf(next_d.x), __builtin_amdgcn_rcpf(next_d.y), __builtin_amdgcn_rcpf(next_d.z));
        if (wf_any(listed)) {
            const uint32_t slot = wf_reserve(&ctr[bounce + 1].exact_count, listed);
            if (listed && slot < W.ecap) exact_next[slot] = next_idx;
            else if (listed) ctr[0].overflow = 1u;
        }
        if constexpr (VIS1) {   // the entries of the paths that ended here instead (a handful per launch): counted for the frame plan
            const bool unlisted = ended_inline && slack_is_capped(__builtin_amdgcn_rcpf(next_d.x), __builtin_amdgcn_rcpf(next_d.y), __builtin_amdgcn_rcpf(next_d.z));
            const unsigned long long m = __ballot(unlisted);
            if (unlisted && wf_lane_rank(m) == 0u) atomicAdd(&ctr[bounce + 1].exact_elided, (uint32_t)__popcll(m));
        }
    }
    if (survive) {
        float4* qr = wf_ray_rec(queue_out, next_idx);
        float4* qp = wf_path_rec(queue_out, W.qcap_out, next_idx);
        qr[0] = make_float4(next_o.x, next_o.y, next_o.z, next_d.x);
        qr[1] = make_float4(next_d.y, next_d.z, __uint_as_float(item), __uint_as_float((draw & 0xffffu) | ((bounce + 1) << 16)));
        qp[0] = make_float4(next_thr.x, next_thr.y, next_thr.z, __uint_as_float(out_slot));
        qp[1] = make_float4(color.x, color.y, color.z, 0.f);  // colour is patched by the shadow kernels
        // ... and where none will (lights added inline, or none can contribute) it is final here: stage the path's result
        // for the case that its next cast misses
        if (!to_shadow) wf_prestage_miss(staging, out_slot, color, next_thr, ld3(S.background));
        if (W.use_entry) wf_entry_plane(queue_out, W.qcap_out)[next_idx] = S.prim_entry[PT_PRIM_INDEX(h.pid)];
    }
    if (!LEAN1 && to_shadow) {
        float4* sq = shadow_q + (size_t)sh_idx * 4;
        sq[0] = make_float4(surf.pos.x, surf.pos.y, surf.pos.z, surf.normal.x);
        sq[1] = make_float4(surf.normal.y, surf.normal.z, surf.uv.x, surf.uv.y);
        sq[2] = make_float4(color.x, color.y, color.z, __uint_as_float(survive ? next_idx : 0xffffffffu));
        sq[3] = make_float4(__uint_as_float(out_slot), __uint_as_float(surf.sphere ? WF_FLAG_SPHERE : 0u), 0.f, 0.f);
        contrib[sh_idx] = make_float4(term0.x, term0.y, term0.z, 0.f);
        for (uint32_t li = 1; li < S.n_lights; ++li) {
            // (PARK: one light per trip - two at a time in packed f32 made this rarely taken loop the kernel's register peak.
            // An empty asm, not `#pragma clang loop vectorize(disable)`: a pragma cannot depend on PARK, and on the one loop
            // all variants share it changes the code of every other variant; tests/test_bounce0_four_waves.py holds the
            // register count should a compiler stop honouring it.)
            if (PARK) asm volatile("");
            const DevLight& L = S.lights[li];
            f3 ldir = L.kind == PT_LIGHT_POINT ? normalize3(surf.pos - ld3(L.vec)) : ld3(L.vec);
            f3 c = mul_ew(thr, ct_eval_direct(brdf, normal, view, -1.f * ldir));
            contrib[(size_t)li * W.scap + sh_idx] = make_float4(c.x, c.y, c.z, 0.f);
        }
    } else if ((NEXT || NEXT1) && elided) {   // the sample of a path whose next cast is known to miss
        wf_prestage_miss(staging, out_slot, color, next_thr, ld3(S.background));
    } else if (live && hit && !survive && !((LEAN || LEAN1) && cold)) {  // no light can contribute and the path ends: the sample is complete
        float* out = staging + (size_t)out_slot * 3;
        out[0] = color.x;
        out[1] = color.y;
        out[2] = color.z;
    }
    // draws made HERE (the alpha walk counts its own): since the value this kernel started from, plus the jitter
    if (COUNT && live)
        n_draws += GRID >= 2 ? draw
                             : draw - (ALPHA ? draws[i] : PRIMARY ? 0u : (__float_as_uint(wf_ray_rec(queue_in, i)[1].w) & 0xffffu)) +
                                   ((ALPHA && PRIMARY) ? 2u : 0u);
    };  // shade_one
    if (PRIMARY || !WF_SHADE_AGGREGATE) {
        // grid-stride over the queue, one workgroup-wide step at a time (the loop bound is uniform in the workgroup)
        // Camera-grid cull (k_cam_block_mask): no camera ray of an EMPTY 8x8 pixel block can hit anything, so its samples
        // are the background - no ChaCha block, no cast (the instrumented variant counts them the long way).  A wavefront
        // is one block of one sample; chunks and queues are whole wavefronts.  Nothing is staged for them: k_accumulate
        // adds the background for the pixels of an empty block itself, once per sample.
        // (word W.n_mask_blocks of the table: non-zero if any block is empty - a frame without one pays nothing here)
        const bool cull = PRIMARY && GRID >= 2 && !COUNT && block_empty != nullptr && block_empty[W.n_mask_blocks] != 0u;
        for (uint32_t base = blockIdx.x * WF_SHADE_THREADS; base < n; base += gridDim.x * WF_SHADE_THREADS) {
            const uint32_t e = base + threadIdx.x;
            bool live = e < n;
            if (!PRIMARY && live) {   // bounces >= 1: the hits only (a miss was staged when its record's colour became final)
                const uint32_t word = entry_word(e);
                live = word != WF_HIT_PENDING && word != 0xffffffffu;
            }
            if (cull) {   // a step whose four wavefronts are all empty skips the compaction's barriers as well
                const uint32_t g0 = (W.item_base + base) >> 6;
                bool step_empty = true;
#pragma unroll
                for (uint32_t k = 0; k < WF_SHADE_THREADS / 64; ++k) {
                    const bool em = base + 64u * k >= n || block_empty[pt_fastdiv(g0 + k, W.P.div_batch)] != 0u;
                    step_empty = step_empty && em;
                    live = (k == wave && em) ? false : live;
                }
                if (step_empty) continue;   // (the same answer in every thread of the workgroup)
            }
            shade_one(e, live);
        }
    } else {
        // Hit aggregation (bounces >= 1).  Three of four secondary rays of an open scene leave into the background:
        // shaded in queue order, 23 % of the lanes would carry the material fetch, the BRDF and the GGX sample while
        // the others wait (27.7 of 64 lanes active per vector instruction, profiles/r02_a_pmc.json).  So a first
        // pass over a step's 256 entries reads the hit words only and collects the indices of the hits in LDS; whenever
        // 256 are waiting - or the queue has ended - they are shaded together.  A miss costs its 4-byte word and nothing
        // else: its result (background term, mod.rs:184-186) was staged when the record's colour became final
        // (wf_prestage_miss).  The order in which paths are shaded is free (results are keyed by out_slot), so no bit
        // changes.
        // The pass over the queue sweeps WF_SHADE_SWEEP words per thread and step (one 16-byte load): the sweep is a chain of
        // load -> ballots -> barrier -> LDS -> barrier per step, and a step of 256 words finds ~90 hits.  The lists of the second
        // launch (scattered words, a few thousand entries) keep one word per thread.
        __shared__ uint32_t agg[(1 + WF_SHADE_SWEEP) * WF_SHADE_THREADS];
        __shared__ uint32_t agg_cnt[WF_SHADE_THREADS / 64];
        const uint32_t per = list_pass ? 1u : (uint32_t)WF_SHADE_SWEEP;
        uint32_t have = 0;   // waiting hits (the same value in every thread; at most 255 + 256 * WF_SHADE_SWEEP)
        uint32_t base = blockIdx.x * WF_SHADE_THREADS * per;
        while (true) {
            while (have < WF_SHADE_THREADS && base < n) {
                const uint32_t e0 = base + threadIdx.x * per;
                base += gridDim.x * WF_SHADE_THREADS * per;
                uint32_t word[WF_SHADE_SWEEP];
#pragma unroll
                for (uint32_t j = 0; j < WF_SHADE_SWEEP; ++j) word[j] = WF_HIT_PENDING;
                static_assert(WF_SHADE_SWEEP == 4, "the sweep loads the words as one uint4");
                if (!list_pass && e0 + WF_SHADE_SWEEP <= n) {   // (e0 is a multiple of four: one aligned load of the words' plane)
                    const uint4 w4 = hits[e0 >> 2];
                    word[0] = w4.x, word[1] = w4.y, word[2] = w4.z, word[3] = w4.w;
                } else {
                    for (uint32_t j = 0; j < per; ++j)
                        if (e0 + j < n) word[j] = entry_word(e0 + j);
                }
                // (a miss: nothing to do, see above)  The hits keep their queue order - lane after lane, a lane's words in
                // order -: the exclusive prefix of the lanes' hit counts (0..4) comes from one ballot per bit of the count.
                // (Ranked word by word instead, neighbours in the queue land in different batches of 256: the frame lost
                // what the pre-staged misses had gained, profiles/r05_experiments.txt item 3.)
                uint32_t mine_n = 0;
#pragma unroll
                for (uint32_t j = 0; j < WF_SHADE_SWEEP; ++j) mine_n += (word[j] != WF_HIT_PENDING && word[j] != 0xffffffffu) ? 1u : 0u;
                uint32_t before = 0, in_wave = 0;
#pragma unroll
                for (uint32_t b = 0; b < 3u; ++b) {
                    const unsigned long long m = __ballot((mine_n >> b) & 1u);
                    before += wf_lane_rank(m) << b;
                    in_wave += (uint32_t)__popcll(m) << b;
                }
                if ((threadIdx.x & 63u) == 0) agg_cnt[wave] = in_wave;
                __syncthreads();
                uint32_t pos = have + before, total = 0;
                for (uint32_t k = 0; k < WF_SHADE_THREADS / 64; ++k) {
                    if (k < wave) pos += agg_cnt[k];
                    total += agg_cnt[k];
                }
#pragma unroll
                for (uint32_t j = 0; j < WF_SHADE_SWEEP; ++j)
                    if (word[j] != WF_HIT_PENDING && word[j] != 0xffffffffu) agg[pos++] = e0 + j;
                have += total;
                __syncthreads();
            }
            if (have == 0) break;
            const uint32_t take = have < WF_SHADE_THREADS ? have : (uint32_t)WF_SHADE_THREADS;
            have -= take;
            uint32_t mine = threadIdx.x < take ? agg[have + threadIdx.x] : 0u;
            __syncthreads();
            if (!LEAN1 && (W.sort_octants & 2u)) {
                // Material sorting (measured option, PT_WF_SORT=2): the 256 hits of a step are ordered by the model -
                // i.e. the material - of the primitive they hit (8 classes, stable counting sort: ballot per class,
                // mbcnt rank, prefix over classes and waves in LDS), so that a wavefront shades one material's
                // texture set.  The order in which paths are shaded is free: no bit changes.
                __shared__ uint32_t agg_sorted[WF_SHADE_THREADS];
                uint32_t key = 8u, rank = 0u;
                if (threadIdx.x < take) {
                    const uint32_t prim = entry_word(mine) & 0x0fffffffu;
                    key = __float_as_uint(S.prim_attr[(size_t)prim * 4 + 3].w) & 7u;
                }
#pragma unroll
                for (uint32_t k = 0; k < 8u; ++k) {
                    const unsigned long long m = __ballot(key == k);
                    if ((threadIdx.x & 63u) == 0) sh_oct[k][wave] = (uint32_t)__popcll(m);
                    if (key == k) rank = wf_lane_rank(m);
                }
                __syncthreads();
                if (threadIdx.x < 8u * (WF_SHADE_THREADS / 64)) {
                    uint32_t before = 0;
                    for (uint32_t j = 0; j < threadIdx.x; ++j) before += sh_oct[j / (WF_SHADE_THREADS / 64)][j % (WF_SHADE_THREADS / 64)];
                    sh_oct_off[threadIdx.x / (WF_SHADE_THREADS / 64)][threadIdx.x % (WF_SHADE_THREADS / 64)] = before;
                }
                __syncthreads();
                if (threadIdx.x < take) agg_sorted[sh_oct_off[key][wave] + rank] = mine;
                __syncthreads();
                mine = threadIdx.x < take ? agg_sorted[threadIdx.x] : 0u;
                __syncthreads();
            }
            shade_one(mine, threadIdx.x < take);
        }
    }
    if constexpr (NEXT) {   // (threads 0 and 2: the words they alone wrote)
        // the elided count as records of the next queue: the frame plan sizes by written + elided
        if (threadIdx.x == 2 && sh_cnt[3][2]) {
            atomicAdd(&ctr[W.bounce + 1].elided_count, sh_cnt[3][2]);
            atomicAdd(next_ctr + 2, (unsigned long long)sh_cnt[3][2]);
        }
        if (threadIdx.x == 0 && sh_cnt[3][0]) atomicAdd(next_ctr + 1, (unsigned long long)sh_cnt[3][0]);
        // (CONT_LOAD) the workgroup cast for a light of unknown visibility: next_ctr[8] counts such workgroups.  (Written by the
        // lanes that cast, in front of their step's barriers: visible to thread 1 here.)
        if constexpr (CONT_LOAD && !LEAN) {
            if (threadIdx.x == 1 && sh_cnt[3][1]) atomicAdd(next_ctr + 8, 1ull);
        }
    }
    if constexpr (VIS1) {   // (threads 0-3: the words they alone wrote; next_ctr: pt_scene::hit2_unknown)
        const uint32_t mine_acc = threadIdx.x < 4u ? fused_acc[threadIdx.x] : 0u;
        if (threadIdx.x == 0 && NEXT1 && mine_acc) atomicAdd(next_ctr + 1, (unsigned long long)mine_acc);
        if (threadIdx.x == 1 && mine_acc) atomicAdd(next_ctr + 5, (unsigned long long)mine_acc);
        if (threadIdx.x == 2 && mine_acc) {   // as records of the next queue: the frame plan sizes by written + elided
            atomicAdd(&ctr[W.bounce + 1].elided_count, mine_acc);
            atomicAdd(next_ctr + 2, (unsigned long long)mine_acc);
        }
        if (threadIdx.x == 3 && mine_acc) {   // ... and as records of this bounce's shadow queue
            atomicAdd(&ctr[W.bounce].inlined_count, mine_acc);
            atomicAdd(next_ctr + 4, (unsigned long long)mine_acc);
        }
    }
    if (COUNT && n_draws) atomicAdd(&gctr->rng_draws, (unsigned long long)n_draws);
    if (COUNT && n_new) atomicAdd(&gctr->samples, (unsigned long long)n_new);
    if (COUNT && n_moot) {
        atomicAdd(&gctr->shadow_rays, (unsigned long long)n_moot);
        atomicAdd(&gctr->shadow_skipped, (unsigned long long)n_moot);
    }
    if (COUNT && PRIMARY && n_hits) atomicAdd(&gctr->bounce0_hits, (unsigned long long)n_hits);
    if (COUNT && n_masked) {   // (ray_cast calls the reference makes and this pipeline proves empty)
        atomicAdd(&gctr->segments, (unsigned long long)n_masked);
        atomicAdd(&gctr->masked_casts, (unsigned long long)n_masked);
        if (PRIMARY) atomicAdd(&gctr->bounce0_masked, (unsigned long long)n_masked);
    }
    if (COUNT && GRID != 0) {
        atomicAdd(&gctr->segments, (unsigned long long)lc.segments);
        atomicAdd(&gctr->shadow_rays, (unsigned long long)lc.shadow_rays);
        atomicAdd(&gctr->tris_tested, (unsigned long long)lc.tris);
        atomicAdd(&gctr->grid_tris, (unsigned long long)lc.tris);
        atomicAdd(&gctr->restarts, (unsigned long long)lc.restarts);
        if (GRID >= 2) {
            atomicAdd(&gctr->trace_tris, (unsigned long long)n_cam_tris);
            atomicAdd(&gctr->bounce0_cam_tris, (unsigned long long)n_cam_tris);
            atomicAdd(&gctr->bounce0_tris, (unsigned long long)lc.tris);
            atomicAdd(&gctr->bounce0_shadow_rays, (unsigned long long)lc.shadow_rays);
        }
        if (ALPHA) atomicAdd(&gctr->shaded_hits, (unsigned long long)lc.shaded);
    }
