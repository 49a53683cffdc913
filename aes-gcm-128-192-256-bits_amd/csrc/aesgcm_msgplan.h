// aesgcm_msgplan.h -- which launches a SINGLE MESSAGE (or a range of one: a shard, a streaming chunk) takes, decided in one place: from a call, the context's rules
// and the addresses of its scratch, msg_plan() writes a MsgPlan -- a short list of k_main / k_body / k_fold / k_combine launches (and the 16-byte clear of the chaining
// value), each with its finished parameter struct and workgroup count.  No HIP call and no aesgcm_ctx: the host runtime walks the plan on a stream (msg_run,
// aesgcm_host.hip: timing, events, generation numbers, the queue sets' toggle, error texts), the CPU harness walks the same plan with its kernel emulators over
// host vectors (tests/host_emul/emul.cpp), and tests/golden/launch_plan_msg.txt pins what it decides, launch by launch (tests/fake_hip/msg_drive.py).
// The fillers of the parameter structs (plan_main, plan_body, plan_body_cyc, plan_fold, plan_combine_*: aesgcm_stream.h) are called as they are.
// HOST ONLY -- no kernel source includes this file -- and NOT self-contained: the kernels' launch geometry (AESGCM_BODY_WG, AESGCM_BODYH_WG, FOLD_CLOSE_MAX_WGS) and
// the ABI's codes come from aesgcm_internal.h, which the includer has in front.
#pragma once
#include <string.h>

// What the call is after.  TAG, CARRY and POLY take the same launches over the range and differ in the closing k_combine alone.
enum MsgGoal {
    MSG_TAG,        // the tag of a whole message, into the tag slot (crypt_dev)
    MSG_CARRY,      // Y' = Y H^blocks ^ P(range) into the chaining value *dst (streaming sessions, the pipelined path, the pieces of a large range)
    MSG_POLY,       // P(range) H^after into *dst (aesgcm_shard_crypt_dev, aesgcm_ghash)
    MSG_RAW,        // no GHASH at all: one k_main launch (MODE_KS, MODE_ECB)
    MSG_PROBE       // k_body's dealt chunks over a virtual range and the k_fold levels behind them, nothing else (aesgcm_ctx_ceiling_probe)
};
struct MsgCall {
    MsgGoal goal; int mode;
    const uint8_t *iv; const void *aad; u64 aad_len; const void *in; u64 len; void *out; u64 first_block;
    uint4 *dst; u64 after;             // CARRY, POLY: where the result goes; POLY: the exponent
    bool main_only;                    // the range is one k_main launch whatever its size (what came through the staging buffers; aesgcm_ghash)
};
// the context's options, copied
struct MsgRules {
    u32 G, tw; u64 body_min;
    bool cyc_capable, cyc_fuse, fold_close; int cyc_half; u32 cyc_prio;
    u64 cyc_min, cyc_min_fused, cyc_half_max, cyc_max, cyc_max_fused, cyc_max_pieces;
};
// the context's scratch: addresses the launches carry, never dereferenced here.  parts holds what the last plan asked for (MsgPlan::parts_need)
struct MsgScratch {
    uint4 *parts, *fold_a, *fold_b;
    uint4 *tag;                        // four slots: [0] the tag, [1] a session's chaining value, [2] a large range's, [3] E_K(IV || 1) between launches
    uint4 *tag_host;                   // the pinned host slot (device address)
    u32 *counter[2]; u32 qset;         // the two sets of chunk queues, and which one the next dealt launch uses
    unsigned long long *cyc;           // accumulators of the in-launch closings
    const uint4 *ptab;                 // KeyMaterial::ptab
};
struct MsgStep {
    enum Kind { CLEAR, MAIN, BODY, FOLD, COMBINE } kind;
    int mode; u32 wgs;
    bool measured;                     // MAIN, BODY: the launch the context's timing, trace and last_np are about (not the head or tail beside a k_body launch)
    bool dealt;                        // MAIN, BODY: takes its chunks from the queues -- the next launch uses the other set
    bool publishes;                    // the launch leaves a result in the host slot: it takes a generation number (given back when the launch fails)
    union { uint4 *clear; MainParams m; BodyParams b; FoldParams f; CombineParams c; };
};
#define MSG_MAX_STEPS 20               /* clear, then head, body and tail at k_main / k_body + three k_fold levels + k_combine each, then the closing k_combine: 17 */
struct MsgPlan {
    MsgStep step[MSG_MAX_STEPS]; u32 n;
    int rc;                            // what the call returns once the steps have run (a refusal may stand behind launches already planned, as it stood behind them when they were made one by one)
    u32 fold_overflow;                 // rc = AESGCM_EHIP: output items of the k_fold level that fit no buffer
    size_t parts_need;                 // items of `parts` the steps write: the caller grows the buffer and plans again when it holds fewer
    int shape;                         // MSG_TAG: AESGCM_LAUNCH_* for aesgcm_ctx_last_launch
};

// the items a launch (and the k_fold levels behind it) left for k_combine
struct MsgItems { const uint4 *ptr; u32 np; u64 eA; const uint4 *tail_item; u32 tail_blocks; bool closed, ej0; };   // closed: the launch finished the tag itself; ej0: E_K(IV || 1) is in tag[3]

template <class InFlight>
struct MsgPlanner {
    MsgPlan &pl; const MsgCall &c; const MsgRules &r; const MsgScratch &s; InFlight &others_in_flight; u32 qset;

    MsgStep &add(MsgStep::Kind kind, int mode = 0) {
        MsgStep &t = pl.step[pl.n++];
        t.kind = kind; t.mode = mode; t.wgs = 1; t.measured = true; t.dealt = t.publishes = false;
        return t;
    }
    void need(size_t items) { if (items > pl.parts_need) pl.parts_need = items; }
    const uint4 *tab(u64 e) const { const int k = ptab_index(e); return k < 0 ? nullptr : s.ptab + (size_t)k * 512; }
    static bool unaligned(const void *in, const void *out) { return (((uintptr_t)in | (uintptr_t)out) & 15) != 0; }
    // THE rule for the end of folding: k_combine takes up to 64 items unfolded when their spacing has precomputed tables (H^eA, and H^(4 eA), H^(16 eA) for its second and third level)
    bool combine_takes(u32 n, u64 eA) const { return n == 1 || (n <= COMBINE_MAX_ITEMS && tab(eA) && (n <= 4 || tab(4 * eA)) && (n <= 16 || tab(16 * eA))); }

    // k_fold levels over n items (period, eA, eB as in FoldParams) until k_combine can take what is left.  close: a level of at most FOLD_CLOSE_MAX_WGS workgroups closes
    // the tag itself -- every closing workgroup stages the lanes' tables (33 KB) and spends ~4 us: the 256 workgroups of a 1 GiB message's first level are one round on
    // the chip and the step gains 11 us (cfg2: 976 -> 963 us); the 2048 of 16 GiB would be eight rounds and cost what they save (profiles/archive/r03c/fold_close_ab.txt),
    // so there the first level stays plain and the second (64 workgroups) closes
    MsgItems fold(const uint4 *items, u32 n, u32 period, u64 eA, u64 eB, const FoldClose *close) {
        const uint4 *cur = items;
        int which = 0;
        while (period > 1 || !combine_takes(n, eA)) {
            MsgStep &t = add(MsgStep::FOLD);
            FoldParams &f = t.f;
            plan_fold(f, cur, which ? s.fold_b : s.fold_a, n, period, eA, eB);
            f.tabA = tab(f.eA); f.tabB = tab(f.eB); f.tabC = tab(f.eC);
            const u32 G = t.wgs = fold_wgs(n, f.group);
            if (close && G <= FOLD_CLOSE_MAX_WGS) {
                f.close = *close;
                f.close.on = 1; f.close.step = fold_out_step(f);
                t.publishes = true;
                return MsgItems{nullptr, 0, 0, nullptr, 0, true, true};
            }
            if (G > (which ? FOLD_B_ITEMS : FOLD_A_ITEMS)) { --pl.n; pl.rc = AESGCM_EHIP; pl.fold_overflow = G; break; }
            eA = fold_out_step(f); eB = 0; period = 1;
            cur = f.out; n = G; which ^= 1;
        }
        return MsgItems{cur, n, n > 1 || cur == items ? eA : 0, nullptr, 0, false, true};      // (one folded item has no spacing)
    }
    // the fused kernel over (aad, data) and the k_fold levels over its chunk items.  items: GHASH partials are wanted; want_tail: a single chunk closes the tag itself
    MsgItems main(int mode, const void *aad, u64 aad_len, const void *in, u64 len, void *out, u64 first_block, bool items, bool want_tail, bool measured) {
        const MsgItems none = {nullptr, 0, 0, nullptr, 0, false, false};
        const bool gh = mode == MODE_ENC || mode == MODE_DEC;
        if (unaligned(in, out)) { pl.rc = AESGCM_EALIGN; return none; }
        MsgStep &t = add(MsgStep::MAIN, mode);
        MainParams &p = t.m;
        memset(&p, 0, sizeof p);
        const u32 C = plan_main(p, mode, r.tw, c.iv, aad, aad_len, in, len, out, first_block, nullptr);
        if (!C) { --pl.n; return none; }
        if (gh) need(C);
        p.parts = s.parts;
        t.wgs = (C + 1 + AESGCM_MAIN_WG / 64 - 1) / (AESGCM_MAIN_WG / 64);          // one wave per chunk is enough for small inputs (+ one spare for E_K(J0))
        if (t.wgs > r.G) t.wgs = r.G;
        plan_queues(C, &p.nq, &p.seg);
        if ((u64)t.wgs * (AESGCM_MAIN_WG / 64) >= (u64)C + 1) p.nq = 0;              // a wave per chunk and a spare: static assignment, the dispensers are not touched
        p.counter = s.counter[qset]; p.counter_zero = s.counter[qset ^ 1u];
        t.measured = measured;
        if ((t.dealt = p.nq != 0)) qset ^= 1u;                                        // the launch leaves the other set zeroed for the next dealt one
        if (!gh || !items) return none;
        p.ej0 = s.tag + 3;
        if (want_tail && C == 1) {                                                    // k_main's tail leaves the tag in the slot and in the host slot
            p.tail = 1; p.tag_out = s.tag; p.tag_host = s.tag_host; t.publishes = true;
            return MsgItems{nullptr, 0, 0, nullptr, 0, true, true};
        }
        return fold(s.parts, C, 1, (u64)64 * p.Tw, 0, nullptr);
    }
    // k_body over the planned split + the k_fold levels over its interleaved chunk items
    MsgItems body(int mode, const BodySplit &b, const void *in, void *out, u64 first_block, const FoldClose *close) {
        MsgStep &t = add(MsgStep::BODY, mode);
        BodyParams &p = t.b;
        memset(&p, 0, sizeof p);
        need((size_t)4 * b.S);
        plan_body(p, b, c.iv, in, out, first_block, s.parts);
        p.ej0 = s.tag + 3;
        const u32 waves_per_wg = AESGCM_BODY_WG / 64;
        t.wgs = (p.C + waves_per_wg - 1) / waves_per_wg;
#if AESGCM_T4
        if (t.wgs > r.G / 2) t.wgs = r.G / 2;                                         // one 136 KiB workgroup per CU
#else
        if (t.wgs > r.G) t.wgs = r.G;
#endif
        plan_queues(p.C, &p.nq, &p.seg);
        p.counter = s.counter[qset]; p.counter_zero = s.counter[qset ^ 1u];
        t.dealt = true; qset ^= 1u;
        // items 4s + v: phases 64 blocks apart inside a super-chunk, super-chunks 256 T blocks apart
        return fold(s.parts, p.C, 4, 64, (u64)256 * b.T, close);
    }
    // A whole range -- AAD, data from any first block, ragged end -- as ONE k_body launch of cyclic rows (plan_body_cyc) and the k_fold level over its 4096 items, when
    // the range is of that size (whether it was).  whole: the range is a whole message, whose launch closes the tag itself (cyc_close)
    bool cyc(int mode, const void *aad, u64 aad_len, const void *in, u64 len, void *out, u64 first_block, bool whole, MsgItems *it) {
        const bool fused = whole && r.cyc_fuse;
        if (!r.cyc_capable || len < (fused ? r.cyc_min_fused : r.cyc_min)) return false;
        if (unaligned(in, out)) return false;                                         // the caller's other path reports the alignment
        // a range with pieces around its body (AAD, an odd first block, a ragged end) costs the other paths a launch pair per piece (+45 .. 80 us,
        // profiles/archive/r03c/general_shape.txt): for those the cyclic launch stays ahead for longer
        const bool pieces = aad_len || (first_block & 255) || (len & 1023);
        const u64 lo = fused ? r.cyc_min_fused : r.cyc_min, hi = pieces ? r.cyc_max_pieces : fused ? r.cyc_max_fused : r.cyc_max;
        const bool half = fused && len < r.cyc_half_max && (r.cyc_half == 1 || (r.cyc_half == 2 && others_in_flight()));   // two workgroups per CU: for messages in flight beside each other
        MsgStep &t = add(MsgStep::BODY, mode);
        BodyParams &p = t.b;
        if (!plan_body_cyc(p, mode, c.iv, aad, aad_len, in, len, out, first_block, s.parts, lo, hi, half ? BODY_CYC_WAVES_HALF : BODY_CYC_WAVES)) { --pl.n; return false; }
        need((size_t)BODY_CYC_WAVES + 1);
        if (whole) pl.shape = half ? AESGCM_LAUNCH_CYCLIC_HALF : AESGCM_LAUNCH_CYCLIC;
        p.prio_rows = r.cyc_prio;
        t.wgs = half ? BODY_CYC_WAVES_HALF / (AESGCM_BODYH_WG / 64) : BODY_CYC_WAVES / (AESGCM_BODY_WG / 64);
        if (fused) {                                                                  // the launch closes the tag itself: nothing behind it
            p.fuse = 1; p.aad_len = aad_len; p.ct_len = len; p.acc = s.cyc;
            p.tag_out = s.tag; p.tag_host = s.tag_host; t.publishes = true;
            *it = MsgItems{nullptr, 0, 0, nullptr, 0, true, true};
            return true;
        }
        p.ej0 = s.tag + 3;
        *it = fold(s.parts, BODY_CYC_WAVES, 1, 64, 0, nullptr);                       // always BODY_CYC_WAVES items, 64 blocks apart
        if (p.tb) { it->tail_item = s.parts + (size_t)BODY_CYC_WAVES * 64; it->tail_blocks = p.tb; }
        return true;
    }
    // k_combine over the items: their spacing and its tables
    void combine(CombineParams q, const MsgItems &it) {
        q = combine_with_items(q, it.eA, it.tail_item, it.tail_blocks);
        if (q.kind == PARTS_ITEM && q.np > 1) { q.tabA = tab(q.eA); q.tabB = q.np > 4 ? tab(4 * q.eA) : nullptr; q.tabC = q.np > 16 ? tab(16 * q.eA) : nullptr; }
        MsgStep &t = add(MsgStep::COMBINE);
        if ((t.publishes = q.out == s.tag)) q.out_host = s.tag_host;                  // results that go to the tag slot are mirrored to the pinned host slot
        t.c = q;
    }
    void carry(const MsgItems &it, uint4 *state, u64 nb) { combine(plan_combine_carry(it.ptr, it.np, PARTS_ITEM, state, nb), it); }
    // Y' = Y * H^nb ^ P(aad, data) for a whole range, Y in *state.  Large ranges go head / k_body / tail, each piece folded into the state in order; small ones are a
    // single k_main launch.  Whether a launch left E_K(IV || 1) behind for the call's last k_combine
    bool range(const void *aad, u64 aad_len, const unsigned char *in, u64 len, unsigned char *out, u64 first_block, uint4 *state) {
        const u64 n_aad = (aad_len + 15) / 16, nb = n_aad + (len + 15) / 16;
        MsgItems it;
        BodySplit b;
        if (!c.main_only && cyc(c.mode, aad, aad_len, in, len, out, first_block, false, &it)) {      // mid-size ranges: the whole range in one k_body launch of cyclic rows
            if (!pl.rc) carry(it, state, nb);
            return true;
        }
        if (c.main_only || !plan_body_split(len, first_block, r.tw, r.body_min, &b)) {
            it = main(c.mode, aad, aad_len, in, len, out, first_block, true, false, true);
            if (!pl.rc && nb) carry(it, state, nb);
            return false;
        }
        if (unaligned(in, out)) { pl.rc = AESGCM_EALIGN; return false; }
        if (n_aad + b.head_blocks) {
            it = main(c.mode, aad, aad_len, in, 16 * b.head_blocks, out, first_block, true, false, false);
            if (pl.rc) return false;
            carry(it, state, n_aad + b.head_blocks);
        }
        it = body(c.mode, b, in, out, first_block, nullptr);
        if (pl.rc) return true;
        carry(it, state, b.body_blocks);
        const u64 done = b.head_blocks + b.body_blocks, tail = len - 16 * done;
        if (tail) {
            it = main(c.mode, nullptr, 0, in + 16 * done, tail, out + 16 * done, first_block + done, true, false, false);
            if (!pl.rc) carry(it, state, (tail + 15) / 16);
        }
        return true;
    }
    // the closing k_combine of TAG and POLY over the items of the range's one launch
    void close(const MsgItems &it) {
        if (pl.rc || it.closed) return;
        CombineParams q = c.goal == MSG_TAG ? plan_combine_tag(it.ptr, it.np, PARTS_ITEM, c.iv, c.aad_len, c.len, s.tag) : plan_combine_poly(it.ptr, it.np, PARTS_ITEM, c.after, c.dst);
        if (c.goal == MSG_TAG && it.ej0) q.ej0 = s.tag + 3;                           // same IV, same stream: the launch left E_K(IV || 1) behind
        combine(q, it);
    }
    void plan() {
        const unsigned char *in = (const unsigned char *)c.in;
        unsigned char *out = (unsigned char *)c.out;
        BodySplit b;
        MsgItems it;
        if (c.goal == MSG_RAW) { main(c.mode, nullptr, 0, in, c.len, out, c.first_block, false, false, true); return; }
        if (c.goal == MSG_PROBE) { if (plan_body_split(c.len, 0, r.tw, 0, &b)) body(c.mode, b, in, out, 0, nullptr); else pl.rc = AESGCM_EARG; return; }
        if (c.goal == MSG_CARRY) { range(c.aad, c.aad_len, in, c.len, out, c.first_block, c.dst); return; }
        const bool whole = c.goal == MSG_TAG;
        if (!c.main_only && cyc(c.mode, c.aad, c.aad_len, in, c.len, out, c.first_block, whole, &it)) {   // mid-size: cyclic rows take AAD, data and the ragged end in one launch
            close(it);
            return;
        }
        if (!c.main_only && plan_body_split(c.len, c.first_block, r.tw, r.body_min, &b)) {
            pl.shape = AESGCM_LAUNCH_DEALT;
            if (!c.aad_len && !b.head_blocks && c.len == 16 * b.body_blocks) {
                // the whole range is one aligned body (the benchmark's shape; the 8-GPU job's shards): no chaining value to carry, k_body's items go straight to the
                // result -- and a whole message's tag comes out of k_fold (when there is a k_fold launch at all)
                FoldClose fc = {};
                fc.ct_len = c.len; fc.ej0 = s.tag + 3; fc.acc = s.cyc; fc.tag_out = s.tag; fc.tag_host = s.tag_host;
                close(body(c.mode, b, in, out, c.first_block, whole && r.fold_close ? &fc : nullptr));
                return;
            }
            // large: head / k_body / tail folded into a device-side chaining value, then the result from it
            uint4 *state = s.tag + 2;
            add(MsgStep::CLEAR).clear = state;
            const bool ej0 = range(c.aad, c.aad_len, in, c.len, out, c.first_block, state);
            if (pl.rc) return;
            CombineParams q = whole ? plan_combine_final(state, c.iv, c.aad_len, c.len, s.tag) : plan_combine_poly(nullptr, 0, PARTS_NONE, 0, c.dst);
            if (whole) q.ej0 = ej0 ? s.tag + 3 : nullptr;                            // left by k_body (every piece of this message writes the same value)
            else { q.carry = state; q.has_carry = 1; q.e_carry = c.after; }           // W = Y * H^after
            combine(q, MsgItems{});
            return;
        }
        pl.shape = AESGCM_LAUNCH_MAIN;
        close(main(c.mode, c.aad, c.aad_len, in, c.len, out, c.first_block, true, whole, true));     // (a single chunk: k_main's tail closes)
    }
};

// others_in_flight(): is a message of another context of the device under way -- asked only where the half shape of the cyclic rows hangs on it (cyc_half = 2)
template <class InFlight>
static inline void msg_plan(MsgPlan &pl, const MsgCall &c, const MsgRules &r, const MsgScratch &s, InFlight &&others_in_flight) {
    pl.n = 0; pl.rc = AESGCM_OK; pl.fold_overflow = 0; pl.parts_need = 0; pl.shape = AESGCM_LAUNCH_NONE;
    MsgPlanner<InFlight> p = {pl, c, r, s, others_in_flight, s.qset};
    p.plan();
}
