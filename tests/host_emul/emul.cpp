// CPU harness: runs the SAME per-lane code the HIP kernels run (csrc/aesgcm_dev.h is __host__
// __device__) over an emulated launch -- LDS image, workgroup/lane geometry, front padding, Horner
// with K, per-lane tail powers, workgroup fold, k_combine fold -- and compares ciphertext and tag with
// the oracle (oracle/aesgcm_oracle.c, linked in).  It exists because the build container has no GPU:
// it pins the arithmetic and the index algebra before any GPU minute is spent.  Test infrastructure only.
#include "../../aes-gcm-128-192-256-bits_amd/csrc/aesgcm_internal.h"      // (the kernels' launch geometry, as the launchers see it; the lane code through aesgcm_dev.h, aesgcm_rows.h)
#include "../../aes-gcm-128-192-256-bits_amd/csrc/aesgcm_msgplan.h"
#include "aesgcm_bs.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <stdint.h>
#include <algorithm>
#include <vector>

extern "C" {
int orc_key_expand(const uint8_t *key, size_t key_len, uint8_t *rk, int *nr);
int orc_aes_encrypt_block(const uint8_t *rk, int nr, const uint8_t in[16], uint8_t out[16]);
void orc_gfmul(const uint8_t h[16], const uint8_t x[16], uint8_t z[16]);
int orc_gcm_crypt(int dec, const uint8_t *key, size_t key_len, const uint8_t iv[12], const uint8_t *aad, size_t aad_len,
                  const uint8_t *in, size_t len, uint8_t *out, uint8_t tag[16]);
void orc_ghash_update(const uint8_t h[16], uint8_t y[16], const uint8_t *data, size_t len);
void orc_fill_splitmix64(uint8_t *buf, size_t len, uint64_t seed, uint64_t first_word);
uint8_t orc_sbox(uint8_t x);
}

static int g_fail = 0;
#define CHECK(cond, ...) do { if (!(cond)) { g_fail++; printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } while (0)

static DevTables g_tb;
static void init_tables() { for (u32 x = 0; x < 256; x++) { u32 s = sbox_calc(x); g_tb.sbox[x] = (uint8_t)s; g_tb.te0[x] = te0_calc(s); g_tb.te1[x] = rotl32(te0_calc(s), 8); g_tb.te2[x] = rotl32(te0_calc(s), 16); g_tb.te3[x] = rotl32(te0_calc(s), 24); } }

// emulated k_setup (same barrier structure: compute every lane's product, then commit)
static void emu_setup(KeyMaterial *km, const uint8_t *key, int key_len, int pre_nr, u32 G) {
    static uint4 tab[AESGCM_NPW];
    setup_lane0(km, g_tb.sbox, key, key_len, pre_nr, G, tab);
    for (int d = 0; d < 4; d++) {
        for (int j = 0; j < AESGCM_LOG_WG; j++) {
            static uint4 prod[AESGCM_WG]; static bool act[AESGCM_WG];
            for (int tid = 0; tid < AESGCM_WG; tid++) act[tid] = setup_level(tab, j, tid, &prod[tid]);
            for (int tid = 0; tid < AESGCM_WG; tid++) if (act[tid]) tab[(1 << j) + tid] = prod[tid];
        }
        for (int k = 0; k < AESGCM_NPW; k++) km->pw[d][k] = tab[k];
        if (d == 1) for (int tid = 0; tid < AESGCM_WG; tid++) setup_beta_lane(km, tab, tid);
        if (d < 3) { uint4 next = tab[AESGCM_WG]; tab[0] = gf_one_mo(); tab[1] = next; }
    }
    for (u32 k = 0; k < AESGCM_NPTAB; k++) for (u32 tid = 0; tid < 512; tid++) setup_ptab_lane(km, k, tid);
    for (u32 e = 0; e < AESGCM_NLTAB; e++) for (u32 tid = 0; tid < 32; tid++) setup_ltab_lane(km, e, tid);
}

static void xor_g(G128 &a, const G128 &b) { for (int k = 0; k < 4; k++) a.w[k] ^= b.w[k]; }

template <int NR, int MODE>
static void emu_main_nr(const KeyMaterial *km, const MainParams &p) {
    static unsigned char smem[AESGCM_LDS_BYTES] __attribute__((aligned(16)));
    constexpr bool GH = (MODE == MODE_ENC || MODE == MODE_DEC);
    for (u32 tid = 0; tid < AESGCM_MAIN_WG; tid++) main_fill_lds(smem, km, &g_tb, tid, GH);   // image is workgroup independent
    // the dispenser hands chunk c to whichever wave asks next; results do not depend on who that is, so the
    // harness walks the chunks in a scrambled order to make any accidental order dependence visible
    for (u32 k = 0; k < p.C; k++) {
        const u32 c = (p.C - 1) - k;      // reverse order
        for (u32 lane = 0; lane < 64; lane++) {
            const CtrConsts cc = main_lane_consts<MODE>(km, p, smem, lane);
            uint4 acc = main_chunk_lane<NR, MODE>(km, p, smem, cc, c, lane);
            if (GH) p.parts[(size_t)c * 64 + lane] = acc;
        }
    }
}
static void emu_main(int mode, const KeyMaterial *km, const MainParams &p) {
#define D(NR) switch (mode) { case MODE_ENC: emu_main_nr<NR, MODE_ENC>(km, p); break; case MODE_DEC: emu_main_nr<NR, MODE_DEC>(km, p); break; \
                              case MODE_KS: emu_main_nr<NR, MODE_KS>(km, p); break; default: emu_main_nr<NR, MODE_ECB>(km, p); }
    if (km->nr == 10) { D(10) } else if (km->nr == 12) { D(12) } else { D(14) }
#undef D
}
// emulated cyc_close(): the fused closing of a cyclic launch, workgroup by workgroup with the same lane pieces (tree levels, lane terms from the staged
// tables, the weight through a two-table Shoup form, the terms that occur once in workgroup 0); the accumulator slots are plain XORs here
static void emu_cyc_close(const KeyMaterial *km, const BodyParams &p, const uint4 *items, const uint4 *last, uint4 ej0) {
    static unsigned char smem[CYC_LDS_END] __attribute__((aligned(16)));
    const u32 wgs = BODY_CYC_WAVES / 16;
    G128 slots[CYC_ACC_SLOTS];
    memset(slots, 0, sizeof slots);
    u32 arrived = 0;
    for (u32 gg = 0; gg < wgs; gg++) {
        const u32 g = (gg * 37u + 5u) % wgs;                               // any arrival order
        for (u32 tid = 0; tid < 1024; tid++) {
            reinterpret_cast<uint4 *>(smem + CYC_LDS_TREE_TAB)[tid] = (&km->ptab[0][0])[tid];
            reinterpret_cast<uint4 *>(smem + CYC_LDS_TREE_TAB)[1024u + tid] = (&km->ptab[0][0])[1024u + tid];
            for (u32 k = tid; k < 2048; k += 1024) {
                *reinterpret_cast<uint4 *>(smem + cyc_ltab_off(k)) = cyc_ltab_entry(km, k, p.tb);
                if (g == 0 && p.tb) *reinterpret_cast<uint4 *>(smem + cyc_ltab_off(k, CYC_LDS_LTAB0)) = cyc_ltab_entry(km, k, 0u);
            }
            *reinterpret_cast<uint4 *>(smem + cyc_stage_off(0) + (tid >> 6) * 1024u + (tid & 63u) * 16u) = items[(size_t)(16 * g + (tid >> 6)) * 64 + (tid & 63u)];
        }
        uint4 y[64];
        for (u32 level = 0; level < 4; level++)
            for (u32 wv = 0; wv < (8u >> level); wv++) for (u32 lane = 0; lane < 64; lane++) {
                const uint4 v = cyc_tree_lane(smem, level, wv, lane);
                if (level < 3) *reinterpret_cast<uint4 *>(smem + cyc_stage_off(level + 1) + wv * 1024u + lane * 16u) = v; else y[lane] = v;
            }
        G128 z = {{0, 0, 0, 0}};
        for (u32 lane = 0; lane < 64; lane++) xor_g(z, cyc_lane_term_lds(smem, y[lane], lane));
        if (g + 1 != wgs) {
            for (u32 lane = 0; lane < 32; lane++) *reinterpret_cast<uint4 *>(smem + CYC_LDS_WTAB + 16u * lane) = shoup2_entry(mo_to_be(km->pw[1][wgs - 1 - g]), lane);
            z = shoup2_gmul_lds(z, reinterpret_cast<const uint4 *>(smem + CYC_LDS_WTAB));
        }
        if (g == 0) {
            if (p.tb) for (u32 lane = 0; lane < 64; lane++) xor_g(z, cyc_lane_term_lds(smem, last[lane], lane, CYC_LDS_LTAB0));
            xor_g(z, tag_len_term(km, p.aad_len, p.ct_len));
            xor_g(z, mo_to_be(ej0));
        }
        xor_g(slots[g & (CYC_ACC_SLOTS - 1u)], z);
        ++arrived;
    }
    CHECK(arrived == wgs, "cyc_close arrivals");
    G128 t = {{0, 0, 0, 0}};
    for (u32 k = 0; k < CYC_ACC_SLOTS; k++) xor_g(t, slots[k]);
    *p.tag_out = be_to_mo(t);
}
template <int NR, int MODE>
static void emu_body_nr(const KeyMaterial *km, const BodyParams &p) {
    static unsigned char smem[AESGCM_LDS_BYTES_T4] __attribute__((aligned(16)));
    for (u32 tid = 0; tid < AESGCM_MAIN_WG; tid++) main_fill_lds(smem, km, &g_tb, tid, true, AESGCM_MAIN_WG, p.cyc ? GH_TAB_K2P18 : GH_TAB_K256);
#if AESGCM_T4
    for (u32 tid = 0; tid < AESGCM_MAIN_WG; tid++) fill_lds_t4(smem, &g_tb, tid, AESGCM_MAIN_WG);     // second table region (T1 | T3)
#endif
    if (p.cyc) {                                                        // cyclic rows: one strand and one item per wave (k_body<.., true>)
        for (u32 k = 0; k < BODY_CYC_WAVES; k++) {
            const u32 w = (k * 2741u + 17u) % BODY_CYC_WAVES;           // scrambled order (2741 is odd: a permutation)
            for (u32 lane = 0; lane < 64; lane++) {
                const CtrConsts cc = ctr_round1_consts(p.iv0, p.iv1, p.iv2, km->rk, smem, (lane & 31u) << 2);
                p.parts[(size_t)w * 64 + lane] = body_cyc_lane<NR, MODE>(km, &g_tb, p, smem, cc, w, lane);
                if (w == 0 && p.tb) p.parts[(size_t)BODY_CYC_WAVES * 64 + lane] = body_cyc_last_lane<NR, MODE>(km, p, smem, cc, lane);
            }
        }
        if (p.fuse) {                                                   // the launch closes the tag itself
            const CtrConsts cc = ctr_round1_consts(p.iv0, p.iv1, p.iv2, km->rk, smem, 0);
            u32 s0, s1, s2, s3;
            ctr_rounds_lds<NR>(bswap32(1u), cc, s0, s1, s2, s3, km->rk, smem, 0);
            emu_cyc_close(km, p, p.parts, p.parts + (size_t)BODY_CYC_WAVES * 64, make_uint4(s0, s1, s2, s3));
        }
        return;
    }
    for (u32 k = 0; k < p.C; k++) {
        const u32 c = (k * 7 + 3) % p.C == k ? k : (p.C - 1) - k;      // scrambled order (any permutation will do)
        for (u32 lane = 0; lane < 64; lane++) {
            const CtrConsts cc = ctr_round1_consts(p.iv0, p.iv1, p.iv2, km->rk, smem, (lane & 31u) << 2);
            p.parts[(size_t)c * 64 + lane] = body_chunk_lane<NR, MODE>(km, &g_tb, p, smem, cc, c, lane);
        }
    }
}
static void emu_body(int mode, const KeyMaterial *km, const BodyParams &p) {
#define D(NR) if (mode == MODE_DEC) emu_body_nr<NR, MODE_DEC>(km, p); else emu_body_nr<NR, MODE_ENC>(km, p);
    if (km->nr == 10) { D(10) } else if (km->nr == 12) { D(12) } else { D(14) }
#undef D
}
static G128 emu_pow_h(const KeyMaterial *km, u64 e) { return gf_pow_h_serial(km, e); }
// emulated k_combine: the same lane pieces (in-launch item fold, one level of per-lane table multiplies through km->ltab)
static void emu_combine(const KeyMaterial *km, const CombineParams &p0) {
    static unsigned char smem[CMB_LDS_BYTES] __attribute__((aligned(16)));
    const CombineParams &p = p0;
    const bool tag = p.want_tag != 0, items = p.kind == PARTS_ITEM;
    CHECK(!(items && p.np > 1) || (p.np <= COMBINE_MAX_ITEMS && p.tabA && (p.np <= 4 || p.tabB) && (p.np <= 16 || p.tabC)), "emu_combine: %u items not foldable", p.np);
    const u32 J1 = items ? fold4_groups(p.np) : 0, J2 = items ? fold4_groups(J1) : 0;
    if (items && p.np > 1) memcpy(smem + CMB_LDS_TABA, p.tabA, 8192);
    if (J1 > 1) memcpy(smem + CMB_LDS_TABB, p.tabB, 8192);
    if (J2 > 1) memcpy(smem + CMB_LDS_TABC, p.tabC, 8192);
    memcpy(smem + CMB_LDS_SBOX, g_tb.sbox, 256);
    for (u32 w = 0; w < J1; w++) for (u32 lane = 0; lane < 64; lane++)
        *reinterpret_cast<uint4 *>(smem + CMB_LDS_STAGE1 + w * 1024u + lane * 16u) = combine_fold_items(combine_fold_load(p, w, lane), smem, CMB_LDS_TABA);
    for (u32 w = 0; w < J2; w++) for (u32 lane = 0; lane < 64; lane++)
        *reinterpret_cast<uint4 *>(smem + CMB_LDS_STAGE2 + w * 1024u + lane * 16u) = combine_fold_staged(smem, CMB_LDS_STAGE1, J1, w, CMB_LDS_TABB, lane);
    G128 acc = {{0, 0, 0, 0}};
    if (items) {
        for (u32 lane = 0; lane < 64; lane++) xor_g(acc, shoup2_gmul(mo_to_be(combine_fold_staged(smem, CMB_LDS_STAGE2, J2, 0, CMB_LDS_TABC, lane)), km->ltab[(tag ? 65u : 63u) - lane + (p.tail_item ? p.tail_blocks : 0u)]));
        if (p.tail_item) for (u32 lane = 0; lane < 64; lane++) xor_g(acc, shoup2_gmul(mo_to_be(p.tail_item[lane]), km->ltab[(tag ? 65u : 63u) - lane]));
    } else if (p.kind == PARTS_GATHERED) {
        for (u32 tid = 0; tid < p.np; tid++) {
            G128 z = mo_to_be(p.parts[(size_t)tid * (p.stride ? p.stride : 1u)]);
            if (tag) z = shoup2_gmul(z, km->ltab[2]);
            xor_g(acc, z);
        }
    }
    if (tag) {
        xor_g(acc, tag_len_term(km, p.aad_len, p.ct_len));
        xor_g(acc, p.ej0 ? mo_to_be(*p.ej0) : combine_ej0_bytes(km, smem + CMB_LDS_SBOX, p));
        if (p.has_carry && !p.e_carry) xor_g(acc, shoup2_gmul(mo_to_be(*p.carry), km->ltab[2]));
    }
    if (!tag && p.e) acc = gf_mul(acc, emu_pow_h(km, p.e));
    if (p.has_carry && (!tag || p.e_carry)) {
        G128 c = mo_to_be(*p.carry);
        if (p.e_carry) c = gf_mul(c, emu_pow_h(km, p.e_carry));
        if (tag) c = gf_mul(c, mo_to_be(km->pw[0][2]));
        xor_g(acc, c);
    }
    *p.out = be_to_mo(acc);
}

// An emulated context: key material, the planner's rules (the context's options) and host vectors for its scratch.  go() makes the PRODUCT's plan for a call
// (msg_plan, csrc/aesgcm_msgplan.h -- the one aesgcm_host.hip runs on a stream) and walks it with the kernel emulators above.
struct Emu {
    KeyMaterial km;
    // no cyclic rows and no k_body split unless a test asks: every size through k_main.  Cyclic rows, when on, from one whole body row (every size)
    MsgRules rules = {512, 0, ~0ull, false, true, true, 0, 0, 1024, 1024, 0, ~0ull, ~0ull, ~0ull};
    std::vector<uint4> parts, fold_a, fold_b;
    uint4 slots[4];                 // the context's d_tag: tag, a session's chaining value, a large range's, E_K(IV || 1)
    MsgPlan last;                   // the plan of the last call
    Emu(const uint8_t *key, int key_len, u32 tw) : parts(64), fold_a((size_t)64 * FOLD_A_ITEMS), fold_b((size_t)64 * FOLD_B_ITEMS) { rules.tw = tw; emu_setup(&km, key, key_len, 0, 512); }
    template <class F> u32 count(MsgStep::Kind kind, F f) const { u32 n = 0; for (u32 k = 0; k < last.n; k++) n += last.step[k].kind == kind && f(last.step[k]); return n; }
    u32 n_cyc() const { return count(MsgStep::BODY, [](const MsgStep &t) { return t.b.cyc != 0; }); }             // cyclic launches of the last call
    u32 n_body() const { return count(MsgStep::BODY, [](const MsgStep &) { return true; }); }                      // k_body launches of any kind
    u32 n_fold_close() const { return count(MsgStep::FOLD, [](const MsgStep &t) { return t.f.close.on != 0; }); }   // k_fold levels that closed the tag
    // what the launch's chunk-0 wave leaves in the slot for k_combine and the closings
    void leave_ej0(uint4 *ej0, u32 iv0, u32 iv1, u32 iv2) {
        CombineParams q = {};
        q.iv0 = iv0; q.iv1 = iv1; q.iv2 = iv2;
        if (ej0) *ej0 = be_to_mo(combine_ej0_bytes(&km, g_tb.sbox, q));
    }
    // k_fold's closing (FoldClose): the workgroups of the level turn their output items into the tag
    void fold_closing(const FoldParams &f, u32 G) {
        static unsigned char lds[FOLD_LDS_CLOSE_BYTES] __attribute__((aligned(16)));
        for (u32 k = 0; k < 2048; k++) *reinterpret_cast<uint4 *>(lds + cyc_ltab_off(k, FOLD_LDS_LTAB)) = cyc_ltab_entry(&km, k, 0u);
        G128 slots[CYC_ACC_SLOTS];
        memset(slots, 0, sizeof slots);
        for (u32 gg = 0; gg < G; gg++) {
            const u32 g = (gg * 29u + 3u) % G == gg ? gg : G - 1 - gg;      // any arrival order
            G128 z = {{0, 0, 0, 0}};
            for (u32 lane = 0; lane < 64; lane++) xor_g(z, cyc_lane_term_lds(lds, f.out[(size_t)g * 64 + lane], lane, FOLD_LDS_LTAB));
            const u64 e = f.close.step * (u64)(G - 1 - g);
            for (u32 d = 0; d < 4; d++) {
                const u32 dig = (u32)(e >> (AESGCM_LOG_WG * d)) & (u32)(AESGCM_WG - 1);
                if (!dig) continue;
                for (u32 lane = 0; lane < 32; lane++) *reinterpret_cast<uint4 *>(lds + FOLD_LDS_WTAB + 16u * lane) = shoup2_entry(mo_to_be(km.pw[d][dig]), lane);
                z = shoup2_gmul_lds(z, reinterpret_cast<const uint4 *>(lds + FOLD_LDS_WTAB));
            }
            if (g + 1 == G) { xor_g(z, tag_len_term(&km, f.close.aad_len, f.close.ct_len)); xor_g(z, mo_to_be(*f.close.ej0)); }
            xor_g(slots[g & (CYC_ACC_SLOTS - 1u)], z);
        }
        G128 t = {{0, 0, 0, 0}};
        for (u32 k = 0; k < CYC_ACC_SLOTS; k++) xor_g(t, slots[k]);
        *f.close.tag_out = be_to_mo(t);
    }
    // one k_fold level
    void emu_fold(const FoldParams &f, u32 G) {
        static unsigned char smem[FOLD_LDS_BYTES] __attribute__((aligned(16)));
        for (u32 tid = 0; tid < FOLD_WG; tid++) {
            fold_fill_lds(smem, &km, f.tabA, f.eA, 0u, tid, FOLD_WG);
            if (f.period > 1) fold_fill_lds(smem, &km, f.tabB, f.eB, 8192u, tid, FOLD_WG);
            fold_fill_lds(smem, &km, f.tabC, f.eC, 16384u, tid, FOLD_WG);
        }
        for (u32 g = 0; g < G; g++) {
            u32 start, end;
            const u32 J = fold_wg_range(f.n, f.group, g, &start, &end);
            for (u32 w = 0; w < J; w++) for (u32 lane = 0; lane < 64; lane++)
                *reinterpret_cast<uint4 *>(smem + FOLD_LDS_TAB + w * 1024u + lane * 16u) = fold_wave_lane(f, smem, start, end, J, w, lane);
            for (u32 lane = 0; lane < 64; lane++) f.out[(size_t)g * 64 + lane] = fold_wg_lane(smem, J, lane);
        }
        if (f.close.on) { CHECK(f.close.ej0 != nullptr, "fold closing without E_K(J0)"); fold_closing(f, G); }
    }
    // k_main's tail (single-chunk message: no k_combine launch): every term one table multiply deep
    void emu_main_tail(const MainParams &p) {
        G128 P = {{0, 0, 0, 0}};
        for (u32 lane = 0; lane < 64; lane++) xor_g(P, tag_lane_term(&km, p.parts[lane], lane));
        xor_g(P, tag_len_term(&km, p.aad_len, p.len));
        xor_g(P, mo_to_be(*p.ej0));
        *p.tag_out = be_to_mo(P);
    }
    // plan the call as the host runtime does (the scratch grown to what the plan needs, then planned again) and execute every step
    const MsgPlan &go(const MsgCall &call) {
        for (;;) {
            const MsgScratch s = {parts.data(), fold_a.data(), fold_b.data(), slots, nullptr, {nullptr, nullptr}, 0, nullptr, &km.ptab[0][0]};
            msg_plan(last, call, rules, s, [] { return false; });
            if (last.parts_need * 64 <= parts.size()) break;
            parts.resize(last.parts_need * 64);
        }
        CHECK(last.rc == AESGCM_OK, "the plan refuses the call: %d", last.rc);
        for (u32 k = 0; k < last.n; k++) {
            const MsgStep &t = last.step[k];
            switch (t.kind) {
            case MsgStep::CLEAR: *t.clear = make_uint4(0, 0, 0, 0); break;
            case MsgStep::MAIN: emu_main(t.mode, &km, t.m); leave_ej0(t.m.ej0, t.m.iv0, t.m.iv1, t.m.iv2); if (t.m.tail) emu_main_tail(t.m); break;
            case MsgStep::BODY: CHECK(!t.b.cyc || t.b.cw == BODY_CYC_WAVES, "the half shape has no emulator"); emu_body(t.mode, &km, t.b); leave_ej0(t.b.ej0, t.b.iv0, t.b.iv1, t.b.iv2); break;
            case MsgStep::FOLD: emu_fold(t.f, t.wgs); break;
            case MsgStep::COMBINE: emu_combine(&km, t.c); break;
            }
        }
        return last;
    }
    // the calls of the tests: a whole message's tag; a range into a chaining value; a range's weighted polynomial value; keystream / ECB
    void crypt(int dec, const uint8_t iv[12], const uint8_t *aad, u64 aad_len, const uint8_t *in, u64 len, uint8_t *out, uint8_t tag[16]) {
        go(MsgCall{MSG_TAG, dec ? MODE_DEC : MODE_ENC, iv, aad, aad_len, in, len, out, 0, nullptr, 0, false});
        memcpy(tag, &slots[0], 16);
    }
    void carry(int mode, const uint8_t *iv, const void *aad, u64 aad_len, const void *in, u64 len, void *out, u64 first_block, uint4 *Y, bool main_only) {
        go(MsgCall{MSG_CARRY, mode, iv, aad, aad_len, in, len, out, first_block, Y, 0, main_only});
    }
    void poly(int mode, const uint8_t *iv, const void *aad, u64 aad_len, const void *in, u64 len, void *out, u64 first_block, u64 after, uint4 *W) {
        go(MsgCall{MSG_POLY, mode, iv, aad, aad_len, in, len, out, first_block, W, after, false});
    }
    void raw(int mode, const uint8_t *iv, const void *in, u64 len, void *out, u64 first_block) { go(MsgCall{MSG_RAW, mode, iv, nullptr, 0, in, len, out, first_block, nullptr, 0, true}); }
};

static std::vector<uint8_t> rnd(size_t n, u64 seed) {
    std::vector<uint8_t> v(n + 16);     // slack keeps .data() valid for n = 0
    orc_fill_splitmix64(v.data(), n, seed, 0);
    v.resize(n);
    return v;
}
// 16-byte aligned copy (the device data path requires aligned in/out)
struct ABuf { uint8_t *p; size_t n; ABuf(size_t n_) : n(n_) { p = (uint8_t *)aligned_alloc(16, (n + 31) / 16 * 16 + 16); memset(p, 0xA5, (n + 31) / 16 * 16 + 16); } ~ABuf() { free(p); } };

static void test_units() {
    for (u32 x = 0; x < 256; x++) CHECK(g_tb.sbox[x] == orc_sbox((uint8_t)x), "sbox[%u]", x);
    // k_fold level plan for every item count and both first-level periods: each level's output fits the buffer it is written to
    // (A, B, A, ...), the walk ends at <= COMBINE_MAX_ITEMS items, and the group is a power of two and a multiple of the period
    for (u32 period : {1u, 4u}) for (u32 n0 = COMBINE_MAX_ITEMS + 1; n0 <= AESGCM_MAX_CHUNKS; n0 += (n0 < 70000 ? 1 : 4099)) {
        u32 n = n0, per = period, which = 0, levels = 0;
        while (n > COMBINE_MAX_ITEMS || per > 1) {
            const u32 g = fold_group(n, per), G = fold_wgs(n, g);
            CHECK(g >= 1 && g <= FOLD_GROUP && (g & (g - 1)) == 0 && g % per == 0, "fold_group(%u, %u) = %u", n, per, g);
            CHECK(G <= (which ? FOLD_B_ITEMS : FOLD_A_ITEMS), "fold level %u of n0 = %u leaves %u items", levels, n0, G);
            CHECK(G < n || n == 1, "fold level does not shrink: %u -> %u", n, G);
            n = G; per = 1; which ^= 1; if (++levels > 4) break;
        }
        CHECK(levels <= 3, "n0 = %u needs %u k_fold levels", n0, levels);
    }
    // gf_mul vs oracle
    for (int i = 0; i < 200; i++) {
        auto a = rnd(16, 100 + i), b = rnd(16, 900 + i);
        if (i == 0) { memset(a.data(), 0, 16); a[0] = 0x80; }
        uint4 am, bm; memcpy(&am, a.data(), 16); memcpy(&bm, b.data(), 16);
        uint4 z = gf_mul_mo(am, bm);
        uint8_t zo[16]; orc_gfmul(b.data(), a.data(), zo);
        CHECK(memcmp(&z, zo, 16) == 0, "gf_mul %d", i);
    }
}

// bitsliced AES (tests/host_emul/aesgcm_bs.h: the round-2 experiment that measured 0.7 x; kept under test because its S-box circuit is tools/sbox_lut3.py's output): the LUT3-mapped S-box on all 256 inputs, the transpose, and whole blocks (32 per
// "lane") for the three key sizes against the oracle's literal cipher
static void test_bitslice() {
    {   // S-box: byte values 0..255 in 8 lanes-worth of 32 slots
        for (u32 base = 0; base < 256; base += 32) {
            u32 x[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            for (u32 i = 0; i < 32; i++) for (u32 b = 0; b < 8; b++) x[b] |= (((base + i) >> b) & 1u) << i;
            bs_sbox(x[0], x[1], x[2], x[3], x[4], x[5], x[6], x[7]);
            for (u32 i = 0; i < 32; i++) {
                u32 y = 0;
                for (u32 b = 0; b < 8; b++) y |= ((x[b] >> i) & 1u) << b;
                CHECK(y == orc_sbox((uint8_t)(base + i)), "bs_sbox %u", base + i);
            }
        }
    }
    {   // transpose
        u32 w[32], ref[32];
        auto r = rnd(128, 4242);
        memcpy(w, r.data(), 128); memcpy(ref, r.data(), 128);
        bs_transpose32(w);
        for (u32 p = 0; p < 32; p++) for (u32 i = 0; i < 32; i++) CHECK(((w[i] >> p) & 1u) == ((ref[p] >> i) & 1u), "transpose %u %u", p, i);
    }
    for (int kl : {16, 24, 32}) {
        auto key = rnd((size_t)kl, 5000 + kl);
        uint8_t rk[240]; int nr = 0;
        orc_key_expand(key.data(), (size_t)kl, rk, &nr);
        static u32 rkm[15 * 128];
        bs_key_masks(rk, nr, rkm);
        auto in = rnd(32 * 16, 6000 + kl);
        u32 st[128];
        for (int q = 0; q < 128; q++) st[q] = 0;
        for (u32 i = 0; i < 32; i++) for (u32 j = 0; j < 16; j++) for (u32 b = 0; b < 8; b++) st[8 * j + b] |= (u32)((in[16 * i + j] >> b) & 1u) << i;
        for (int q = 0; q < 128; q++) st[q] ^= rkm[q];                      // AddRoundKey 0
        bs_rounds(st, rkm, nr);
        for (u32 i = 0; i < 32; i++) {
            uint8_t want[16], got[16];
            orc_aes_encrypt_block(rk, nr, in.data() + 16 * i, want);
            for (u32 j = 0; j < 16; j++) { got[j] = 0; for (u32 b = 0; b < 8; b++) got[j] |= (uint8_t)(((st[8 * j + b] >> i) & 1u) << b); }
            CHECK(memcmp(want, got, 16) == 0, "bitsliced AES-%d block %u", 8 * kl, i);
        }
    }
}

// batch-path pieces: Shoup 4-bit multiply against the bit-serial multiply, in-kernel key schedule against the oracle
static void test_batch_pieces() {
    static unsigned char smem[BATCH_LDS_BYTES] __attribute__((aligned(16)));
    for (u32 tid = 0; tid < AESGCM_WG; tid++) main_fill_lds(smem, nullptr, &g_tb, tid, false, AESGCM_WG);
    for (u32 v = 0; v < 16; v++) *reinterpret_cast<u32 *>(smem + BATCH_LDS_RTAB_OFF + 4 * v) = shoup_rem_calc(v);
    for (int it = 0; it < 50; it++) {
        auto cb = rnd(16, 7000 + it), yb = rnd(16, 8000 + it);
        if (it == 1) memset(yb.data(), 0xFF, 16);
        if (it == 2) { memset(yb.data(), 0, 16); yb[15] = 1; }
        uint4 cm, ym; memcpy(&cm, cb.data(), 16); memcpy(&ym, yb.data(), 16);
        const G128 c = mo_to_be(cm), y = mo_to_be(ym);
        const u32 tab = 256 * (it % 8);
        for (u32 v = 0; v < 16; v++) { G128 e = shoup_entry(c, v); *reinterpret_cast<uint4 *>(smem + tab + 16 * v) = make_uint4(e.w[0], e.w[1], e.w[2], e.w[3]); }
        const G128 z = shoup_mul(y, smem, tab), want = gf_mul(y, c);
        CHECK(memcmp(&z, &want, 16) == 0, "shoup_mul %d", it);
        {   // byte-wise variant with the two tables Th, Tl (k_batch3)
            static unsigned char t2[512] __attribute__((aligned(16)));
            for (u32 v = 0; v < 16; v++) {
                const G128 e = shoup_entry(c, v), el = gf_mulx4(e);
                *reinterpret_cast<uint4 *>(t2 + 16 * v) = make_uint4(e.w[0], e.w[1], e.w[2], e.w[3]);
                *reinterpret_cast<uint4 *>(t2 + 256 + 16 * v) = make_uint4(el.w[0], el.w[1], el.w[2], el.w[3]);
            }
            const G128 z2 = shoup2_mul(y, t2, 0u);
            CHECK(memcmp(&z2, &want, 16) == 0, "shoup2_mul %d", it);
            const G128 z3 = shoup2_mul_dr(y, t2, 0u);                  // round 4: the same product with the reduction delayed
            CHECK(memcmp(&z3, &want, 16) == 0, "shoup2_mul_dr %d", it);
            u32 Vo[6], Vh[6];                                           // ... and split over an owner and a helper lane (k_batch3 at 8 lanes per packet)
            shoup2_half_dr(y.w[0], y.w[1], t2, 0u, Vo);
            shoup2_half_dr(y.w[2], y.w[3], t2, 0u, Vh);
            const G128 z4 = shoup2_pair_join(Vo, Vh);
            CHECK(memcmp(&z4, &want, 16) == 0, "shoup2_half_dr / pair_join %d", it);
        }
        const G128 s1 = gf_sqr(y), s2 = gf_mul(y, y), s3 = gf_sqr(c), s4 = gf_mul(c, c);
        CHECK(memcmp(&s1, &s2, 16) == 0 && memcmp(&s3, &s4, 16) == 0, "gf_sqr %d", it);
    }
    for (int klen : {16, 24, 32}) {
        auto key = rnd(klen, 9000 + klen);
        uint8_t rkb[240]; int nr; orc_key_expand(key.data(), klen, rkb, &nr);
        u32 rk[60];
        for (u32 lane : {0u, 17u, 63u}) {
            const u32 lb = (lane & 31u) << 2;
            if (klen == 16) batch_key_expand<10>(key.data(), rk, smem, lb);
            else if (klen == 24) batch_key_expand<12>(key.data(), rk, smem, lb);
            else batch_key_expand<14>(key.data(), rk, smem, lb);
            CHECK(memcmp(rk, rkb, 16 * (nr + 1)) == 0, "batch_key_expand %d lane %u", klen, lane);
        }
    }
}

// packets under one key, 2^LG lanes per packet (k_pktg): per-packet IV/AAD/length; lane accumulators, the H^2 step with the
// length block in lane G-2, the cross-lane tree with wave-uniform constants, E_K(J0) from the one-lane-per-packet pass
template <int NR, int DEC, int LG, bool SC = false>
static uint4 emu_pktg_packet(const KeyMaterial *km, const PktParams &p, const unsigned char *smem, u32 pkt, u32 extra_iters, u32 grp) {
    constexpr u32 G = 1u << LG;
    const PktInfo q = pkt_info<SC>(p, pkt);                       // SC: the body of k_pktgs (places from the arrays of addresses behind p.route)
    const u32 iters = pktg_iters(q, G) + extra_iters;             // a wave runs to the longest packet of its groups
    uint4 acc[G];
    for (u32 l = 0; l < G; l++) acc[l] = pktg_close_lane<LG>(pktg_lane<NR, DEC, LG>(km, p, q, smem, l, grp * G + l, iters, true), q, smem, l);
    for (int j = 0; j < LG; j++) {
        uint4 o[G];
        for (u32 l = 0; l < G; l++) o[l] = pktg_tree_offer(acc[l], smem, j);
        for (u32 l = 0; l < G; l++) if (l & (1u << j)) acc[l] = xor4(acc[l], o[l ^ (1u << j)]);
    }
    return xor4(acc[G - 1], pktg_ej0_lane<NR>(km, p, smem, pkt, (pkt * 5 + 3) % 64));
}
template <int LG, bool SC = false>
static uint4 emu_pktg(const KeyMaterial *km, int dec, const PktParams &p, const unsigned char *smem, u32 pkt, u32 extra, u32 grp) {
    if (km->nr == 10) return dec ? emu_pktg_packet<10, 1, LG, SC>(km, p, smem, pkt, extra, grp) : emu_pktg_packet<10, 0, LG, SC>(km, p, smem, pkt, extra, grp);
    if (km->nr == 12) return dec ? emu_pktg_packet<12, 1, LG, SC>(km, p, smem, pkt, extra, grp) : emu_pktg_packet<12, 0, LG, SC>(km, p, smem, pkt, extra, grp);
    return dec ? emu_pktg_packet<14, 1, LG, SC>(km, p, smem, pkt, extra, grp) : emu_pktg_packet<14, 0, LG, SC>(km, p, smem, pkt, extra, grp);
}
static void test_packets(int key_len, u64 seed) {
    auto key = rnd(key_len, seed);
    Emu E(key.data(), key_len, 0);
    const u32 lens[] = {0, 1, 15, 16, 17, 48, 1000, 1008, 1024, 4096, 4100, 70000, 0, 256, 240};
    const u32 aads[] = {0, 20, 28, 16, 0, 33, 68, 0, 5, 0, 12, 64, 16, 0, 16};
    const int n = 15;
    std::vector<u64> doff(n + 1, 0), aoff(n + 1, 0);
    for (int i = 0; i < n; i++) { doff[i + 1] = doff[i] + lens[i]; aoff[i + 1] = aoff[i] + aads[i]; }
    ABuf in(doff[n]), out(doff[n]);
    auto aad = rnd(aoff[n], seed + 1), ivs = rnd(12 * n, seed + 2);
    orc_fill_splitmix64(in.p, doff[n], seed + 3, 0);
    std::vector<uint8_t> tags(16 * n);
    PktParams p; memset(&p, 0, sizeof p);
    p.ivs = ivs.data(); p.aad = aad.data(); p.in = in.p; p.out = out.p; p.tags = tags.data();
    p.data_off = doff.data(); p.aad_off = aoff.data(); p.n_pkts = n; p.aligned = 1;
    static unsigned char smem[PKTG_LDS_BYTES(6)] __attribute__((aligned(16)));
    for (int lg : {2, 3, 4, 6}) {
        memset(smem, 0xEE, sizeof smem);
        for (u32 tid = 0; tid < AESGCM_PKT_WG; tid++) pktg_fill_lds(smem, &E.km, &g_tb, tid, AESGCM_PKT_WG, lg);
        for (int dec = 0; dec < 2; dec++) {
            p.in = dec ? out.p : in.p; p.out = out.p;           // decrypt in place
            for (u32 pkt = 0; pkt < (u32)n; pkt++) {
                const u32 extra = (pkt % 3 == 1) ? 2 : 0, grp = pkt & ((64u >> lg) - 1u);
                const uint4 t = lg == 2 ? emu_pktg<2>(&E.km, dec, p, smem, pkt, extra, grp) : lg == 3 ? emu_pktg<3>(&E.km, dec, p, smem, pkt, extra, grp)
                              : lg == 4 ? emu_pktg<4>(&E.km, dec, p, smem, pkt, extra, grp) : emu_pktg<6>(&E.km, dec, p, smem, pkt, extra, grp);
                std::vector<uint8_t> ref(lens[pkt] + 16); uint8_t rtag[16];
                if (!dec) {
                    orc_gcm_crypt(0, key.data(), key_len, ivs.data() + 12 * pkt, aad.data() + aoff[pkt], aads[pkt], in.p + doff[pkt], lens[pkt], ref.data(), rtag);
                    CHECK(memcmp(ref.data(), out.p + doff[pkt], lens[pkt]) == 0, "pktg ct %u lg %d", pkt, lg);
                    memcpy(tags.data() + 16 * pkt, &t, 16);
                } else {
                    CHECK(memcmp(in.p + doff[pkt], out.p + doff[pkt], lens[pkt]) == 0, "pktg dec %u lg %d", pkt, lg);
                    memcpy(rtag, tags.data() + 16 * pkt, 16);
                }
                CHECK(memcmp(&t, rtag, 16) == 0, "pktg tag %u len %u aad %u dec %d lg %d", pkt, lens[pkt], aads[pkt], dec, lg);
            }
        }
    }
    // the same packets, one lane per packet (k_pktl): tags must equal the ones above, decrypt restores the input
    static unsigned char smem_h[AESGCM_LDS_BYTES] __attribute__((aligned(16)));
    for (u32 tid = 0; tid < AESGCM_MAIN_WG; tid++) main_fill_lds(smem_h, &E.km, &g_tb, tid, true, AESGCM_MAIN_WG, GH_TAB_H);
    ABuf out2(doff[n]);
    std::vector<uint8_t> tags2(16 * n + 16), tags3(16 * n + 16);
    std::vector<int> auth(n, -1);
    for (int dec = 0; dec < 2; dec++) {
        p.in = dec ? out2.p : in.p; p.out = out2.p;
        p.tags = dec ? tags3.data() + 1 : tags2.data();        // an unaligned tag array takes the bytewise store
        p.expect = dec ? tags2.data() : nullptr; p.auth = dec ? auth.data() : nullptr;
        for (u32 pkt = 0; pkt < (u32)n; pkt++) {
            const u32 lane = (pkt * 7) % 64;
            if (E.km.nr == 10) { if (dec) pktl_lane<10, 1>(&E.km, p, smem_h, pkt, lane); else pktl_lane<10, 0>(&E.km, p, smem_h, pkt, lane); }
            else if (E.km.nr == 12) { if (dec) pktl_lane<12, 1>(&E.km, p, smem_h, pkt, lane); else pktl_lane<12, 0>(&E.km, p, smem_h, pkt, lane); }
            else { if (dec) pktl_lane<14, 1>(&E.km, p, smem_h, pkt, lane); else pktl_lane<14, 0>(&E.km, p, smem_h, pkt, lane); }
        }
        if (!dec) {
            CHECK(memcmp(tags2.data(), tags.data(), 16 * n) == 0, "pktl tags");
            std::vector<uint8_t> ref(doff[n] + 16); uint8_t rtag[16];
            for (int k = 0; k < n; k++) {
                orc_gcm_crypt(0, key.data(), key_len, ivs.data() + 12 * k, aad.data() + aoff[k], aads[k], in.p + doff[k], lens[k], ref.data(), rtag);
                CHECK(memcmp(ref.data(), out2.p + doff[k], lens[k]) == 0, "pktl ct %d", k);
            }
        } else {
            CHECK(memcmp(tags3.data() + 1, tags.data(), 16 * n) == 0, "pktl dec tags");
            CHECK(memcmp(out2.p, in.p, doff[n]) == 0, "pktl dec data");
            for (int k = 0; k < n; k++) CHECK(auth[k] == 1, "pktl auth %d", k);
        }
    }
}

static void test_key(int key_len, u32 G /* rows per chunk override, 0 = production rule */, u64 seed, const std::vector<std::pair<u64, u64>> &sizes) {
    auto key = rnd(key_len, seed);
    Emu E(key.data(), key_len, G);
    uint8_t rk[240]; int nr;
    orc_key_expand(key.data(), key_len, rk, &nr);
    CHECK((int)E.km.nr == nr && memcmp(E.km.rk_bytes, rk, 16 * (nr + 1)) == 0, "key schedule len %d", key_len);
    uint8_t zero[16] = {0}, h[16];
    orc_aes_encrypt_block(rk, nr, zero, h);
    CHECK(memcmp(&E.km.h, h, 16) == 0, "H");
    // power tables spot checks: pw[0][k] = H^k via oracle repeated multiply
    {
        uint8_t acc[16] = {0x80};
        for (int k = 0; k <= AESGCM_WG; k++) {
            if (k == 0 || k == 1 || k == 2 || k == 3 || k == 255 || k == 256 || k == 257 || k == 511 || k == 512 || k == AESGCM_WG - 1 || k == AESGCM_WG)
                CHECK(memcmp(&E.km.pw[0][k], acc, 16) == 0, "pw[0][%d]", k);
            orc_gfmul(h, acc, acc);
        }
        CHECK(memcmp(&E.km.pw[1][1], &E.km.pw[0][AESGCM_WG], 16) == 0, "beta");
        uint4 b2 = gf_mul_mo(E.km.pw[1][1], E.km.pw[1][1]);
        CHECK(memcmp(&E.km.pw[1][2], &b2, 16) == 0, "beta^2");
        uint4 g3 = gf_mul_mo(gf_mul_mo(E.km.pw[2][1], E.km.pw[2][1]), E.km.pw[2][1]);
        CHECK(memcmp(&E.km.pw[2][3], &g3, 16) == 0, "gamma^3");
        CHECK(memcmp(&E.km.pw[3][1], &E.km.pw[2][AESGCM_WG], 16) == 0, "delta");
    }
    // the five-bit GHASH tables of the three fixed Horner constants: Y * c through ghash_mul_const_lds against the bit-serial
    // product, on every single-bit value (each of the 26 groups, the three that straddle a dword included) and random ones
    for (int which = 0; which < 3; which++) {
        static unsigned char smem[AESGCM_LDS_BYTES] __attribute__((aligned(16)));
        for (u32 tid = 0; tid < AESGCM_MAIN_WG; tid++) main_fill_lds(smem, &E.km, &g_tb, tid, true, AESGCM_MAIN_WG, which);
        const uint4 c = which == GH_TAB_K64 ? E.km.pw[0][64] : which == GH_TAB_H ? E.km.h : E.km.pw[0][256];
        for (int i = 0; i < 128 + 64; i++) {
            uint4 y;
            if (i < 128) { u32 w[4] = {0, 0, 0, 0}; w[i >> 5] = 1u << (i & 31); y = make_uint4(w[0], w[1], w[2], w[3]); }
            else { auto r = rnd(16, seed * 131 + i); memcpy(&y, r.data(), 16); }
            const uint4 a = ghash_mul_const_lds(y, smem), b = gf_mul_mo(y, c);
            CHECK(memcmp(&a, &b, 16) == 0, "ghash_mul_const_lds table %d case %d", which, i);
        }
    }
    // ECB through the LDS round code
    {
        const size_t nb = 700;
        ABuf in(16 * nb), out(16 * nb);
        orc_fill_splitmix64(in.p, 16 * nb, seed + 5, 0);
        E.raw(MODE_ECB, nullptr, in.p, 16 * nb, out.p, 0);
        for (size_t i = 0; i < nb; i++) { uint8_t o[16]; orc_aes_encrypt_block(rk, nr, in.p + 16 * i, o); CHECK(memcmp(o, out.p + 16 * i, 16) == 0, "ecb block %zu", i); }
    }
    for (auto &sz : sizes) {
        const u64 al = sz.first, n = sz.second;
        auto iv = rnd(12, seed + 11 + n), aad = rnd(al, seed + 12 + al);
        ABuf pt(n), ct(n), ref(n), back(n);
        orc_fill_splitmix64(pt.p, n, seed + 13, 0);
        uint8_t tag[16], rtag[16], dtag[16];
        // misalign the AAD on purpose for odd sizes
        std::vector<uint8_t> aad_buf(al + 32);
        uint8_t *aadp = aad_buf.data() + ((al & 1) ? 3 : 0);
        if (al) memcpy(aadp, aad.data(), al);
        E.crypt(0, iv.data(), aadp, al, pt.p, n, ct.p, tag);
        orc_gcm_crypt(0, key.data(), key_len, iv.data(), aad.data(), al, pt.p, n, ref.p, rtag);
        CHECK(memcmp(ct.p, ref.p, n) == 0, "ct  key %d G %u aad %llu len %llu", key_len, G, (unsigned long long)al, (unsigned long long)n);
        CHECK(memcmp(tag, rtag, 16) == 0, "tag key %d G %u aad %llu len %llu", key_len, G, (unsigned long long)al, (unsigned long long)n);
        CHECK(ct.p[n] == 0xA5, "overrun past ragged tail");
        E.crypt(1, iv.data(), aadp, al, ct.p, n, back.p, dtag);
        CHECK(memcmp(back.p, pt.p, n) == 0 && memcmp(dtag, rtag, 16) == 0, "dec key %d G %u aad %llu len %llu", key_len, G, (unsigned long long)al, (unsigned long long)n);
    }
}

// shards: split one message over R ranks (each with its own emulated context), gather, finalize
static void test_shards(int key_len, u32 G, u64 al, u64 n, int R, u64 seed) {
    auto key = rnd(key_len, seed), iv = rnd(12, seed + 1), aad = rnd(al, seed + 2);
    ABuf pt(n), ct(n), ref(n);
    orc_fill_splitmix64(pt.p, n, seed + 3, 0);
    uint8_t rtag[16];
    orc_gcm_crypt(0, key.data(), key_len, iv.data(), aad.data(), al, pt.p, n, ref.p, rtag);
    Emu E(key.data(), key_len, G);
    const u64 total_blocks = (n + 15) / 16;
    std::vector<uint4> gathered(R);
    u64 first = 0;
    for (int r = 0; r < R; r++) {
        u64 blocks = total_blocks / R + ((u64)r < total_blocks % R ? 1 : 0);
        u64 end = first + blocks;
        u64 len = (end == total_blocks ? n : 16 * end) - 16 * first;
        E.poly(MODE_ENC, iv.data(), r == 0 ? aad.data() : nullptr, r == 0 ? al : 0, pt.p + 16 * first, len, ct.p + 16 * first, first, total_blocks - end, &gathered[r]);
        first = end;
    }
    uint4 t;
    emu_combine(&E.km, plan_combine_tag(gathered.data(), R, PARTS_GATHERED, iv.data(), al, n, &t));
    CHECK(memcmp(ct.p, ref.p, n) == 0, "shard ct R %d", R);
    CHECK(memcmp(&t, rtag, 16) == 0, "shard tag key %d G %u aad %llu len %llu R %d", key_len, G, (unsigned long long)al, (unsigned long long)n, R);
}

// head / k_body / tail split (absorb_range): whole messages and shards with arbitrary first blocks
static void test_body(int key_len, u32 G, u64 al, u64 n, u64 seed, bool cyc = false) {
    auto key = rnd(key_len, seed), iv = rnd(12, seed + 1), aad = rnd(al, seed + 2);
    ABuf pt(n), ct(n), ref(n), back(n);
    orc_fill_splitmix64(pt.p, n, seed + 3, 0);
    uint8_t rtag[16], tag[16], dtag[16];
    orc_gcm_crypt(0, key.data(), key_len, iv.data(), aad.data(), al, pt.p, n, ref.p, rtag);
    Emu E(key.data(), key_len, G);
    E.rules.cyc_capable = cyc; E.rules.body_min = 4096;
    if (cyc) {                                                          // first with k_fold / k_combine behind the launch, then (below) with the fused closing
        uint8_t utag[16];
        E.rules.cyc_fuse = false;
        E.crypt(0, iv.data(), aad.data(), al, pt.p, n, ct.p, utag);
        CHECK(memcmp(utag, rtag, 16) == 0, "cyclic unfused tag key %d aad %llu len %llu", key_len, (unsigned long long)al, (unsigned long long)n);
        E.rules.cyc_fuse = true;
        memset(ct.p, 0xA5, n);
    }
    E.crypt(0, iv.data(), aad.data(), al, pt.p, n, ct.p, tag);
    CHECK(E.n_body() == 1, "body split did not apply: len %llu G %u", (unsigned long long)n, G);
    CHECK(!cyc || E.n_cyc() == 1, "cyclic rows did not take the message: len %llu", (unsigned long long)n);
    CHECK(cyc || al || (n % 4096) || n < 16 * 256 * 40 || E.n_fold_close() == 1, "k_fold did not close the message: len %llu", (unsigned long long)n);
    CHECK(memcmp(ct.p, ref.p, n) == 0, "body ct key %d G %u aad %llu len %llu", key_len, G, (unsigned long long)al, (unsigned long long)n);
    CHECK(memcmp(tag, rtag, 16) == 0, "body tag key %d G %u aad %llu len %llu", key_len, G, (unsigned long long)al, (unsigned long long)n);
    CHECK(ct.p[n] == 0xA5, "body overrun");
    E.crypt(1, iv.data(), aad.data(), al, ct.p, n, back.p, dtag);
    CHECK(memcmp(back.p, pt.p, n) == 0 && memcmp(dtag, rtag, 16) == 0, "body dec key %d G %u", key_len, G);
    // the same message as R shards, every shard into a chaining value (MSG_CARRY) from its own first block
    for (int R : {2, 3}) {
        ABuf ct2(n);
        const u64 total_blocks = (n + 15) / 16;
        std::vector<uint4> gathered(R);
        u64 first = 0; int nsplit = 0;
        for (int r = 0; r < R; r++) {
            u64 blocks = total_blocks / R + ((u64)r < total_blocks % R ? 1 : 0), end = first + blocks;
            u64 len = (end == total_blocks ? n : 16 * end) - 16 * first;
            uint4 Y = make_uint4(0, 0, 0, 0);
            E.carry(MODE_ENC, iv.data(), r == 0 ? aad.data() : nullptr, r == 0 ? al : 0, pt.p + 16 * first, len, ct2.p + 16 * first, first, &Y, false);
            nsplit += E.n_body();
            CombineParams q = plan_combine_poly(nullptr, 0, PARTS_NONE, 0, &gathered[r]);
            q.carry = &Y; q.has_carry = 1; q.e_carry = total_blocks - end;
            emu_combine(&E.km, q);
            first = end;
        }
        uint4 t;
        emu_combine(&E.km, plan_combine_tag(gathered.data(), R, PARTS_GATHERED, iv.data(), al, n, &t));
        CHECK(nsplit > 0, "no shard took the split");
        CHECK(memcmp(ct2.p, ref.p, n) == 0 && memcmp(&t, rtag, 16) == 0, "body shards R %d key %d G %u", R, key_len, G);
    }
}

// streaming: AAD in chunks, data in chunks, running state carried through combine
static void test_stream(int key_len, u32 G, u64 al, u64 n, u64 chunk, u64 seed) {
    auto key = rnd(key_len, seed), iv = rnd(12, seed + 1), aad = rnd(al, seed + 2);
    ABuf pt(n), ct(n), ref(n);
    orc_fill_splitmix64(pt.p, n, seed + 3, 0);
    uint8_t rtag[16];
    orc_gcm_crypt(0, key.data(), key_len, iv.data(), aad.data(), al, pt.p, n, ref.p, rtag);
    Emu E(key.data(), key_len, G);
    uint4 Y = make_uint4(0, 0, 0, 0);
    for (u64 off = 0; off < al; off += chunk) {
        u64 m = al - off < chunk ? al - off : chunk;
        E.carry(MODE_ENC, iv.data(), aad.data() + off, m, nullptr, 0, nullptr, 0, &Y, true);
    }
    for (u64 off = 0; off < n; off += chunk) {
        u64 m = n - off < chunk ? n - off : chunk;
        E.carry(MODE_ENC, iv.data(), nullptr, 0, pt.p + off, m, ct.p + off, off / 16, &Y, true);
    }
    uint4 t;
    emu_combine(&E.km, plan_combine_final(&Y, iv.data(), al, n, &t));
    CHECK(memcmp(ct.p, ref.p, n) == 0, "stream ct");
    CHECK(memcmp(&t, rtag, 16) == 0, "stream tag key %d aad %llu len %llu chunk %llu", key_len, (unsigned long long)al, (unsigned long long)n, (unsigned long long)chunk);
}

static void test_keystream_and_ghash(u64 seed) {
    auto key = rnd(32, seed), iv = rnd(12, seed + 1);
    Emu E(key.data(), 32, 2);
    uint8_t rk[240]; int nr; orc_key_expand(key.data(), 32, rk, &nr);
    const u64 first = 0x01FFFF00ull - 2, nb = 600;      // counter crosses a 2^8, 2^16, 2^24 carry boundary
    ABuf out(16 * nb);
    E.raw(MODE_KS, iv.data(), out.p, 16 * nb, out.p, first);
    for (u64 i = 0; i < nb; i++) {
        uint8_t cb[16], o[16]; memcpy(cb, iv.data(), 12);
        u32 c = (u32)(2 + first + i); cb[12] = c >> 24; cb[13] = c >> 16; cb[14] = c >> 8; cb[15] = c;
        orc_aes_encrypt_block(rk, nr, cb, o);
        CHECK(memcmp(o, out.p + 16 * i, 16) == 0, "keystream block %llu", (unsigned long long)i);
    }
    // GHASH chaining value Y = P*H
    for (u64 n : {1ull, 16ull, 17ull, 8191ull, 20000ull}) {
        auto d = rnd(n, seed + n);
        uint4 y; E.poly(MODE_ENC, iv.data(), d.data(), n, nullptr, 0, nullptr, 0, 1, &y);
        uint8_t yo[16] = {0}; orc_ghash_update((const uint8_t *)&E.km.h, yo, d.data(), n);
        CHECK(memcmp(&y, yo, 16) == 0, "ghash len %llu", (unsigned long long)n);
    }
}

// Many messages under one key by rows (k_rows / k_rows_close, csrc/aesgcm_rows.h): the cut (fixed-size records: arithmetic; offset arrays: the planner's two
// prefix sums), every block in a scrambled order with the same piece walk and lane code as k_rows, the record slots of the closing in a scrambled order with plain
// XORs for the atomics; ciphertext and tags against the oracle, and the zero-at-rest rule of the shared scratch.
// g_route_min != 0 (offset arrays / scattered only): the call is ROUTED per message as k_len_scan + k_rows_plan do on the device (round 6) -- messages whose data + AAD
// lie below the mark are the packet kernels' (here: pktl_lane, a lane each), the row launches must see them as nothing: no unit, no smalls block, no slot, no arrival
static u32 g_route_min = 0;
template <int NR>
static void emu_rows_nr(const KeyMaterial *km, int dec, RowsParams &p, u32 waves, u32 force_d) {
    static unsigned char smem[AESGCM_LDS_BYTES_T4] __attribute__((aligned(16)));
    for (u32 tid = 0; tid < AESGCM_MAIN_WG; tid++) main_fill_lds(smem, km, &g_tb, tid, true, AESGCM_MAIN_WG, GH_TAB_K64);
    for (u32 tid = 0; tid < AESGCM_MAIN_WG; tid++) fill_lds_t4(smem, &g_tb, tid, AESGCM_MAIN_WG);
    const u32 n = p.n_pkts;
    p.waves = waves;
    std::vector<u64> prefix(n + 1, 0), sprefix(n + 1, 0);
    std::vector<u32> slot_base(n + 1, 0);
    RowsHdr hdr;
    memset(&hdr, 0, sizeof hdr);
    size_t slots;
    const bool var = p.data_off || p.aad_off || p.len_arr;
    const u32 route_min = var ? g_route_min : 0u;
    u32 n_small = 0;
    auto geom_m = [&](u32 m) { return rows_geom_of(rows_msg(p, m), route_min); };
    auto na_m = [&](u32 m) { return rows_na_of(rows_msg(p, m), route_min); };
    auto small_m = [&](u32 m) { const RowsMsg q = rows_msg(p, m); return rows_is_small(q.len, q.alen, route_min); };
    if (var) {                                                           // k_rows_plan
        hdr.route_min = route_min;
        p.hdr = &hdr;
        CHECK(rows_route_min(p) == route_min, "rows: route_min");
        for (u32 m = 0; m < n; m++) {
            if (small_m(m)) { ++n_small; CHECK(rows_units(geom_m(m), na_m(m)) == 0 && rows_smalls(geom_m(m), na_m(m)) == 0 && rows_slots(geom_m(m), na_m(m), prefix[m], 7) == 0, "rows: a routed message counts"); }
            prefix[m + 1] = prefix[m] + rows_units(geom_m(m), na_m(m));
            sprefix[m + 1] = sprefix[m] + rows_smalls(geom_m(m), na_m(m));
        }
        hdr.G = prefix[n]; hdr.n_small = n_small;
        rows_cut(hdr.G, waves, force_d, ROWS_NB_CAP, &hdr.D, &hdr.NB, &hdr.dyn);
        for (u32 m = 0; m < n; m++) slot_base[m + 1] = slot_base[m] + rows_slots(geom_m(m), na_m(m), prefix[m], hdr.D);
        slots = ROWS_SLOTS_PER_MSG * (size_t)n + ROWS_NB_CAP;
        CHECK(slot_base[n] <= slots, "rows: %u slots planned, %zu held", slot_base[n], slots);
        p.prefix = prefix.data(); p.sprefix = sprefix.data(); p.slot_base = slot_base.data();
    } else {
        const RowsGeom g = rows_geom(p.pkt_len);
        const u32 na = rows_na(p.aad_len);
        p.U = rows_units(g, na); p.S = rows_smalls(g, na); p.G = (u64)n * p.U;
        rows_cut(p.G, waves, force_d, (u64)1 << 30, &p.D, &p.NB, &p.dyn);
        p.SM = p.U ? rows_nat_count(g, na) + (p.U - 1u) / p.D + 1u : 0u;
        slots = (size_t)n * p.SM;
    }
    p.slot_cap = (u32)slots;
    std::vector<RowsRec> rec(slots + 1);
    memset(rec.data(), 0, rec.size() * sizeof(RowsRec));
    std::vector<unsigned long long> acc(2 * (size_t)n + 2, 0);
    std::vector<u32> cnt(n + 1, 0), made_of(n + 1, 0);
    p.rec = rec.data(); p.acc = acc.data(); p.cnt = cnt.data();
    const u64 G = p.hdr ? p.hdr->G : p.G;
    const u32 D = p.hdr ? p.hdr->D : p.D, NB = p.hdr ? p.hdr->NB : p.NB, dyn = p.hdr ? p.hdr->dyn : p.dyn;
    CHECK(dyn || NB <= waves, "rows: %u blocks for %u waves", NB, waves);
    auto put = [&](u32 slot, const G128 &z, u64 e, u32 m, u32 flags) {
        CHECK(slot < slots && !rec[slot].flags, "rows: slot %u of %zu taken twice (message %u)", slot, slots, m);
        RowsRec r; r.w = z; r.e = e; r.msg = m; r.flags = flags;
        rec[slot] = r;
        ++made_of[m];
    };
    for (u32 kb = 0; kb < NB; kb++) {
        const u32 b = NB - 1 - kb;                                       // last block first
        u64 g = (u64)b * D;
        const u64 g_end = g + D < G ? g + D : G;
        u32 m = rows_find_msg(p, g);
        while (g < g_end) {
            const RowsMsg mq = rows_msg(p, m);
            const RowsGeom geo = geom_m(m);
            const u64 g0 = rows_unit_base(p, m);
            const u32 U = rows_units(geo, na_m(m)), sbase = rows_slot_base(p, m);
            if (U == 0) { ++m; continue; }                                 // a message shorter than a row has no unit: the closing alone sees it
            CHECK(g >= g0 && g < g0 + U, "rows: unit %llu outside message %u", (unsigned long long)g, m);
            while (g < g_end && g < g0 + U) {
                const RowsPiece pc = rows_piece(geo, sbase, g0, (u32)(g - g0), g_end - g, D);
                G128 z = {{0, 0, 0, 0}};
                for (u32 lane = 0; lane < 64; lane++) {
                    const CtrConsts cc = ctr_round1_consts(load_le32(p.ivs + 12 * m), load_le32(p.ivs + 12 * m + 4), load_le32(p.ivs + 12 * m + 8), km->rk, smem, (lane & 31u) << 2);
                    if (pc.kind == ROWS_RUN) {
                        const uint4 a = dec ? rows_run_lane<NR, MODE_DEC>(km, &g_tb, p, mq, pc, smem, cc, lane, 0, 0) : rows_run_lane<NR, MODE_ENC>(km, &g_tb, p, mq, pc, smem, cc, lane, 0, 0);
                        xor_g(z, rows_run_term(km, a, lane));
                    } else if (pc.kind == ROWS_TAIL) {
                        xor_g(z, dec ? rows_tail_lane<NR, 1>(km, p, mq, smem, cc, lane) : rows_tail_lane<NR, 0>(km, p, mq, smem, cc, lane));
                    } else {
                        xor_g(z, rows_aad_lane(km, p, mq, smem, lane));
                    }
                }
                put(pc.slot, z, pc.e, m, pc.kind == ROWS_TAIL ? ROWS_REC_VALID : (ROWS_REC_VALID | ROWS_REC_WEIGH));
                g += pc.len;
            }
            ++m;
        }
    }
    // k_rows_close: the lanes last first; lane i is message i (its length block and E_K(J0)), slot i, and the blocks i, i + lanes, ... of the smalls axis
    u32 finals = 0;
    auto due = [&](u32 m) { const RowsMsg mq = rows_msg(p, m); return rows_pieces(geom_m(m), na_m(m), rows_unit_base(p, m), D); };
    auto arrive = [&](u32 m, const G128 &z) {
        acc[2 * m] ^= ((unsigned long long)z.w[0] << 32) | z.w[1]; acc[2 * m + 1] ^= ((unsigned long long)z.w[2] << 32) | z.w[3];
        if (++cnt[m] == due(m)) {
            G128 t; t.w[0] = (u32)(acc[2 * m] >> 32); t.w[1] = (u32)acc[2 * m]; t.w[2] = (u32)(acc[2 * m + 1] >> 32); t.w[3] = (u32)acc[2 * m + 1];
            acc[2 * m] = acc[2 * m + 1] = 0; cnt[m] = 0;
            store_block_bytes(p.tags + (size_t)m * 16, be_to_mo(t), 16);
            ++finals;
        }
    };
    // the messages of the packet kernels: a lane each (k_pktl), reading the same arrays
    if (n_small) {
        static unsigned char smem_h[AESGCM_LDS_BYTES] __attribute__((aligned(16)));
        for (u32 tid = 0; tid < AESGCM_MAIN_WG; tid++) main_fill_lds(smem_h, km, &g_tb, tid, true, AESGCM_MAIN_WG, GH_TAB_H);
        PktParams k; memset(&k, 0, sizeof k);
        k.ivs = p.ivs; k.aad = p.aad; k.in = p.in; k.out = p.out; k.tags = p.tags; k.data_off = p.data_off; k.aad_off = p.aad_off; k.n_pkts = n; k.aad_len = p.aad_len; k.aligned = 1;
        hdr.sc_in = (u64)(uintptr_t)p.in_ptr; hdr.sc_out = (u64)(uintptr_t)p.out_ptr; hdr.sc_aad = (u64)(uintptr_t)p.aad_ptr; hdr.sc_len = (u64)(uintptr_t)p.len_arr; hdr.sc_alen = (u64)(uintptr_t)p.alen_arr;
        k.route = &hdr; k.scattered = p.len_arr ? 1u : 0u;
        for (u32 m = 0; m < n; m++) {
            if (!small_m(m)) continue;
            if (k.scattered) { if (dec) pktl_lane<NR, 1, false, false, true>(km, k, smem_h, m, (m * 5u) % 64u); else pktl_lane<NR, 0, false, false, true>(km, k, smem_h, m, (m * 5u) % 64u); }
            else if (dec) pktl_lane<NR, 1>(km, k, smem_h, m, (m * 5u) % 64u); else pktl_lane<NR, 0>(km, k, smem_h, m, (m * 5u) % 64u);
        }
    }
    const size_t lanes = slots > n ? slots : n;
    for (size_t k = 0; k < lanes; k++) {
        const size_t i = lanes - 1 - k;
        if (i < n && !small_m((u32)i)) arrive((u32)i, rows_msg_term(km, g_tb.te0, p, (u32)i));
        for (u64 t = i; t < rows_small_total(p); t += lanes) {
            G128 z;
            u64 e_run = 0;
            const u32 m = dec ? rows_small_block<1>(km, g_tb.te0, p, t, &z, &e_run) : rows_small_block<0>(km, g_tb.te0, p, t, &z, &e_run);
            ++made_of[m];
            arrive(m, rows_small_due(km, z, e_run));                       // (the kernel XORs the blocks of a segment first and pays once: the multiply is linear)
        }
        if (i >= slots) continue;
        const RowsRec r = rec[i];
        if (!(r.flags & ROWS_REC_VALID)) continue;
        rec[i].flags = 0;
        arrive(r.msg, rows_weigh(km, r));
    }
    CHECK(finals == n - n_small, "rows: %u of %u messages closed", finals, n - n_small);
    for (u32 m = 0; m < n; m++) {
        CHECK(!acc[2 * m] && !acc[2 * m + 1] && !cnt[m], "rows: message %u not zero at rest", m);
        if (small_m(m)) CHECK(made_of[m] == 0, "rows: message %u is the packet kernels' and fell into %u pieces here", m, made_of[m]);
        else CHECK(made_of[m] + 1u == due(m), "rows: message %u fell into %u pieces", m, made_of[m]);
    }
}
// var: 0 fixed-size records, 1 offset arrays, 2 messages wherever they live (arrays of addresses and lengths: every message with a gap of its own in front, in and
// out at different spacings)
static void test_rows(int key_len, u64 seed, u32 waves, u32 force_d, int var, const std::vector<u32> &lens, const std::vector<u32> &aads, u32 misalign = 0) {
    auto key = rnd(key_len, seed);
    Emu E(key.data(), key_len, 0);
    const u32 n = (u32)lens.size();
    const u64 gi = var == 2 ? 48 : 0, go = var == 2 ? 80 : 0;                // gaps between the messages of the scattered form (input, output)
    std::vector<u64> doff(n + 1, misalign), aoff(n + 1, 0);
    for (u32 i = 0; i < n; i++) { doff[i + 1] = doff[i] + lens[i]; aoff[i + 1] = aoff[i] + aads[i]; }
    ABuf in(doff[n] + gi * n), out(doff[n] + go * n), back(doff[n] + gi * n);
    auto aad = rnd(aoff[n], seed + 1), ivs = rnd(12 * n, seed + 2);
    orc_fill_splitmix64(in.p, doff[n] + gi * n, seed + 3, 0);
    std::vector<uint8_t> tags(16 * n + 16), tags2(16 * n + 16);
    std::vector<u64> in_ptr(n), out_ptr(n), aad_ptr(n);
    std::vector<u32> alens(aads);
    for (int dec = 0; dec < 2; dec++) {
        RowsParams p; memset(&p, 0, sizeof p);
        p.ivs = ivs.data(); p.tags = dec ? tags2.data() : tags.data();
        p.n_pkts = n;
        if (var == 2) {                                                  // encrypt in -> out, decrypt out -> back
            for (u32 k = 0; k < n; k++) {
                in_ptr[k] = (u64)(uintptr_t)((dec ? out.p : in.p) + doff[k] + (dec ? go : gi) * k);
                out_ptr[k] = (u64)(uintptr_t)((dec ? back.p : out.p) + doff[k] + (dec ? gi : go) * k);
                aad_ptr[k] = (u64)(uintptr_t)(aad.data() + aoff[k]);
            }
            p.in_ptr = in_ptr.data(); p.out_ptr = out_ptr.data(); p.len_arr = lens.data();
            if (aoff[n]) { p.aad_ptr = aad_ptr.data(); p.alen_arr = alens.data(); }
        } else {
            p.aad = aad.data(); p.in = dec ? out.p : in.p; p.out = out.p;
            if (var) { p.data_off = doff.data(); if (aoff[n]) p.aad_off = aoff.data(); }        // (no AAD anywhere: no AAD array -- empty messages then have no unit at all)
            else { p.pkt_len = lens[0]; p.aad_len = aads[0]; }
        }
        if (E.km.nr == 10) emu_rows_nr<10>(&E.km, dec, p, waves, force_d); else if (E.km.nr == 12) emu_rows_nr<12>(&E.km, dec, p, waves, force_d); else emu_rows_nr<14>(&E.km, dec, p, waves, force_d);
        if (!dec) {
            for (u32 k = 0; k < n; k++) {
                std::vector<uint8_t> ref(lens[k] + 16); uint8_t rtag[16];
                orc_gcm_crypt(0, key.data(), key_len, ivs.data() + 12 * k, aad.data() + aoff[k], aads[k], in.p + doff[k] + gi * k, lens[k], ref.data(), rtag);
                CHECK(memcmp(ref.data(), out.p + doff[k] + go * k, lens[k]) == 0, "rows ct %u len %u waves %u D %u var %d", k, lens[k], waves, force_d, var);
                CHECK(memcmp(rtag, tags.data() + 16 * k, 16) == 0, "rows tag %u len %u aad %u waves %u D %u var %d", k, lens[k], aads[k], waves, force_d, var);
            }
        } else {
            if (var == 2) { for (u32 k = 0; k < n; k++) CHECK(memcmp(back.p + doff[k] + gi * k, in.p + doff[k] + gi * k, lens[k]) == 0, "rows dec data %u (scattered) waves %u D %u", k, waves, force_d); }
            else CHECK(memcmp(out.p + misalign, in.p + misalign, doff[n] - misalign) == 0, "rows dec data waves %u D %u var %d", waves, force_d, var);
            CHECK(memcmp(tags2.data(), tags.data(), 16 * n) == 0, "rows dec tags waves %u D %u var %d", waves, force_d, var);
        }
    }
}

// emulated k_wipe_failed: every lane of its grid (a wave per packet, four waves per workgroup) through wipe_failed_lane, the kernel's own code
static void emu_wipe_failed(unsigned char *out, const int *auth, const u64 *data_off, u32 n_pkts, u32 pkt_len, const u64 *out_ptr, const u32 *len_arr, const RowsHdr *hdr) {
    for (u32 b = 0; b < (n_pkts + 3u) / 4u; b++)
        for (u32 t = 0; t < 256; t++) wipe_failed_lane(out, auth, data_off, n_pkts, pkt_len, out_ptr, len_arr, hdr, b * 4u + (t >> 6), t & 63u);
}
static unsigned char wipe_mark(size_t i) { return (unsigned char)((i * 131u + 7u) | 1u); }      // never zero
// one wipe over a heap buffer of exactly `sz` bytes (out = its byte `mis`) filled with wipe_mark: afterwards exactly the ranges `zeroed` (relative to out) are zeros.
// Offsets that fall, gaps of 2^29 and lengths of 2^28 point far outside the buffer: a wipe that went there is a heap overflow the sanitizer build reports.
static void wipe_case(const char *name, size_t sz, u32 mis, const std::vector<u64> &doff, const std::vector<int> &auth, const std::vector<std::pair<u64, u64>> &zeroed,
                      u32 pkt_len = 0, bool refused = false) {
    unsigned char *buf = (unsigned char *)malloc(sz);
    for (size_t i = 0; i < sz; i++) buf[i] = wipe_mark(i);
    RowsHdr hdr;
    memset(&hdr, 0, sizeof hdr);
    hdr.bad = refused ? 1u : 0u;
    const u32 n = (u32)auth.size();
    emu_wipe_failed(buf + mis, auth.data(), doff.empty() ? nullptr : doff.data(), n, pkt_len, nullptr, nullptr, refused ? &hdr : nullptr);
    std::vector<unsigned char> want(sz);
    for (size_t i = 0; i < sz; i++) want[i] = wipe_mark(i);
    for (auto &z : zeroed) memset(want.data() + mis + z.first, 0, z.second - z.first);
    size_t first = sz;
    for (size_t i = 0; i < sz && first == sz; i++) if (buf[i] != want[i]) first = i;
    CHECK(first == sz, "wipe %s: byte %zu of %zu is %02x, wanted %02x", name, first, sz, first < sz ? buf[first] : 0, first < sz ? want[first] : 0);
    free(buf);
}
static void test_wipe() {
    const u64 G29 = 1ull << 29, L28 = 1ull << 28;
    // offsets that fall: packet 1 (100 -> 40) and packet 4 (250 -> 0) are left alone whatever auth says; packet 3 [200, 250) is zeroed
    wipe_case("falling", 300, 0, {0, 100, 40, 200, 250, 0}, {1, 0, 1, 0, 0}, {{200, 250}});
    wipe_case("falling by one", 64, 0, {0, 30, 29, 64}, {0, 0, 0}, {{0, 30}, {29, 64}});
    // a gap of 2^29 bytes: packet 1 seems to be 2^29 bytes long (never wiped), packet 0 is
    wipe_case("gap", 128, 0, {0, 64, 64 + G29, 64 + G29 + 10}, {0, 0, 1}, {{0, 64}});
    // fixed-size records: 2^28 bytes each is beyond the bound (aesgcm_wipe_failed_dev), 100 bytes from an odd address are not
    wipe_case("pkt_len 2^28", 64, 0, {}, {0}, {}, (u32)L28);
    wipe_case("pkt_len 100", 311, 3, {}, {0, 1, 0}, {{0, 100}, {200, 300}}, 100);
    // odd byte addresses, lengths around 16-byte boundaries, zero-length packets between them and at the very end of the buffer
    for (u32 mis : {1u, 3u, 7u, 8u, 15u}) {
        const std::vector<u64> lens = {1, 15, 16, 17, 0, 31, 33, 0, 1000, 4097, 2, 0};
        std::vector<u64> doff = {0};
        for (u64 l : lens) doff.push_back(doff.back() + l);
        std::vector<int> auth;
        std::vector<std::pair<u64, u64>> z;
        for (size_t i = 0; i < lens.size(); i++) {
            auth.push_back((int)((i + mis) % 3 == 0));
            if (!auth.back() && lens[i]) z.push_back({doff[i], doff[i + 1]});
        }
        wipe_case("odd addresses", mis + doff.back(), mis, doff, auth, z);
    }
    // a refused call (hdr->bad): every verdict zero, nothing wiped; the same call not refused wipes everything
    wipe_case("refused", 4200, 5, {0, 1000, 1000, 3000, 4100}, {0, 0, 0, 0}, {}, 0, true);
    wipe_case("not refused", 4200, 5, {0, 1000, 1000, 3000, 4100}, {0, 0, 0, 0}, {{0, 4100}});
    // the scattered form (aesgcm_messages_crypt_dev): addresses and 32-bit lengths; 2^28 bytes is left alone, 2^28 - 1 bytes is wiped to the last byte
    {
        const size_t sa = 64, sb = L28 - 1;
        unsigned char *a = (unsigned char *)malloc(sa), *b = (unsigned char *)malloc(sb);
        for (size_t i = 0; i < sa; i++) a[i] = wipe_mark(i);
        memset(b, 0xEE, sb);
        const u64 ptr[5] = {(u64)(uintptr_t)a, (u64)(uintptr_t)b, (u64)(uintptr_t)(a + sa), (u64)(uintptr_t)(a + 5), (u64)(uintptr_t)(a + 40)};
        const u32 len[5] = {(u32)L28, (u32)(L28 - 1), 0, 17, 0xFFFFFFFFu};
        const int auth[5] = {0, 0, 0, 0, 0};
        emu_wipe_failed(nullptr, auth, nullptr, 5, 0, ptr, len, nullptr);
        size_t bad_a = sa, bad_b = sb;
        for (size_t i = 0; i < sa && bad_a == sa; i++) if (a[i] != ((i >= 5 && i < 22) ? 0 : wipe_mark(i))) bad_a = i;
        static const unsigned char zeros[4096] = {};
        for (size_t i = 0; i < sb && bad_b == sb; i += 4096) if (memcmp(b + i, zeros, sb - i < 4096 ? sb - i : 4096)) bad_b = i;
        CHECK(bad_a == sa && bad_b == sb, "wipe scattered: first wrong byte %zu (of 64), %zu (of 2^28 - 1)", bad_a, bad_b);
        RowsHdr hdr;
        memset(&hdr, 0, sizeof hdr);
        hdr.bad = 1;
        for (size_t i = 0; i < sa; i++) a[i] = wipe_mark(i);
        emu_wipe_failed(nullptr, auth, nullptr, 5, 0, ptr, len, &hdr);
        for (size_t i = 0; i < sa && bad_a == sa; i++) if (a[i] != wipe_mark(i)) bad_a = i;
        CHECK(bad_a == sa, "wipe scattered, refused: byte %zu written", bad_a);
        free(a); free(b);
    }
}

// ================================================================================================
// The alignment grid of the packet kernels (tests/pkt_grid.py states the same rules for the GPU tests, tests/test_gpu_pkt_grid.py): every (start residue, length)
// cell through every form of the lane code the kernels instantiate -- pktl_lane with four T-tables as k_pktl launches it (768-lane form, ILP form, with the launch's
// PktDesc records), the scattered form of k_pktls, and the lane groups of k_pktg / k_pktgs -- in arenas with canary guards, input and output at differing residues.
// After EVERY packet the bytes around it (GRID_GUARD on either side) are compared with what they should be, so a store outside the packet names its cell; the whole
// arenas are compared at the end.  Reads may be anywhere inside the arena; what lies outside it is the sanitizer build's.
// ================================================================================================
static const u32 GRID_GUARD = 256;
static const uint8_t GRID_CANARY_IN = 0xC3, GRID_CANARY_OUT = 0x5E;
static const u32 GRID_AADS[13] = {0, 1, 12, 15, 16, 17, 20, 28, 31, 32, 33, 40, 20};       // period 13: coprime to the residues' 16 and 128 and to the forged tags' 7
static void grid_group_edges(std::vector<u32> &v, u32 G) { for (u32 m : {G - 1, G, G + 1, 2 * G - 1, 2 * G, 2 * G + 1}) for (int d = -1; d <= 1; d++) v.push_back((u32)(16 * (int)m + d)); }
// all: every length 0 .. 272 and the group edges of every lane group; else L_c -- the edges of the lane's loops -- and the group edges of G lanes (0: none)
static std::vector<u32> grid_lengths(bool all, u32 G) {
    std::vector<u32> v;
    if (all) { for (u32 l = 0; l <= 272; l++) v.push_back(l); for (u32 g : {4u, 8u, 16u, 64u}) grid_group_edges(v, g); }
    else {
        v = {0, 1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 79, 80, 81, 111, 112, 113, 127, 128, 129, 143, 144, 145, 191, 192, 193, 255, 256, 257, 271, 272};
        if (G) grid_group_edges(v, G);
    }
    std::sort(v.begin(), v.end());
    v.erase(std::unique(v.begin(), v.end()), v.end());
    return v;
}
// byte-packed packets such that every length of L starts at every residue mod M: fillers of 1 .. M - 1 bytes (ordinary packets) steer the starts
static void grid_walk(std::vector<u32> &lens, u64 &pos, u32 M, const std::vector<u32> &L) {
    for (u32 l : L) {
        std::vector<char> seen(M, 0);
        for (u32 k = 0; k < M; k++) {
            u32 f = 0;
            while (seen[(pos + f) % M]) f++;
            if (f) { lens.push_back(f); pos += f; }
            seen[pos % M] = 1;
            lens.push_back(l); pos += l;
        }
    }
}
struct GridArena {
    uint8_t *p; size_t n;
    GridArena(size_t n_, uint8_t fill) : n(n_) { p = (uint8_t *)aligned_alloc(128, (n + 127) / 128 * 128); memset(p, fill, n); }       // on a 128-byte line: offsets are residues
    GridArena(const GridArena &o) : n(o.n) { p = (uint8_t *)aligned_alloc(128, (n + 127) / 128 * 128); memcpy(p, o.p, n); }
    ~GridArena() { free(p); }
};
// the bytes [lo - GRID_GUARD, hi + GRID_GUARD) of two arenas: the first that differs, relative to lo, or INT64_MIN
static long long grid_window_diff(const GridArena &got, const GridArena &want, u64 lo, u64 hi) {
    const u64 a = lo > GRID_GUARD ? lo - GRID_GUARD : 0, b = hi + GRID_GUARD < got.n ? hi + GRID_GUARD : got.n;
    if (!memcmp(got.p + a, want.p + a, b - a)) return INT64_MIN;
    for (u64 i = a; i < b; i++) if (got.p[i] != want.p[i]) return (long long)i - (long long)lo;
    return INT64_MIN;
}
enum GridForm { GF_LANE, GF_LANE_ILP, GF_LANE_DESC, GF_G4, GF_G8, GF_G16, GF_WAVE };
static const char *const GRID_FORM_NAME[] = {"lane", "lane_ilp", "lane_desc", "g4", "g8", "group16", "wave"};
static u32 grid_form_G(int form) { return form == GF_G4 ? 4u : form == GF_G8 ? 8u : form == GF_G16 ? 16u : form == GF_WAVE ? 64u : 0u; }
// one packet through one form of the lane code: pktl_lane as k_pktl / k_pktls instantiate it (AESGCM_PKTL_T4 tables; ILP only without SC), or a lane group
static uint4 grid_packet(const KeyMaterial *km, int form, bool sc, int dec, const PktParams &p, const unsigned char *smem, u32 pkt, const PktDesc *desc) {
    constexpr bool T4 = AESGCM_PKTL_T4 != 0;
    const u32 lane = (pkt * 7u + 3u) % 64u;
    if (form <= GF_LANE_DESC) {
        const PktDesc *d = form == GF_LANE_DESC ? desc + pkt : nullptr;
        const u32 k = d ? 0u : pkt;                              // (as pktl_body passes them)
#define GL(NR) do { if (sc) { if (dec) pktl_lane<NR, 1, T4, false, true>(km, p, smem, k, lane, d); else pktl_lane<NR, 0, T4, false, true>(km, p, smem, k, lane, d); } \
                    else if (form == GF_LANE_ILP) { if (dec) pktl_lane<NR, 1, T4, true, false>(km, p, smem, k, lane, d); else pktl_lane<NR, 0, T4, true, false>(km, p, smem, k, lane, d); } \
                    else { if (dec) pktl_lane<NR, 1, T4, false, false>(km, p, smem, k, lane, d); else pktl_lane<NR, 0, T4, false, false>(km, p, smem, k, lane, d); } } while (0)
        if (km->nr == 10) GL(10); else if (km->nr == 12) GL(12); else GL(14);
#undef GL
        uint4 t; memcpy(&t, p.tags + (size_t)pkt * 16, 16);
        return t;
    }
    const u32 lg = form == GF_G4 ? 2u : form == GF_G8 ? 3u : form == GF_G16 ? 4u : 6u, extra = (pkt % 3 == 1) ? 2 : 0, grp = pkt & ((64u >> lg) - 1u);
    if (sc) return lg == 2 ? emu_pktg<2, true>(km, dec, p, smem, pkt, extra, grp) : lg == 3 ? emu_pktg<3, true>(km, dec, p, smem, pkt, extra, grp) : emu_pktg<4, true>(km, dec, p, smem, pkt, extra, grp);
    return lg == 2 ? emu_pktg<2>(km, dec, p, smem, pkt, extra, grp) : lg == 3 ? emu_pktg<3>(km, dec, p, smem, pkt, extra, grp) : lg == 4 ? emu_pktg<4>(km, dec, p, smem, pkt, extra, grp)
                                                                                                                              : emu_pktg<6>(km, dec, p, smem, pkt, extra, grp);
}
static const unsigned char *grid_lds(const KeyMaterial *km, int form) {
    if (form <= GF_LANE_DESC) {
        static unsigned char smem[AESGCM_LDS_BYTES_T4] __attribute__((aligned(16)));
        const u32 WG = form == GF_LANE_ILP ? 512u : (u32)AESGCM_PKTL_WG;            // (AESGCM_PKTL_WG_ILP)
        memset(smem, 0xEE, sizeof smem);
        for (u32 tid = 0; tid < WG; tid++) { main_fill_lds(smem, km, &g_tb, tid, true, WG, GH_TAB_H); fill_lds_t4(smem, &g_tb, tid, WG); }
        return smem;
    }
    static unsigned char smem[PKTG_LDS_BYTES(6)] __attribute__((aligned(16)));
    const int lg = form == GF_G4 ? 2 : form == GF_G8 ? 3 : form == GF_G16 ? 4 : 6;
    memset(smem, 0xEE, sizeof smem);
    for (u32 tid = 0; tid < AESGCM_PKT_WG; tid++) pktg_fill_lds(smem, km, &g_tb, tid, AESGCM_PKT_WG, lg);
    return smem;
}
// One grid through one form.  in_at / out_at / aad_at: where message k lies in its arena (packed form: in_at == out_at, consecutive; the output arena is then used
// from byte out_shift on, so that the two residues differ).  Encrypt out of place, then decrypt the ORACLE's ciphertext with one tag in seven forged: in place
// (packed) or to a third arena at the input's places (scattered).  Returns the packets run.
struct GridLayout { std::vector<u32> lens, aads; std::vector<u64> in_at, out_at, aad_at; u64 size_in, size_out, size_aad; bool packed; };
static u32 grid_run(Emu &E, const uint8_t *key, int key_len, int form, bool sc, const GridLayout &g, u64 seed) {
    const u32 n = (u32)g.lens.size(), out_shift = g.packed ? 5u : 0u;
    const char *fname = GRID_FORM_NAME[form];
    const int fails_before = g_fail;
    GridArena in(g.size_in, GRID_CANARY_IN), aad(g.size_aad, GRID_CANARY_IN), out(g.size_out + 16, GRID_CANARY_OUT);
    auto ivs = rnd(12 * (size_t)n, seed + 2);
    {
        auto r = rnd(g.size_in, seed + 3), ra = rnd(g.size_aad, seed + 1);
        for (u32 k = 0; k < n; k++) { memcpy(in.p + g.in_at[k], r.data() + g.in_at[k], g.lens[k]); memcpy(aad.p + g.aad_at[k], ra.data() + g.aad_at[k], g.aads[k]); }
    }
    const GridArena in0(in), aad0(aad);
    GridArena want(out), ct_in(g.packed ? in : out);                      // ct_in: the decrypt's input, the oracle's ciphertext at the output's places (packed: at the input's, guards as the input's)
    std::vector<uint8_t> rtags(16 * (size_t)n), tags(16 * (size_t)n + 16), bad(16 * (size_t)n);
    for (u32 k = 0; k < n; k++) {
        std::vector<uint8_t> ref(g.lens[k] + 16);
        orc_gcm_crypt(0, key, key_len, ivs.data() + 12 * k, aad.p + g.aad_at[k], g.aads[k], in.p + g.in_at[k], g.lens[k], ref.data(), rtags.data() + 16 * k);
        memcpy(ct_in.p + (g.packed ? g.in_at[k] : g.out_at[k]), ref.data(), g.lens[k]);
    }
    // the call's arrays as the kernels read them
    std::vector<u64> doff(n + 1), aoff(n + 1), in_ptr(n), out_ptr(n), aad_ptr(n);
    std::vector<int> auth(n);
    std::vector<PktDesc> desc(n);
    RowsHdr hdr;
    PktParams p;
    auto setup = [&](const uint8_t *src, uint8_t *dst, const std::vector<u64> &src_at, const std::vector<u64> &dst_at) {
        memset(&p, 0, sizeof p); memset(&hdr, 0, sizeof hdr);
        p.ivs = ivs.data(); p.tags = tags.data(); p.n_pkts = n;
        LenSrc ls; memset(&ls, 0, sizeof ls);
        DescSrc ds = {desc.data(), ivs.data(), nullptr, nullptr, nullptr};
        if (g.packed) {
            for (u32 k = 0; k < n; k++) { doff[k] = src_at[k]; aoff[k] = g.aad_at[k]; }
            doff[n] = src_at[n - 1] + g.lens[n - 1]; aoff[n] = g.aad_at[n - 1] + g.aads[n - 1];
            p.in = src; p.out = dst; p.aad = aad.p; p.data_off = doff.data(); p.aad_off = aoff.data();
            p.aligned = ((((uintptr_t)src | (uintptr_t)dst) & 15) == 0) ? 1u : 0u;
            ls.off = doff.data(); ls.aoff = aoff.data();
        } else {
            for (u32 k = 0; k < n; k++) { in_ptr[k] = (u64)(uintptr_t)(src + src_at[k]); out_ptr[k] = (u64)(uintptr_t)(dst + dst_at[k]); aad_ptr[k] = (u64)(uintptr_t)(aad.p + g.aad_at[k]); }
            hdr.sc_in = (u64)(uintptr_t)in_ptr.data(); hdr.sc_out = (u64)(uintptr_t)out_ptr.data(); hdr.sc_aad = (u64)(uintptr_t)aad_ptr.data();
            hdr.sc_len = (u64)(uintptr_t)g.lens.data(); hdr.sc_alen = (u64)(uintptr_t)g.aads.data();
            p.route = &hdr; p.scattered = 1; p.aligned = 1;
            ls.len_arr = g.lens.data(); ls.alen_arr = g.aads.data();
            ds.in_ptr = in_ptr.data(); ds.out_ptr = out_ptr.data(); ds.aad_ptr = aad_ptr.data();
        }
        for (u32 k = 0; k < n; k++) desc[k] = len_src_desc(ls, ds, k, g.lens[k], g.aads[k]);       // what k_len_scatter writes for a lane per packet
        if (form == GF_LANE_DESC) p.desc = desc.data();
    };
    const unsigned char *smem = grid_lds(&E.km, form);
    // encrypt, out of place
    setup(in.p, out.p + out_shift, g.in_at, g.out_at);
    for (u32 k = 0; k < n; k++) {
        const uint4 t = grid_packet(&E.km, form, sc, 0, p, smem, k, desc.data());
        const u64 at = out_shift + g.out_at[k];
        memcpy(want.p + at, ct_in.p + (g.packed ? g.in_at[k] : g.out_at[k]), g.lens[k]);
        const long long d = grid_window_diff(out, want, at, at + g.lens[k]);
        CHECK(d == INT64_MIN && !memcmp(&t, rtags.data() + 16 * k, 16), "packet grid %s%s AES-%d enc: in %% 16 = %u (%% 128 = %u), out %% 16 = %u, len %u, aad %u at %% 16 = %u (packet %u): %s, first wrong byte %lld",
              fname, sc ? " scattered" : "", 8 * key_len, (u32)(g.in_at[k] % 16), (u32)(g.in_at[k] % 128), (u32)(at % 16), g.lens[k], g.aads[k], (u32)(g.aad_at[k] % 16), k,
              d == INT64_MIN ? "tag" : "bytes", d == INT64_MIN ? 0ll : d);
        if (g_fail != fails_before) return k;                       // the first cell is the finding
    }
    CHECK(!memcmp(out.p, want.p, out.n) && !memcmp(in.p, in0.p, in.n) && !memcmp(aad.p, aad0.p, aad.n), "packet grid %s%s AES-%d enc: arenas", fname, sc ? " scattered" : "", 8 * key_len);
    // decrypt the oracle's ciphertext: packed in place, scattered to a third arena at the input's places; one tag in seven forged, the first and the last among them
    memcpy(bad.data(), rtags.data(), bad.size());
    for (u32 k = 0; k < n; k++) if (k % 7 == 0 || k == n - 1) bad[16 * k + k % 16] ^= (uint8_t)(1u << (k % 8));
    GridArena back(g.packed ? ct_in : GridArena(g.size_in, GRID_CANARY_OUT));
    GridArena wantb(back);
    const GridArena ct0(ct_in);
    if (g.packed) setup(back.p, back.p, g.in_at, g.in_at); else setup(ct_in.p, back.p, g.out_at, g.in_at);
    p.expect = bad.data(); p.auth = auth.data();
    memset(tags.data(), 0, tags.size());
    for (u32 k = 0; k < n; k++) auth[k] = -1;
    for (u32 k = 0; k < n; k++) {
        const uint4 t = grid_packet(&E.km, form, sc, 1, p, smem, k, desc.data());
        const u64 at = g.in_at[k];
        memcpy(wantb.p + at, in0.p + at, g.lens[k]);
        const long long d = grid_window_diff(back, wantb, at, at + g.lens[k]);
        const bool forged = k % 7 == 0 || k == n - 1, auth_ok = form > GF_LANE_DESC || auth[k] == (forged ? 0 : 1);     // (a lane group's verdict is the kernel's, not the lane code's)
        CHECK(d == INT64_MIN && !memcmp(&t, rtags.data() + 16 * k, 16) && auth_ok, "packet grid %s%s AES-%d dec: in %% 16 = %u, out %% 16 = %u (%% 128 = %u), len %u, aad %u (packet %u): %s, first wrong byte %lld",
              fname, sc ? " scattered" : "", 8 * key_len, (u32)((g.packed ? g.in_at[k] : g.out_at[k]) % 16), (u32)(at % 16), (u32)(at % 128), g.lens[k], g.aads[k], k,
              d != INT64_MIN ? "bytes" : auth_ok ? "tag" : "verdict", d == INT64_MIN ? 0ll : d);
        if (g_fail != fails_before) return n + k;
    }
    CHECK(!memcmp(back.p, wantb.p, back.n) && (g.packed || !memcmp(ct_in.p, ct0.p, ct_in.n)) && !memcmp(aad.p, aad0.p, aad.n), "packet grid %s%s AES-%d dec: arenas", fname, sc ? " scattered" : "", 8 * key_len);
    return 2 * n;
}
// packed: every length of `l16` at every start mod 16, every length of `l128` at every start mod 128
static GridLayout grid_packed(const std::vector<u32> &l16, const std::vector<u32> &l128) {
    GridLayout g;
    g.packed = true;
    u64 pos = 0;
    grid_walk(g.lens, pos, 16, l16);
    grid_walk(g.lens, pos, 128, l128);
    const u32 n = (u32)g.lens.size();
    u64 a = GRID_GUARD, c = GRID_GUARD;
    for (u32 k = 0; k < n; k++) { g.aads.push_back(GRID_AADS[k % 13]); g.in_at.push_back(a); g.aad_at.push_back(c); a += g.lens[k]; c += g.aads[k]; }
    g.out_at = g.in_at;
    g.size_in = g.size_out = a + GRID_GUARD; g.size_aad = c + GRID_GUARD;
    // completeness
    std::vector<char> s16(16 * 4096, 0), s128(128 * 4096, 0);
    for (u32 k = 0; k < n; k++) { s16[(g.in_at[k] % 16) * 4096 + g.lens[k]] = 1; s128[(g.in_at[k] % 128) * 4096 + g.lens[k]] = 1; }
    u32 miss = 0;
    for (u32 l : l16) for (u32 r = 0; r < 16; r++) miss += !s16[r * 4096 + l];
    for (u32 l : l128) for (u32 r = 0; r < 128; r++) miss += !s128[r * 4096 + l];
    CHECK(!miss && n, "packed grid: %u cells missing", miss);
    return g;
}
// scattered: every length of L at (input residue a, output residue b) for all 16 a and `nb` values of b (16: every pair; fewer: b walks with the length), 1 .. 19
// guard bytes between neighbours in every arena
static GridLayout grid_scattered(const std::vector<u32> &L, u32 nb) {
    GridLayout g;
    g.packed = false;
    std::vector<u32> cells;                                                  // a | b << 4 | length index << 8
    for (u32 li = 0; li < L.size(); li++) for (u32 a = 0; a < 16; a++) for (u32 j = 0; j < nb; j++) cells.push_back(a | (((nb == 16 ? j : a + 1 + 5 * j + li) % 16) << 4) | (li << 8));
    const u32 n = (u32)cells.size();
    u32 step = n / 3 | 1;
    auto gcd = [](u32 x, u32 y) { while (y) { const u32 t = x % y; x = y; y = t; } return x; };
    while (gcd(step, n) != 1) step += 2;                                     // neighbours of unlike length and residue
    auto place = [](u64 pos, u32 res, u32 i) { u64 gap = (res + 16 - (pos + 1) % 16) % 16 + 1; if (gap <= 3 && i % 2) gap += 16; return pos + gap; };
    u64 a = GRID_GUARD - 1, b = GRID_GUARD - 1, c = GRID_GUARD - 1;
    std::vector<char> seen(256 * L.size(), 0);
    for (u32 i = 0; i < n; i++) {
        const u32 cell = cells[(u64)i * step % n], len = L[cell >> 8];
        g.lens.push_back(len); g.aads.push_back(GRID_AADS[i % 13]);
        a = place(a, cell & 15, i); g.in_at.push_back(a); a += len;
        b = place(b, (cell >> 4) & 15, i + 1); g.out_at.push_back(b); b += len;
        c = place(c, (5 * i + 3) % 16, i); g.aad_at.push_back(c); c += g.aads[i];
        seen[(cell >> 8) * 256 + (g.in_at[i] % 16) * 16 + g.out_at[i] % 16] = 1;
    }
    u32 hit = 0;
    for (char s : seen) hit += s;
    CHECK(hit == n && n == 16 * nb * L.size(), "scattered grid: %u of %u cells", hit, n);
    g.size_in = a + 1 + GRID_GUARD; g.size_out = b + 1 + GRID_GUARD; g.size_aad = c + 1 + GRID_GUARD;
    return g;
}
// Level 1 (the sanitizer build): L_c at every start mod 16, every form, direction and key size.  Level 2: the full grid -- every length at every start mod 16, L_c at
// every start mod 128, every residue pair of the scattered form -- for every form, the key sizes taking turns so that every form meets each of them at least at level 1's size.
static void test_packet_grid(int level) {
    const int klens[3] = {16, 24, 32};
    std::vector<uint8_t> keys[3];
    Emu *E[3];
    for (int i = 0; i < 3; i++) { keys[i] = rnd(klens[i], 7100 + i); E[i] = new Emu(keys[i].data(), klens[i], 0); }
    u32 ran = 0, turn = 0;
    for (int form = GF_LANE; form <= GF_WAVE; form++) {
        const u32 G = grid_form_G(form);
        const GridLayout small = grid_packed(grid_lengths(false, G), {}), small_sc = grid_scattered(grid_lengths(false, G), 1);
        for (int i = 0; i < 3; i++) {
            ran += grid_run(*E[i], keys[i].data(), klens[i], form, false, small, 7200 + 10 * form + i);
            if (form != GF_LANE_ILP && form != GF_WAVE) ran += grid_run(*E[i], keys[i].data(), klens[i], form, true, small_sc, 7300 + 10 * form + i);      // (no scattered instance of the ILP form or of a wave per packet)
        }
        if (level < 2) continue;
        const int i = turn++ % 3;
        ran += grid_run(*E[i], keys[i].data(), klens[i], form, false, grid_packed(grid_lengths(true, 0), grid_lengths(false, G)), 7400 + form);
        if (form != GF_LANE_ILP && form != GF_WAVE) ran += grid_run(*E[(i + 1) % 3], keys[(i + 1) % 3].data(), klens[(i + 1) % 3], form, true, grid_scattered(grid_lengths(false, G), 16), 7500 + form);
    }
    CHECK(ran > 0, "packet grid ran nothing");
    printf("packet grid: %u packets through the lane code (level %d)\n", ran, level);
    for (int i = 0; i < 3; i++) delete E[i];
}

// ================================================================================================
// The alignment grid at ROW scale (tests/rows_grid.py states the same rules for the GPU tests, tests/test_gpu_rows_grid.py): a message of 1024 R + t bytes is R whole
// rows (a run of them one piece of body_rows_lane), a tail of up to 64 blocks -- up to ROWS_SMALL_TAIL of them on the closing launch's axis, more: one right-aligned row
// (rows_tail_lane) -- and an AAD either side of ROWS_SMALL_AAD.  `lc`: nine lengths at every start mod 128; `full`: R in 0 1 2 3 4 5 9 x tails either side of every
// boundary at every start mod 16.  Byte-packed arenas with canary guards through emu_rows_nr (the planner's prefix sums, the piece walk and the lane code of k_rows and
// k_rows_close) with the library's cut and dealt blocks of 1 and 3 units: encrypt out of place with the output 5 residues off, decrypt of the ORACLE's ciphertext in
// place; whole arenas compared, a difference names the first message and its cell.
// ================================================================================================
static_assert(ROWS_SMALL_TAIL == 16u && ROWS_SMALL_AAD == 64u, "the row grid's lengths lie either side of these");
static const u32 ROWS_GRID_AADS[13] = {0, 1, 13, 16, 20, 1007, 1008, 1009, 1023, 1024, 1025, 1040, 2048 + 7};      // period 13; 64 blocks and 65
static std::vector<u32> rows_grid_lengths(bool lc) {
    if (lc) return {1023, 1024, 1024 + 1, 1024 + 16 * ROWS_SMALL_TAIL, 1024 + 16 * ROWS_SMALL_TAIL + 1, 2 * 1024 + 1023, 4 * 1024, 5 * 1024 + 17, 9 * 1024 + 257};
    std::vector<u32> v;
    for (u32 R : {0u, 1u, 2u, 3u, 4u, 5u, 9u})
        for (u32 t : {0u, 1u, 15u, 16u, 17u, 255u, 256u, 257u, 272u, 511u, 512u, 1007u, 1008u, 1009u, 1023u}) if (R || t >= 257) v.push_back(1024 * R + t);
    std::sort(v.begin(), v.end());
    return v;
}
static GridLayout rows_grid_layout(const std::vector<u32> &l16, const std::vector<u32> &l128) {
    GridLayout g;
    g.packed = true;
    u64 pos = 0;
    grid_walk(g.lens, pos, 16, l16);
    grid_walk(g.lens, pos, 128, l128);
    const u32 n = (u32)g.lens.size();
    u64 a = GRID_GUARD, c = GRID_GUARD;
    for (u32 k = 0; k < n; k++) { g.aads.push_back(ROWS_GRID_AADS[k % 13]); g.in_at.push_back(a); g.aad_at.push_back(c); a += g.lens[k]; c += g.aads[k]; }
    g.out_at = g.in_at;
    g.size_in = g.size_out = a + GRID_GUARD; g.size_aad = c + GRID_GUARD;
    // completeness: every (start, length) cell; AADs of 64 and of 65 blocks at every residue of their own
    std::vector<u64> seen;                                                   // length << 8 | modulus bit << 7 | residue
    for (u32 k = 0; k < n; k++) { seen.push_back((u64)g.lens[k] << 8 | (g.in_at[k] % 16)); seen.push_back((u64)g.lens[k] << 8 | 128 | (g.in_at[k] % 128)); }
    std::sort(seen.begin(), seen.end());
    u32 miss = 0, aad_res[2] = {0, 0};
    for (u32 l : l16) for (u32 r = 0; r < 16; r++) miss += !std::binary_search(seen.begin(), seen.end(), (u64)l << 8 | r);
    for (u32 l : l128) for (u32 r = 0; r < 128; r++) miss += !std::binary_search(seen.begin(), seen.end(), (u64)l << 8 | 128 | r);
    for (u32 k = 0; k < n; k++) if (g.aads[k] == 1024 || g.aads[k] == 1025) aad_res[g.aads[k] - 1024] |= 1u << (g.aad_at[k] % 16);
    CHECK(!miss && n && aad_res[0] == 0xFFFFu && aad_res[1] == 0xFFFFu, "row grid: %u cells missing, AAD residues %04x %04x", miss, aad_res[0], aad_res[1]);
    return g;
}
// the first byte at which two arenas differ, named by the message that owns it (or the guard in front of which message)
static void rows_grid_same(const GridArena &got, const GridArena &want, const GridLayout &g, u32 shift, u32 D, int key_len, const char *what) {
    if (!memcmp(got.p, want.p, got.n)) return;
    u64 i = 0;
    while (got.p[i] == want.p[i]) i++;
    u32 k = 0;
    const u32 n = (u32)g.lens.size();
    while (k < n && g.in_at[k] + shift + g.lens[k] <= i) k++;
    const bool guard = k == n || i < g.in_at[k] + shift;
    if (k == n) k = n - 1;
    CHECK(false, "row grid AES-%d %s D %u: arena byte %llu is %02x, wanted %02x: %s message %u (byte %lld of it): start %% 16 = %u (%% 128 = %u), out %% 16 = %u, len %u = %u rows + %u tail blocks, aad %u (%u blocks) at %% 16 = %u",
          8 * key_len, what, D, (unsigned long long)i, got.p[i], want.p[i], guard ? "a guard byte next to" : "inside", k, (long long)i - (long long)(g.in_at[k] + shift),
          (u32)(g.in_at[k] % 16), (u32)(g.in_at[k] % 128), (u32)((g.in_at[k] + shift) % 16), g.lens[k], g.lens[k] >> 10, ((g.lens[k] & 1023u) + 15u) >> 4, g.aads[k], (g.aads[k] + 15u) >> 4, (u32)(g.aad_at[k] % 16));
}
static u32 rows_grid_run(const uint8_t *key, int key_len, const GridLayout &g, u32 waves, u32 D, u64 seed) {
    Emu E(key, key_len, 0);
    const u32 n = (u32)g.lens.size(), shift = 5;
    const int fails_before = g_fail;
    GridArena in(g.size_in, GRID_CANARY_IN), aad(g.size_aad, GRID_CANARY_IN), out(g.size_out + 16, GRID_CANARY_OUT);
    auto ivs = rnd(12 * (size_t)n, seed + 2);
    {
        auto r = rnd(g.size_in, seed + 3), ra = rnd(g.size_aad, seed + 1);
        for (u32 k = 0; k < n; k++) { memcpy(in.p + g.in_at[k], r.data() + g.in_at[k], g.lens[k]); memcpy(aad.p + g.aad_at[k], ra.data() + g.aad_at[k], g.aads[k]); }
    }
    const GridArena in0(in), aad0(aad);
    GridArena want(out), ct(in);
    std::vector<uint8_t> rtags(16 * (size_t)n), tags(16 * (size_t)n + 16);
    for (u32 k = 0; k < n; k++) {
        std::vector<uint8_t> ref(g.lens[k] + 16);
        orc_gcm_crypt(0, key, key_len, ivs.data() + 12 * k, aad.p + g.aad_at[k], g.aads[k], in.p + g.in_at[k], g.lens[k], ref.data(), rtags.data() + 16 * k);
        memcpy(want.p + shift + g.in_at[k], ref.data(), g.lens[k]);
        memcpy(ct.p + g.in_at[k], ref.data(), g.lens[k]);
    }
    std::vector<u64> doff(n + 1), aoff(n + 1);
    for (u32 k = 0; k < n; k++) { doff[k] = g.in_at[k]; aoff[k] = g.aad_at[k]; }
    doff[n] = g.in_at[n - 1] + g.lens[n - 1]; aoff[n] = g.aad_at[n - 1] + g.aads[n - 1];
    auto call = [&](int dec, const uint8_t *src, uint8_t *dst) {
        RowsParams p; memset(&p, 0, sizeof p);
        p.ivs = ivs.data(); p.tags = tags.data(); p.n_pkts = n; p.aad = aad.p; p.in = src; p.out = dst; p.data_off = doff.data(); p.aad_off = aoff.data();
        memset(tags.data(), 0, tags.size());
        if (E.km.nr == 10) emu_rows_nr<10>(&E.km, dec, p, waves, D); else if (E.km.nr == 12) emu_rows_nr<12>(&E.km, dec, p, waves, D); else emu_rows_nr<14>(&E.km, dec, p, waves, D);
        for (u32 k = 0; k < n && g_fail == fails_before; k++)
            CHECK(!memcmp(tags.data() + 16 * k, rtags.data() + 16 * k, 16), "row grid AES-%d %s D %u: tag of message %u: start %% 16 = %u (%% 128 = %u), len %u = %u rows + %u tail blocks, aad %u (%u blocks) at %% 16 = %u",
                  8 * key_len, dec ? "dec" : "enc", D, k, (u32)(g.in_at[k] % 16), (u32)(g.in_at[k] % 128), g.lens[k], g.lens[k] >> 10, ((g.lens[k] & 1023u) + 15u) >> 4, g.aads[k], (g.aads[k] + 15u) >> 4, (u32)(g.aad_at[k] % 16));
    };
    call(0, in.p, out.p + shift);                                            // encrypt out of place, the output 5 residues off
    rows_grid_same(out, want, g, shift, D, key_len, "enc");
    rows_grid_same(in, in0, g, 0, D, key_len, "enc (input arena)");
    rows_grid_same(aad, aad0, g, 0, D, key_len, "enc (AAD arena)");
    if (g_fail != fails_before) return n;                                    // the first cell is the finding
    GridArena back(ct);
    call(1, back.p, back.p);                                                 // decrypt the oracle's ciphertext in place
    rows_grid_same(back, in0, g, 0, D, key_len, "dec");
    rows_grid_same(aad, aad0, g, 0, D, key_len, "dec (AAD arena)");
    return 2 * n;
}
// Level 1 (the sanitizer build): the `lc` set at every start mod 128.  Level 2: also the `full` set at every start mod 16.  Each with the library's cut (one block per
// wave) and with dealt blocks of 1 and of 3 units, the key sizes taking turns.
static void test_rows_grid(int level) {
    const int klens[3] = {16, 24, 32};
    const u32 Ds[3] = {0, 1, 3};
    u32 ran = 0;
    const GridLayout lc = rows_grid_layout({}, rows_grid_lengths(true));
    for (int i = 0; i < 3; i++) { auto key = rnd(klens[(i + 1) % 3], 7600 + i); ran += rows_grid_run(key.data(), klens[(i + 1) % 3], lc, 37, Ds[i], 7610 + 10 * i); }
    if (level >= 2) {
        const GridLayout full = rows_grid_layout(rows_grid_lengths(false), {});
        for (int i = 0; i < 3; i++) { auto key = rnd(klens[i], 7700 + i); ran += rows_grid_run(key.data(), klens[i], full, 64, Ds[i], 7710 + 10 * i); }
    }
    CHECK(ran > 0, "row grid ran nothing");
    printf("row grid: %u messages through the row code (level %d)\n", ran, level);
}

int main(int argc, char **argv) {
    int level = argc > 1 ? atoi(argv[1]) : 1;
    init_tables();
    if (argc > 2 && !strcmp(argv[2], "grid")) {                 // the alignment grids alone (what a change to the frame lane or to the row code runs first)
        test_packet_grid(level);
        test_rows_grid(level);
        printf(g_fail ? "EMUL FAILED (%d)\n" : "EMUL OK\n", g_fail);
        return g_fail ? 1 : 0;
    }
    test_units();
    test_bitslice();
    const u64 W = AESGCM_WG;     // blocks per chunk at the production Tw = 16
    const std::vector<std::pair<u64, u64>> small = {{0, 0}, {0, 1}, {0, 15}, {0, 16}, {0, 17}, {1, 0}, {20, 48}, {28, 48}, {68, 0}, {16, 63 * 16}, {17, 64 * 16}, {0, 65 * 16 + 5},
                                                    {16, (W - 1) * 16}, {17, W * 16}, {0, (W + 1) * 16 + 5}, {4095, 4097}};
    test_key(16, 0, 1, small);          // production chunking rule
    test_key(24, 1, 2, small);          // Tw = 1: every row its own chunk -> many items, in-kernel fold tables where 64*Tw*16^l is not in ptab
    test_key(32, 3, 3, small);          // Tw = 3: ragged first chunk
    // several rows per chunk (Horner with K = H^64), ragged tails, front padding, > GMAX chunks
    test_key(16, 0, 4, {{0, 16 * W * 3}, {5, 16 * W * 2 + 7}, {33, 16 * (W * 3 - 36) + 1}});
    test_key(32, 2, 5, {{0, 16 * 2048 * 2}, {16, 16 * 2048 * 2 - 16}, {40, 16 * 2048 * 3 + 13}, {1000 * 16, 16 * 6144}});
    test_key(24, 5, 6, {{7, 16 * 8192 + 9}});
    test_key(16, 1, 10, {{0, 16 * 64 * 1500 + 3}, {5, 16 * 64 * 3000}, {16, 16 * 64 * 5000 + 9}});   // 1500 / 3000 / 5000 items: k_fold with 2, 4, 8 items per wave (fold_group)
    if (level >= 3) test_key(32, 1, 11, {{0, 16ull * 64 * 65535}});
    test_key(32, 1, 9, {{3, 16 * 64 * 700 + 11}});      // 700+ chunks > GMAX -> two-stage fold with > 1 stage-1 lanes... one stage-1 workgroup
    test_shards(32, 2, 37, 203 * 16 + 5, 8, 77);
    test_shards(16, 0, 0, 16 * (W * 5 + 100) + 3, 3, 78);
    test_shards(24, 1, 20, 16 * 7, 8, 79);      // fewer blocks than ranks: some shards are empty
    test_stream(32, 2, 40, 1000, 16, 90);
    test_stream(16, 0, 0, 16 * (W * 4 + 52) + 9, 16 * (W + 188), 91);
    test_stream(24, 3, 16 * 40 + 3, 33, 16 * 8, 92);
    test_keystream_and_ghash(55);
    // k_body: T = 1, 2, 3 rows per chunk; lengths chosen so head, tail and ragged end are all non-trivial
    test_body(16, 1, 0, 16 * 3000 + 5, 101);
    test_body(24, 2, 20, 16 * (254 + 2048 * 3 + 777) + 11, 102);
    test_body(32, 3, 37, 16 * 9000, 103);
    test_body(32, 1, 16, 16 * 254 + 16 * 1024 * 2, 104);          // head = 254 blocks exactly, empty tail
    test_body(16, 2, 0, 16 * 256 * 2 * 6, 106);                     // no AAD, no head, no tail: the whole message is one body (direct tag path)
    test_body(32, 1, 0, 16 * 256 * 300, 107);                       // ... with enough items for a k_fold level: its ten workgroups close the tag themselves (FoldClose)
    test_body(24, 3, 0, 16 * 256 * 3 * 40, 116);                    // ... three rows per chunk: the weight of the first workgroup is H^(24576), digit 24 of radix 1024
    test_body(16, 1, 0, 16 * 256 * 7, 108, true);                   // cyclic rows: 28 rows, the other strands leave zero items; the whole message is the body
    test_body(32, 2, 21, 16 * (100 + 256 * 40 + 70) + 3, 109, true); // ... with AAD (a front row), a ragged partial last row, and as shards from odd first blocks (head blocks in the front rows)
    test_body(24, 1, 16 * 70 + 3, 16 * 64 * 9 + 1023, 112, true);   // two front rows of AAD, the longest last row there is (63 blocks + 15 bytes = 64 blocks)
    test_body(16, 1, 16 * 64, 16 * 64 * 5 + 16, 113, true);         // AAD fills its row exactly (no front padding), one whole block behind the body
    test_body(32, 1, 1, 16 * 64 * 3 + 1, 114, true);                 // one byte of AAD, one byte behind the body
    test_batch_pieces();
    test_wipe();
    test_packets(16, 61); test_packets(24, 62); test_packets(32, 63);
    test_packet_grid(level);
    test_rows_grid(level);
    // many messages by rows: offset arrays with every kind of length (empty, shorter than a block, tails of 63 blocks + 15 bytes = two tail rows, whole super-rows,
    // 1 .. 3 rows behind them), AAD of none / a ragged block / more than a row; fixed-size records; one block per wave for few and for many waves (cuts in the
    // middle of strands), dealt blocks of 1 / 2 / 3 / 7 units
    const std::vector<u32> rl = {0, 1, 15, 16, 1023, 1024, 1040, 4096, 4097, 5 * 1024 + 1008 + 15, 3 * 4096 + 2 * 1024 + 17, 9 * 4096, 7 * 4096 + 3 * 1024 + 1023};
    const std::vector<u32> ra = {0, 20, 0, 16, 1, 0, 33, 0, 13, 1024 + 7, 0, 8, 2048};
    test_rows(16, 201, 5, 0, true, rl, ra);
    test_rows(24, 208, 64, 0, true, rl, ra);
    test_rows(32, 209, 4096, 1, true, rl, ra);
    test_rows(32, 202, 16, 3, true, {10 * 4096 + 5, 0, 4096 * 7, 3 * 1024, 1024 * 6 + 100}, {0, 0, 12, 5, 0});
    test_rows(24, 203, 7, 0, true, {65536, 65536 + 1024 + 3, 20000, 131072 + 17}, {20, 0, 28, 0});
    test_rows(32, 204, 3, 0, false, {65536, 65536, 65536}, {0, 0, 0});            // 65 units per message, one message per wave
    test_rows(16, 210, 13, 0, false, {65536, 65536, 65536}, {0, 0, 0});           // 15 units per wave: cuts inside the strands
    test_rows(16, 205, 16, 2, false, {4096 * 5 + 2048 + 9, 4096 * 5 + 2048 + 9, 4096 * 5 + 2048 + 9, 4096 * 5 + 2048 + 9, 4096 * 5 + 2048 + 9}, {13, 13, 13, 13, 13});
    test_rows(24, 211, 16, 7, false, {4096 * 5 + 2048 + 9, 4096 * 5 + 2048 + 9, 4096 * 5 + 2048 + 9}, {0, 0, 0});
    test_rows(24, 206, 16, 0, false, {700, 700}, {0, 0});                       // records shorter than a row: no strand at all, tails only
    test_rows(32, 207, 4, 2, true, {4096 * 3 + 5, 9000, 1024 * 5}, {7, 0, 16}, 5);   // packed back to back from an odd byte address
    test_rows(32, 212, 3, 0, true, {0, 0, 0, 2048, 0, 1024, 1024 + 1009, 0, 0}, {0, 0, 0, 0, 0, 0, 0, 0, 0});   // messages without a unit (empty, no AAD) first, in a row and last; a tail of 64 blocks
    test_rows(16, 213, 5, 1, true, {0, 0, 3000, 0}, {0, 0, 0, 0});
    test_rows(24, 214, 4, 0, false, {0, 0, 0}, {0, 0, 0});                       // fixed-size records of no bytes: no unit in the whole call, the closing makes the tags
    test_rows(24, 215, 4, 0, false, {0, 0, 0}, {5, 5, 5});                       // ... with AAD: an AAD unit each
    test_rows(32, 216, 4, 0, false, {1024, 1024, 1024, 1024, 1024}, {0, 0, 0, 0, 0});   // one row and nothing else per message
    test_rows(16, 217, 2, 0, false, {2033, 2033, 2033}, {0, 0, 0});              // a tail of 64 blocks (the last one byte long)
    test_rows(32, 218, 6, 0, true, {16400, 16400, 100, 16384 + 1023, 0, 5000, 16, 40 * 16 + 3, 2048 + 700}, {13, 13, 1024, 1025, 20, 0, 1023, 600, 16});   // short AADs and tails share units and straddle them; an AAD of exactly 64 blocks; one of 65 (a unit of its own)
    test_rows(24, 219, 5, 2, false, {16400, 16400, 16400, 16400, 16400, 16400, 16400}, {13, 13, 13, 13, 13, 13, 13});      // TLS-shaped records: 2 + 1 blocks of smalls each
    test_rows(16, 220, 9, 0, false, {1024 + 40 * 16, 1024 + 40 * 16, 1024 + 40 * 16, 1024 + 40 * 16, 1024 + 40 * 16}, {30 * 16 + 1, 30 * 16 + 1, 30 * 16 + 1, 30 * 16 + 1, 30 * 16 + 1});   // 31 + 40 blocks per message: every unit boundary inside a segment
    test_rows(32, 221, 3, 1, false, {700, 700, 700}, {2000, 2000, 2000});          // a long AAD (125 blocks) and a tail, no row
    test_rows(32, 222, 6, 0, 2, rl, ra);                                         // messages wherever they live: the lengths of the first case, every message in buffers of its own
    test_rows(16, 223, 4, 2, 2, {16400, 0, 100, 16384 + 1023, 5000, 16, 2048 + 700, 65536 + 1}, {13, 0, 1024, 1025, 0, 20, 16, 0}, 7);
    test_rows(24, 224, 5, 0, 2, {4096, 0, 1024, 3000}, {0, 0, 0, 0});              // ... without AAD arrays
    // ROUTED calls (round 6): the messages below the mark (data + AAD) are the packet kernels', the others go by rows -- the same lengths at three marks: a few
    // small ones, most of them, all of them (no unit in the whole call)
    for (u32 mark : {1024u, 4160u, 200000u}) {
        g_route_min = mark;
        test_rows(16, 230, 5, 0, true, rl, ra);
        test_rows(32, 231, 4, 2, 2, {16400, 0, 100, 16384 + 1023, 5000, 16, 2048 + 700, 65536 + 1}, {13, 0, 1024, 1025, 0, 20, 16, 0}, 7);
        test_rows(24, 232, 3, 0, true, {0, 0, 0, 2048, 0, 1024, 1024 + 1009, 0, 0}, {0, 0, 0, 0, 0, 0, 0, 0, 0});
        g_route_min = 0;
    }
    for (u64 nn = 1, prev = 4; nn < (1u << 22); nn += 1 + nn / 7) {               // the packet kernel shape a routed call takes for nn short messages: never more lanes per packet as they get more
        const u32 lg = route_pick_lg(256, nn);
        CHECK((lg == 0 || lg == 2 || lg == 3 || lg == 4) && lg <= prev, "route_pick_lg(%llu) = %u after %llu", (unsigned long long)nn, lg, (unsigned long long)prev);
        const u32 d = pktg_deal(256, nn, lg ? lg : 2);
        CHECK(d >= (64u >> (lg ? lg : 2)) && d <= 64u && d % (64u >> (lg ? lg : 2)) == 0, "pktg_deal(%llu, %u) = %u", (unsigned long long)nn, lg, d);
        prev = lg;
    }
    if (level > 1) {
        test_key(32, 1, 7, {{123, 16 * 64 * 1100 + 11}});     // 1100 chunks: two stage-1 workgroups
        test_key(16, 0, 8, {{0, 16 * W * 600}});              // production rule, > GMAX chunks of Tw = 16
        test_key(24, 1, 10, {{5, 16 * 64 * 4200 + 3}});        // 4200 one-row chunks: three k_fold levels
        test_body(32, 1, 9, 16 * (200 + 256 * 1100) + 7, 105);  // 4400 body items: interleaved first level + two more
        test_body(24, 1, 0, 16 * 64 * 4096, 110, true);        // cyclic rows: every strand exactly one row (4 MiB)
        test_body(32, 1, 5, 16 * (31 + 64 * 5333 + 50) + 9, 111, true);     // 5333 body rows + a front row: strands of two and of one, residues rotated
        test_body(16, 1, 16 * 64 * 3 + 7, 16 * 64 * 4200, 115, true);       // four front rows, the first strands start with them and go on with body rows
    }
    printf(g_fail ? "EMUL FAILED (%d)\n" : "EMUL OK\n", g_fail);
    return g_fail ? 1 : 0;
}
