// aesgcm_keytab_kernels.hip -- the kernels of key tables (gfx950) and their launchers; the host side is aesgcm_keytab.hip.
//
//   k_kt_setup<NR>          a thread per slot: aes_kexp, H = E_K(0), H^(2^j) for j = 0 .. 6, then the slot's `set` marker.
//   k_kt_batch<NR,DEC,LG>   k_batch3's one pass (8, 16 or 64 lanes per packet, the same dispenser and lane layout) with the key material read from the packet's
//                           slot: no aes_kexp, no E_K(0), no squaring chain in front of the block loop.  E_K(J0) stays per packet (it depends on the IV).
//                           A packet it cannot take -- slot out of range or unset, data / AAD range falling or of 2^28 bytes or more -- reads nothing but its
//                           slot number and offsets: output untouched, tag zero, auth 0, its index into the table's status word (atomicMin).
#include "aesgcm_keytab.h"
#include "aesgcm_lanes.h"

template <int NR>
__global__ __launch_bounds__(256) void k_kt_setup(const DevTables *__restrict__ tb, const KtSetupParams s) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const u32 tid = threadIdx.x;
    main_fill_lds(smem, nullptr, tb, tid, false, 256u);          // T0 | T2 (the S-box of the key schedule is byte 1 of T0)
    __syncthreads();
    const u32 i = blockIdx.x * 256u + tid;
    if (i >= s.n) return;
    const u32 slot = s.slots ? s.slots[i] : s.first + i;
    if (slot >= s.n_slots) { atomicMin(s.status, i); return; }
    const u32 lb = (tid & 31u) << 2;
    u32 rk[4 * (NR + 1)];
    batch_key_expand<NR>(s.keys + (size_t)i * (4 * (NR - 6)), rk, smem, lb);
    u32 s0 = rk[0], s1 = rk[1], s2 = rk[2], s3 = rk[3];
    aes_rounds_lds<NR>(s0, s1, s2, s3, rk, smem, lb);            // H = E_K(0^128)
    G128 h = mo_to_be(make_uint4(s0, s1, s2, s3));
    KtSlot *d = s.tab + slot;
#pragma unroll
    for (int q = 0; q < NR + 1; q++) *reinterpret_cast<uint4 *>(d->rk + 4 * q) = make_uint4(rk[4 * q], rk[4 * q + 1], rk[4 * q + 2], rk[4 * q + 3]);
#pragma unroll
    for (int j = 0; j < KT_HPOW; j++) {
        d->hpow[j] = make_uint4(h.w[0], h.w[1], h.w[2], h.w[3]);
        h = gf_sqr(h);
    }
    d->nr = NR;
    __threadfence();
    d->set = KT_SET;
}

template <int NR, int DEC, int LG>                       // DEC: 0 encrypt, 1 decrypt
__global__ __launch_bounds__(BATCH3_LANES(NR), (BATCH3_LANES(NR) + 255) / 256) void k_kt_batch(const DevTables *__restrict__ tb, const KtParams kp) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const BatchParams &p = kp.b;
    constexpr u32 G = 1u << LG, P = 64u >> LG;
    // LDS as k_batch3: T-tables, then one (8 lanes per packet) or two 512-byte table slots per packet, then 32 bytes per packet for its H and E_K(J0)
    constexpr u32 GRP_TAB = BATCH3_GROUP_LDS_LG(LG) - 32u, WAVES = BATCH3_LANES(NR) / 64u, HSLOTS = BATCH3_LDS_TAB_OFF + WAVES * P * GRP_TAB;
    static_assert(BATCH3_LDS_TAB_OFF % 256u == 0 && GRP_TAB % 256u == 0, "k_kt_batch: table slots are 256-byte aligned");
    constexpr bool ONE_TAB = LG < 4;
    constexpr bool PAIR = BATCH3_PAIR && BATCH3_PERM && BATCH3_DR && LG == 3;
    const u32 tid = threadIdx.x, lane = tid & 63u;
    main_fill_lds(smem, nullptr, tb, tid, false, BATCH3_LANES(NR));
    __syncthreads();
    const u32 lb = (lane & 31u) << 2;
    const u32 wave_id = (u32)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
    const u32 wave_tab = BATCH3_LDS_TAB_OFF + wave_id * P * GRP_TAB, wave_hs = HSLOTS + wave_id * P * 32u;
    const u32 K = p.deal, nb = (p.n_pkts + K - 1) / K;
    u32 pk0 = 0, pk_end = 0;
    for (u32 guard = 0; guard <= p.n_pkts; ++guard, pk0 += P) {      // bounded on purpose (as every dispenser loop)
        if (pk0 >= pk_end) {
            u32 b = 0;
            if (lane == 0) b = atomicAdd(p.counter, 1u) - p.counter_base;
            b = __builtin_amdgcn_readfirstlane(b);
            if (b >= nb) break;
            pk0 = b * K;
            pk_end = pk0 + K < p.n_pkts ? pk0 + K : p.n_pkts;
        }
        u32 grp, l;
        batch3_pos<LG>(lane_id_fresh(), grp, l);
        const u32 tabA = wave_tab + grp * GRP_TAB, hsA = wave_hs + grp * 32u;
        const u32 tabAp = wave_tab + (grp ^ 3u) * GRP_TAB;
        const bool pair_first = (grp & 2u) == 0;
        const bool act = pk0 + grp < pk_end;                 // groups past the end shadow the first packet; their stores are masked
        const u32 pkt = batch_map(p, act ? pk0 + grp : pk0);
        // ---- the packet's slot and ranges; a packet that fails any check reads nothing else (slot 0 stands in for its key material) and stores only its zero tag
        const u32 slot = kp.slots[pkt];
        bool bad = slot >= kp.n_slots;
        const KtSlot *ks = kp.tab + (bad ? 0u : slot);
        u32 pkt_len = p.pkt_len, aad_len = p.aad_len;
        u64 doff = (u64)pkt * p.pkt_len, aoff = (u64)pkt * p.aad_len;
        if (p.data_off) { const u64 e = p.data_off[pkt + 1]; doff = p.data_off[pkt]; bad |= e < doff || e - doff >= ((u64)1 << 28); pkt_len = (u32)(e - doff); }
        if (p.aad_off) { const u64 e = p.aad_off[pkt + 1]; aoff = p.aad_off[pkt]; bad |= e < aoff || e - aoff >= ((u64)1 << 28); aad_len = (u32)(e - aoff); }
        bad |= ks->set != KT_SET;
        if (bad) { pkt_len = 0; aad_len = 0; }
        if (bad && act && l == 0) atomicMin(kp.status, pkt);
        const bool st_ok = act && !bad;
        const unsigned char *ivp = p.ivs + (size_t)pkt * 12;
        const bool aligned = p.aligned && ((doff & 15) == 0);
        const unsigned char *aad = p.aad ? p.aad + aoff : nullptr;
        const unsigned char *in = p.in + doff;
        unsigned char *out = p.out + doff;
        const u32 n_aad = (aad_len + 15) / 16, n_ct = (pkt_len + 15) / 16, n_seq = n_aad + n_ct;
        const u32 iters = batch3_groups_max<LG>((n_seq + G - 1) / G);          // the wave runs to its longest packet; shorter ones idle FIRST (front padding)
        const u32 pad = G * iters - n_seq;

        // ---- the slot's round keys (every lane of a group loads the same lines: one broadcast per group)
        u32 rk[4 * (NR + 1)];
#pragma unroll
        for (int q = 0; q < NR + 1; q++) {
            const uint4 v = *reinterpret_cast<const uint4 *>(ks->rk + 4 * q);
            rk[4 * q] = v.x; rk[4 * q + 1] = v.y; rk[4 * q + 2] = v.z; rk[4 * q + 3] = v.w;
        }
        const u32 iv0 = load_le32(ivp), iv1 = load_le32(ivp + 4), iv2 = load_le32(ivp + 8);
        // ---- E_K(IV || 1) on lane 1 of the group, H from the slot on lane 0: both to the group's LDS slot (read back at the closing, as in k_batch3)
        {
            u32 s0 = iv0 ^ rk[0], s1 = iv1 ^ rk[1], s2 = iv2 ^ rk[2], s3 = 0x01000000u ^ rk[3];
            aes_rounds_lds<NR>(s0, s1, s2, s3, rk, smem, lb);
            const G128 e = mo_to_be(make_uint4(s0, s1, s2, s3));
            const uint4 hv = ks->hpow[0];
            if (l < 2) *reinterpret_cast<uint4 *>(smem + hsA + 16u * l) = l == 0 ? hv : make_uint4(e.w[0], e.w[1], e.w[2], e.w[3]);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        }
        {
            const uint4 sv = ks->hpow[LG];                                          // Horner stride H^(lanes per packet), stored by k_kt_setup
            G128 hs; hs.w[0] = sv.x; hs.w[1] = sv.y; hs.w[2] = sv.z; hs.w[3] = sv.w;
            shoup2_build<LG>(smem, tabA, hs, l);
        }

        // ---- one pass: CTR on the lane's blocks and Horner over its slots (k_batch3's two loops)
        G128 acc; acc.w[0] = acc.w[1] = acc.w[2] = acc.w[3] = 0;
        const CtrConsts cc = ctr_round1_consts(iv0, iv1, iv2, rk, smem, lb);
        if (p.plain) {
            const unsigned char *src = in + 16u * l;
            unsigned char *dst = out + 16u * l;
            for (u32 k = 0; k < iters; k++) {
                if (k) acc = PAIR ? batch3_mul_pair(acc, smem, tabA, tabAp, pair_first) : BATCH3_MUL(acc, smem, tabA);
                const uint4 x = gload16(src);            // (a refused packet's record lies inside the call's array: reading it is harmless, it is never written)
                u32 s0, s1, s2, s3;
                ctr_rounds_lds<NR>(bswap32(2u + k * G + l), cc, s0, s1, s2, s3, rk, smem, lb);
                const uint4 y = make_uint4(x.x ^ s0, x.y ^ s1, x.z ^ s2, x.w ^ s3);
                if (st_ok) gstore16(dst, y);
                const G128 b = mo_to_be(DEC ? x : y);
                acc.w[0] ^= b.w[0]; acc.w[1] ^= b.w[1]; acc.w[2] ^= b.w[2]; acc.w[3] ^= b.w[3];
                src += 16u * G; dst += 16u * G;
            }
        } else
        for (u32 k = 0; k < iters; k++) {
            if (k) acc = PAIR ? batch3_mul_pair(acc, smem, tabA, tabAp, pair_first) : BATCH3_MUL(acc, smem, tabA);
            const u32 v = k * G + l;
            if (v < pad) continue;
            const u32 j = v - pad;
            uint4 gin;
            if (j < n_aad) {
                const u32 off = 16 * j, rem = aad_len - off;
                gin = rem >= 16 ? gload16_any(aad + off) : load_block_bytes(aad + off, rem);
            } else {
                const u32 i = j - n_aad, off = 16 * i, rem = pkt_len - off;
                const bool full = rem >= 16;
                uint4 x;
                if (full) x = aligned ? gload16(in + off) : gload16_any(in + off);
                else x = load_block_bytes(in + off, rem < 16 ? rem : 16);
                u32 s0, s1, s2, s3;
                ctr_rounds_lds<NR>(bswap32(2u + i), cc, s0, s1, s2, s3, rk, smem, lb);
                uint4 y = make_uint4(x.x ^ s0, x.y ^ s1, x.z ^ s2, x.w ^ s3);
                if (rem < 16) y = mask_block(y, rem);
                if (act) {                                       // (a refused packet has no blocks: it never gets here)
                    if (full) { if (aligned) gstore16(out + off, y); else gstore16_any(out + off, y); }
                    else store_block_bytes(out + off, y, rem < 16 ? rem : 16);
                }
                gin = DEC ? x : y;
            }
            const G128 b = mo_to_be(gin);
            acc.w[0] ^= b.w[0]; acc.w[1] ^= b.w[1]; acc.w[2] ^= b.w[2]; acc.w[3] ^= b.w[3];
        }

        // ---- closing, as k_batch3: P = sum_l B_l H^(G-1-l);  tag = P H^2 ^ L H ^ E_K(J0)
        u32 grp2, l2;
        batch3_pos<LG>(lane_id_fresh(), grp2, l2);
        const u32 tabA2 = wave_tab + grp2 * GRP_TAB, tabB2 = ONE_TAB ? tabA2 : tabA2 + 512u, hsA2 = wave_hs + grp2 * 32u;
        const bool act2 = pk0 + grp2 < pk_end;
        const u32 pkt2 = batch_map(p, act2 ? pk0 + grp2 : pk0);
        G128 h;
        { const uint4 hv = *reinterpret_cast<const uint4 *>(smem + hsA2); h.w[0] = hv.x; h.w[1] = hv.y; h.w[2] = hv.z; h.w[3] = hv.w; }
        G128 c = gf_sqr(h);                                     // H^2
        if (ONE_TAB) __builtin_amdgcn_wave_barrier();
        shoup2_build<LG>(smem, tabB2, c, l2);
        const u32 tabAp2 = wave_tab + (grp2 ^ 3u) * GRP_TAB;
        const bool pair_first2 = (grp2 & 2u) == 0;
        acc = PAIR ? batch3_mul_pair(acc, smem, tabB2, tabAp2, pair_first2) : BATCH3_MUL(acc, smem, tabB2);
        if (l2 == G - 2u) { acc.w[1] ^= aad_len * 8u; acc.w[3] ^= pkt_len * 8u; }
        if (ONE_TAB) __builtin_amdgcn_wave_barrier();
        shoup2_build<LG>(smem, tabA2, h, l2);
#pragma unroll
        for (int j = 0; j < LG; j++) {
            if (ONE_TAB) { if (j >= 1) { if (j >= 2) c = gf_sqr(c); __builtin_amdgcn_wave_barrier(); shoup2_build<LG>(smem, tabA2, c, l2); } }
            else if (j >= 2) { c = gf_sqr(c); shoup2_build<LG>(smem, (j & 1) ? tabB2 : tabA2, c, l2); }
            const G128 t = PAIR ? batch3_mul_pair(acc, smem, tabA2, tabAp2, pair_first2) : BATCH3_MUL(acc, smem, (j & 1) ? tabB2 : tabA2);
            G128 o;
            o.w[0] = batch3_partner<LG>(t.w[0], j); o.w[1] = batch3_partner<LG>(t.w[1], j);
            o.w[2] = batch3_partner<LG>(t.w[2], j); o.w[3] = batch3_partner<LG>(t.w[3], j);
            if (l2 & (1u << j)) { acc.w[0] ^= o.w[0]; acc.w[1] ^= o.w[1]; acc.w[2] ^= o.w[2]; acc.w[3] ^= o.w[3]; }
        }
        { const uint4 ev = *reinterpret_cast<const uint4 *>(smem + hsA2 + 16u); acc.w[0] ^= ev.x; acc.w[1] ^= ev.y; acc.w[2] ^= ev.z; acc.w[3] ^= ev.w; }
        if (l2 == G - 1u && act2) {
            const uint4 tag = bad ? make_uint4(0u, 0u, 0u, 0u) : be_to_mo(acc);
            store_block_bytes(p.tags + (size_t)pkt2 * 16, tag, 16);
            if (DEC && p.auth) {
                int ok = !bad;
                if (p.expect && !bad) {
                    const uint4 e = load_block_bytes(p.expect + (size_t)pkt2 * 16, 16);
                    ok = ((e.x ^ tag.x) | (e.y ^ tag.y) | (e.z ^ tag.z) | (e.w ^ tag.w)) == 0;
                }
                p.auth[pkt2] = ok;
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ launchers
#define KT_SETUP_LDS (AESGCM_LDS_AES_OFF + AESGCM_LDS_AES)
#define ATTRCHK(call) do { const hipError_t _e = (call); if (_e != hipSuccess) return _e; } while (0)
hipError_t klaunch_kt_attributes() {
#define SETATTRKT(NR, D) ATTRCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_kt_batch<NR, D, 6>), hipFuncAttributeMaxDynamicSharedMemorySize, BATCH3_LDS_BYTES_LG(6))); \
                         ATTRCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_kt_batch<NR, D, 4>), hipFuncAttributeMaxDynamicSharedMemorySize, BATCH3_LDS_BYTES_LG(4))); \
                         ATTRCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_kt_batch<NR, D, 3>), hipFuncAttributeMaxDynamicSharedMemorySize, BATCH3_LDS_BYTES_LG(3)))
    SETATTRKT(10, 0); SETATTRKT(12, 0); SETATTRKT(14, 0); SETATTRKT(10, 1); SETATTRKT(12, 1); SETATTRKT(14, 1);
#undef SETATTRKT
    ATTRCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_kt_setup<10>), hipFuncAttributeMaxDynamicSharedMemorySize, KT_SETUP_LDS));
    ATTRCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_kt_setup<12>), hipFuncAttributeMaxDynamicSharedMemorySize, KT_SETUP_LDS));
    ATTRCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_kt_setup<14>), hipFuncAttributeMaxDynamicSharedMemorySize, KT_SETUP_LDS));
    return hipSuccess;
}
#undef ATTRCHK

hipError_t klaunch_kt_setup(int nr, hipStream_t st, const DevTables *tb, const KtSetupParams &s) {
    const unsigned wgs = (s.n + 255u) / 256u;
    if (nr == 10) hipLaunchKernelGGL(k_kt_setup<10>, dim3(wgs), dim3(256), KT_SETUP_LDS, st, tb, s);
    else if (nr == 12) hipLaunchKernelGGL(k_kt_setup<12>, dim3(wgs), dim3(256), KT_SETUP_LDS, st, tb, s);
    else hipLaunchKernelGGL(k_kt_setup<14>, dim3(wgs), dim3(256), KT_SETUP_LDS, st, tb, s);
    return hipGetLastError();
}

hipError_t klaunch_kt_batch(int nr, int dec, int lg, unsigned wgs, hipStream_t st, const DevTables *tb, const KtParams &p) {
#define LKT(NR, D, LG) hipLaunchKernelGGL((k_kt_batch<NR, D, LG>), dim3(wgs), dim3(BATCH3_LANES(NR)), BATCH3_LDS_BYTES_LG(LG), st, tb, p)
#define LKTN(D, LG) do { if (nr == 10) LKT(10, D, LG); else if (nr == 12) LKT(12, D, LG); else LKT(14, D, LG); } while (0)
    if (lg == 3) { if (dec) LKTN(1, 3); else LKTN(0, 3); }
    else if (lg == 4) { if (dec) LKTN(1, 4); else LKTN(0, 4); }
    else { if (dec) LKTN(1, 6); else LKTN(0, 6); }
#undef LKTN
#undef LKT
    return hipGetLastError();
}
