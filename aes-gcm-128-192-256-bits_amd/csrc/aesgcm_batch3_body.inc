// the body of k_batch3 (aesgcm_kernels.hip says what it computes and why its lanes are laid out so), of k_kt_batch (aesgcm_keytab_kernels.hip) and of the AEAD kernel of
// every wire family (aesgcm_<family>_kernels.hip).  Each kernel includes this file with `p` (BatchParams), `kt` (KtParams *) and three constants.  SLOTS, the key
// source: false, the packet's raw key (aes_kexp, H = E_K(0) beside E_K(J0), LG squarings of H; kt is null); true, its slot in the key table kt (round keys, H and
// H^(2^LG) as k_kt_setup stored them), and the checks that refuse a packet on its own.  WIRE (needs SLOTS): the packet is a frame in wire format, bytes
// [data_off[pkt], data_off[pkt + 1]) of p.in, laid out by `wf` (aesgcm_wire_fmt) and `wx` (KtWireXParams); p.ivs / p.tags / p.expect / p.aad_off are unused.  WIREX (needs
// WIRE): which format -- 0, AESGCM_WIREX_XPN / _ESN or one of KT_WIREX_* (aesgcm_keytab.h).  What a format decides -- its cut, its nonce, an AAD block built in
// registers, the tag's place -- is aesgcm_wirecut.h's, one function per format, called here once each; SRTP's cut and nonce alone stand here as text.
// The loop is text, not a __device__ function: as one, even force-inlined, k_batch3 compiled to another instruction stream (aesgcm_pktg_body.inc: what that cost there).
// For the same reason the two key sources read a packet's offsets in different orders: each keeps its kernel's instruction stream.  The per-format pieces are the
// measured exception: as functions the wire kernels keep their instruction counts within a handful, their VGPR counts (three instances: one more) and a block loop of the same instructions (in
// half of the instances under other register numbers), though no listing stays byte-identical; where a piece moved the loop itself it stayed text
// (profiles/wirecut/isa_compare.txt).
    static_assert(DEC == 0 || DEC == 1 || (DEC == 2 && !SLOTS), "the probe (DEC == 2) takes raw keys");
    static_assert(!WIRE || SLOTS, "frames in wire format name a slot each");
    static_assert(!WIREX || WIRE, "the number that is not on the wire belongs to a frame in wire format");
    static_assert(WIREX == 0u || WIREX == AESGCM_WIREX_XPN || WIREX == AESGCM_WIREX_ESN || WIREX == KT_WIREX_TLS13 || WIREX == KT_WIREX_TLS12 || WIREX == KT_WIREX_QUIC || WIREX == KT_WIREX_DTLS13 || WIREX == KT_WIREX_DTLS12 ||
                  WIREX == KT_WIREX_SRTP || WIREX == KT_WIREX_SRTCP || WIREX == KT_WIREX_SSH, "one extension or none");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr u32 G = 1u << LG, P = 64u >> LG;
    // LDS behind the T-tables: one (8 lanes per packet) or two 512-byte table slots per packet, 256-byte aligned (shoup2_mul_dr ORs the entry offset into
    // the slot address), then 32 bytes per packet for its H and E_K(J0)
    constexpr u32 GRP_TAB = BATCH3_GROUP_LDS_LG(LG) - 32u, WAVES = BATCH3_LANES(NR) / 64u, HSLOTS = BATCH3_LDS_TAB_OFF + WAVES * P * GRP_TAB;
    static_assert(BATCH3_LDS_TAB_OFF % 256u == 0 && GRP_TAB % 256u == 0, "k_batch3 / k_kt_batch: table slots are 256-byte aligned");
    constexpr bool ONE_TAB = LG < 4;
    constexpr bool PAIR = BATCH3_PAIR && BATCH3_PERM && BATCH3_DR && LG == 3;
    const u32 tid = threadIdx.x, lane = tid & 63u;
    main_fill_lds(smem, nullptr, tb, tid, false, BATCH3_LANES(NR));
    __syncthreads();
    const u32 lb = (lane & 31u) << 2;
    const u32 wave_id = (u32)__builtin_amdgcn_readfirstlane((int)(tid >> 6));                                          // scalar
    const u32 wave_tab = BATCH3_LDS_TAB_OFF + wave_id * P * GRP_TAB, wave_hs = HSLOTS + wave_id * P * 32u;
    constexpr u32 KEYLEN = 4 * (NR - 6);
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
        // the lane's position from a fresh lane id here and again behind the block loop (lane_id_fresh), so that none of it stays in a register across the loop
        u32 grp, l;
        batch3_pos<LG>(lane_id_fresh(), grp, l);
        const u32 tabA = wave_tab + grp * GRP_TAB, hsA = wave_hs + grp * 32u;
        const u32 tabAp = wave_tab + (grp ^ 3u) * GRP_TAB;             // PAIR: the table slot of the packet on lanes ^ 20
        const bool pair_first = (grp & 2u) == 0;                       // lane bit 4 clear
        const bool act = pk0 + grp < pk_end;                 // groups past the end shadow the first packet; their stores are masked
        const u32 pkt = batch_map(p, act ? pk0 + grp : pk0);
        // SLOTS: the packet's slot and ranges.  A packet that fails a check -- slot out of range or unset, data / AAD range falling or of 2^28 bytes or more --
        // reads nothing else (slot 0 stands in for its key material), stores only its zero tag (auth 0) and leaves its index in the table's status word
        // (atomicMin).  With raw keys nothing is checked: bad stays false.
        bool bad = false;
        const KtSlot *ks = nullptr;
        if constexpr (SLOTS) {
            const u32 slot = kt->slots[pkt];                                     // (text, not a call of aesgcm_wirecut.h's kt_slot, which says the same for the mask kernels: as
            bad = slot >= kt->n_slots;                                           // a call it changed k_kt_batch's instruction stream, which no wire format may touch)
            ks = kt->tab + (bad ? 0u : slot);
        }
        const unsigned char *ivp = p.ivs + (size_t)pkt * 12;
        u32 pkt_len = p.pkt_len, aad_len = p.aad_len;
        u64 doff = (u64)pkt * p.pkt_len, aoff = (u64)pkt * p.aad_len;
        [[maybe_unused]] u64 num = 0;                    // QUIC: the packet's full number; DTLS 1.3: the record's
        if constexpr (WIREX == KT_WIREX_SRTP) {
            // An SRTP packet (RFC 7714; RFC 3711 3.1): rtp_hdr | payload | tag[16] | mki.  Its cut and its nonce (below) are the one format that stays text here: as functions of
            // aesgcm_wirecut.h they changed the order of instructions in k_kt_srtp's block loop (profiles/wirecut/isa_compare.txt).  AAD = the header, whose length is parsed
            // from the packet: 12 bytes, 4 per CSRC (the first byte's low four bits), and with its X bit (0x10) an extension of 4 bytes and 4 times the 16-bit length in its
            // bytes 2, 3.  `tail` = what follows the payload: the tag and the MKI's wx->mki_len bytes.  Refused, in this order: the slot, the offsets, more than 65535 bytes, too
            // short for the fixed header and the tail (only then is the first byte read), a version other than 2, the header with its CSRCs does not fit, with the X bit the
            // extension's four fixed bytes do not fit (only then is its length read), the extension does not fit.  A refused packet's bytes are not read past the test that
            // refuses it, its rollover counter never
            const u64 b = p.data_off[pkt], e = p.data_off[pkt + 1];
            const u32 tail = 16u + wx->mki_len;
            bad |= ks->set != KT_SET;
            bad |= e < b || e - b > 65535u || e - b < (u64)(12u + tail);
            const u32 L = bad ? 0u : (u32)(e - b);
            const u32 b0 = bad ? 0x80u : p.in[b];
            bad |= (b0 & 0xC0u) != 0x80u;
            aoff = b;
            u32 hdr = 12u + 4u * (b0 & 15u);                                     // the fixed header and CC CSRCs
            bad |= hdr + tail > L;
            if (b0 & 0x10u) {                                                    // X: a header extension, 4 bytes and 4 * its length field
                bad |= hdr + 4u + tail > L;
                const u32 xl = bad ? 0u : ((u32)p.in[b + hdr + 2u] << 8) | p.in[b + hdr + 3u];
                hdr += 4u + 4u * xl;
                bad |= hdr + tail > L;
            }
            aad_len = bad ? 0u : hdr;
            pkt_len = bad ? 0u : L - tail - hdr;
            doff = b + (bad ? 0u : hdr);
        } else
        if constexpr (WIRE) {
            wire_cut<WIREX>(p, kt, wf, wx, ks, pkt, DEC, bad, aoff, doff, aad_len, pkt_len, num, ivp);
        } else {
        if (p.data_off) {
            if constexpr (SLOTS) { const u64 e = p.data_off[pkt + 1]; doff = p.data_off[pkt]; bad |= e < doff || e - doff >= ((u64)1 << 28); pkt_len = (u32)(e - doff); }
            else { doff = p.data_off[pkt]; pkt_len = (u32)(p.data_off[pkt + 1] - doff); }
        }
        if (p.aad_off) {
            if constexpr (SLOTS) { const u64 e = p.aad_off[pkt + 1]; aoff = p.aad_off[pkt]; bad |= e < aoff || e - aoff >= ((u64)1 << 28); aad_len = (u32)(e - aoff); }
            else { aoff = p.aad_off[pkt]; aad_len = (u32)(p.aad_off[pkt + 1] - aoff); }
        }
        }
        if constexpr (SLOTS) {
            bad |= ks->set != KT_SET;
            if (bad) { pkt_len = 0; aad_len = 0; }
            if (bad && act && l == 0) atomicMin(kt->status, pkt);
        }
        const bool st_ok = SLOTS ? act && !bad : act;       // the plain loop's stores
        const bool aligned = p.aligned && ((doff & 15) == 0);
        const unsigned char *aad = p.aad ? p.aad + aoff : nullptr;
        const unsigned char *in = p.in + doff;
        unsigned char *out = p.out + doff;
        const u32 n_aad = (aad_len + 15) / 16, n_ct = (pkt_len + 15) / 16, n_seq = n_aad + n_ct;
        const u32 iters = batch3_groups_max<LG>((n_seq + G - 1) / G);          // the wave runs to its longest packet; shorter ones idle FIRST (front padding)
        const u32 pad = G * iters - n_seq;

        // ---- the packet's round keys, the same words on every lane of its group: aes_kexp of its raw key (config/config_aes_kexp.py:128-159), or its slot's
        // (one broadcast per group)
        u32 rk[4 * (NR + 1)];
        if constexpr (SLOTS) {
#pragma unroll
            for (int q = 0; q < NR + 1; q++) {
                const uint4 v = *reinterpret_cast<const uint4 *>(ks->rk + 4 * q);
                rk[4 * q] = v.x; rk[4 * q + 1] = v.y; rk[4 * q + 2] = v.z; rk[4 * q + 3] = v.w;
            }
        } else batch_key_expand<NR>(p.keys + (size_t)pkt * KEYLEN, rk, smem, lb);
        u32 iv0, iv1, iv2;
        if constexpr (WIRE) {
            if constexpr (WIREX == KT_WIREX_SRTP) {
                // SRTP (RFC 7714 8.1): the slot's 12-byte salt XOR (00 00 | SSRC | ROC | SEQ) -- SSRC = the packet's bytes 8 .. 11, SEQ its bytes 2, 3, the rollover counter
                // hi[pkt], big-endian.  A refused packet's bytes and counter are not read
                const u32 ssrc = bad ? 0u : gload4_any(p.in + aoff + 8), sq = bad ? 0u : gload4_any(p.in + aoff) & 0xFFFF0000u, roc = bad ? 0u : bswap32(wx->hi[pkt]);
                iv0 = ks->xpn[0] ^ (ssrc << 16); iv1 = ks->xpn[1] ^ (ssrc >> 16) ^ (roc << 16); iv2 = ks->xpn[2] ^ (roc >> 16) ^ sq;
            } else
            wire_nonce<WIREX>(wf, wx, ks, ivp, p.in + aoff, in, pkt_len, num, pkt, bad, iv0, iv1, iv2);
            // out of place: the bytes in front of the payload (header; auth-only: all but the ICV) pass through
            if constexpr (wire_copies_front(WIREX))
            if (p.in != p.out && st_ok) wire_copy_front(p.out + aoff, p.in + aoff, (u32)(doff - aoff), l, G);
        } else { iv0 = load_le32(ivp); iv1 = load_le32(ivp + 4); iv2 = load_le32(ivp + 8); }
        // ---- H on lane 0 and E_K(IV || 1) on lane 1 of the group: with a raw key H = E_K(0^128) in the same pass (gcm_gctr.vhd:141-145), with a slot its stored H
        // Both go to the group's LDS slot (32 bytes behind its tables) and are read back where they are needed: H now and at the closing, E_K(J0) at the very
        // end -- held in registers across the block loop they were part of what the 128-register build spilled.
        {
            const bool h_lane = !SLOTS && l == 0;
            u32 s0 = (h_lane ? 0u : iv0) ^ rk[0], s1 = (h_lane ? 0u : iv1) ^ rk[1], s2 = (h_lane ? 0u : iv2) ^ rk[2];
            u32 s3 = (h_lane ? 0u : 0x01000000u) ^ rk[3];
            aes_rounds_lds<NR>(s0, s1, s2, s3, rk, smem, lb);
            const G128 e = mo_to_be(make_uint4(s0, s1, s2, s3));
            const uint4 hv = SLOTS ? ks->hpow[0] : make_uint4(0u, 0u, 0u, 0u);
            if (l < 2) *reinterpret_cast<uint4 *>(smem + hsA + 16u * l) = SLOTS && l == 0 ? hv : make_uint4(e.w[0], e.w[1], e.w[2], e.w[3]);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        }
        {
            G128 hs;                                                                   // the Horner stride H^(lanes per packet)
            if constexpr (SLOTS) {
                const uint4 sv = ks->hpow[LG];                                         // stored by k_kt_setup
                hs.w[0] = sv.x; hs.w[1] = sv.y; hs.w[2] = sv.z; hs.w[3] = sv.w;
            } else {
                const uint4 hv = *reinterpret_cast<const uint4 *>(smem + hsA);
                G128 h; h.w[0] = hv.x; h.w[1] = hv.y; h.w[2] = hv.z; h.w[3] = hv.w;
                hs = gf_sqr(gf_sqr(gf_sqr(h)));                                        // LG squarings (linear: gf_sqr, no table)
#pragma unroll
                for (int j = 3; j < LG; j++) hs = gf_sqr(hs);
            }
            shoup2_build<LG>(smem, tabA, hs, l);
        }

        // ---- one pass: CTR on the lane's blocks and Horner over its slots
        G128 acc; acc.w[0] = acc.w[1] = acc.w[2] = acc.w[3] = 0;
        const CtrConsts cc = ctr_round1_consts(iv0, iv1, iv2, rk, smem, lb);
        // Records of one size that is a whole number of wave-iterations, no AAD, aligned (cfg5's shape): no padding slot, no AAD slot, no ragged block -- the
        // same work without the per-iteration tests and masks of the general loop below (launch-uniform: BatchParams::plain; never frames, whose lengths are on the
        // device -- k_kt_wirex is built without it)
        if (!WIREX && p.plain) {
            const unsigned char *src = in + 16u * l;
            unsigned char *dst = out + 16u * l;
            for (u32 k = 0; k < iters; k++) {
                if (k) acc = PAIR ? batch3_mul_pair(acc, smem, tabA, tabAp, pair_first) : BATCH3_MUL(acc, smem, tabA);
                const uint4 x = DEC == 2 ? make_uint4(l, k, pkt, 0u) : gload16(src);     // (DEC == 2, the PROBE: the same instruction stream without the data's HBM traffic)
                u32 s0, s1, s2, s3;                                                     // (a refused packet's record lies inside the call's array: it is read, never written)
                ctr_rounds_lds<NR>(bswap32(2u + k * G + l), cc, s0, s1, s2, s3, rk, smem, lb);
                const uint4 y = make_uint4(x.x ^ s0, x.y ^ s1, x.z ^ s2, x.w ^ s3);
                if (st_ok && DEC != 2) gstore16(dst, y);
                const G128 b = mo_to_be(DEC == 1 ? x : y);           // aes_gcm.vhd:207-211
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
                if constexpr (wire_aad_built(WIREX)) {
                    // A number that is not in the frame (ESN's hi, TLS 1.2's seq) is fetched here, once per frame on one lane, from a frame number worked out afresh: loaded
                    // in front of the loop it would be one more register across it.  (A refused frame has no AAD block.)
                    u32 xpkt = 0;
                    if constexpr (wire_aad_num(WIREX)) {
                        u32 xg, xl;
                        batch3_pos<LG>(lane_id_fresh(), xg, xl);
                        xpkt = batch_map(p, pk0 + xg < pk_end ? pk0 + xg : pk0);
                    }
                    gin = wire_aad_block<WIREX>(wx, aad, in, aad_len, pkt_len, off, xpkt);
                } else
                gin = rem >= 16 ? gload16_any(aad + off) : load_block_bytes(aad + off, rem);
            } else {
                const u32 i = j - n_aad, off = 16 * i, rem = pkt_len - off;
                const bool full = rem >= 16;                    // a whole block is one access at any address
                uint4 x;
                if (DEC == 2) x = make_uint4(l, i, pkt, 0u);
                else if (full) x = aligned ? gload16(in + off) : gload16_any(in + off);
                else x = load_block_bytes(in + off, rem < 16 ? rem : 16);
                u32 s0, s1, s2, s3;
                ctr_rounds_lds<NR>(bswap32(2u + i), cc, s0, s1, s2, s3, rk, smem, lb);
                uint4 y = make_uint4(x.x ^ s0, x.y ^ s1, x.z ^ s2, x.w ^ s3);
                if (rem < 16) y = mask_block(y, rem);
                if (act && DEC != 2) {                          // (a refused packet has no blocks: it never gets here)
                    if (full) { if (aligned) gstore16(out + off, y); else gstore16_any(out + off, y); }
                    else store_block_bytes(out + off, y, rem < 16 ? rem : 16);
                }
                gin = DEC == 1 ? x : y;                          // aes_gcm.vhd:207-211
            }
            const G128 b = mo_to_be(gin);
            acc.w[0] ^= b.w[0]; acc.w[1] ^= b.w[1]; acc.w[2] ^= b.w[2]; acc.w[3] ^= b.w[3];
        }

        // ---- closing: P = sum_l B_l H^(G-1-l);  tag = P H^2 ^ L H ^ E_K(J0)  (gcm_ghash.vhd:257,293), as in k_pktg
        u32 grp2, l2;
        batch3_pos<LG>(lane_id_fresh(), grp2, l2);
        const u32 tabA2 = wave_tab + grp2 * GRP_TAB, tabB2 = ONE_TAB ? tabA2 : tabA2 + 512u, hsA2 = wave_hs + grp2 * 32u;
        const bool act2 = pk0 + grp2 < pk_end;
        const u32 pkt2 = batch_map(p, act2 ? pk0 + grp2 : pk0);
        G128 h;
        { const uint4 hv = *reinterpret_cast<const uint4 *>(smem + hsA2); h.w[0] = hv.x; h.w[1] = hv.y; h.w[2] = hv.z; h.w[3] = hv.w; }
        G128 c = gf_sqr(h);                                     // H^2
        if (ONE_TAB) __builtin_amdgcn_wave_barrier();           // every lane is done with the Horner table
        shoup2_build<LG>(smem, tabB2, c, l2);
        const u32 tabAp2 = wave_tab + (grp2 ^ 3u) * GRP_TAB;
        const bool pair_first2 = (grp2 & 2u) == 0;
        acc = PAIR ? batch3_mul_pair(acc, smem, tabB2, tabAp2, pair_first2) : BATCH3_MUL(acc, smem, tabB2);
        if (l2 == G - 2u) { acc.w[1] ^= aad_len * 8u; acc.w[3] ^= pkt_len * 8u; }     // the length block: both < 2^32 bits by the ABI's limits
        if (ONE_TAB) __builtin_amdgcn_wave_barrier();
        shoup2_build<LG>(smem, tabA2, h, l2);                   // the Horner table is no longer needed
#pragma unroll
        for (int j = 0; j < LG; j++) {
            // level j: constant H^(2^j); two slots: H in tabA, H^2 in tabB, then H^4 -> tabA, H^8 -> tabB; one slot: each level rebuilds it (c = H^2 is still at hand for level 1)
            if (ONE_TAB) { if (j >= 1) { if (j >= 2) c = gf_sqr(c); __builtin_amdgcn_wave_barrier(); shoup2_build<LG>(smem, tabA2, c, l2); } }
            else if (j >= 2) { c = gf_sqr(c); shoup2_build<LG>(smem, (j & 1) ? tabB2 : tabA2, c, l2); }
            const G128 t = PAIR ? batch3_mul_pair(acc, smem, tabA2, tabAp2, pair_first2) : BATCH3_MUL(acc, smem, (j & 1) ? tabB2 : tabA2);
            G128 o;
            o.w[0] = batch3_partner<LG>(t.w[0], j); o.w[1] = batch3_partner<LG>(t.w[1], j);
            o.w[2] = batch3_partner<LG>(t.w[2], j); o.w[3] = batch3_partner<LG>(t.w[3], j);
            if (l2 & (1u << j)) { acc.w[0] ^= o.w[0]; acc.w[1] ^= o.w[1]; acc.w[2] ^= o.w[2]; acc.w[3] ^= o.w[3]; }
        }
        { const uint4 ev = *reinterpret_cast<const uint4 *>(smem + hsA2 + 16u); acc.w[0] ^= ev.x; acc.w[1] ^= ev.y; acc.w[2] ^= ev.z; acc.w[3] ^= ev.w; }
        if constexpr (WIRE) {
            // the ICV = the tag's first tag_len bytes, where wire_tag_place says: written (encrypt) or compared (decrypt; copied when out of place) with stores that end at
            // the ICV's end.  A refused frame: nothing but auth 0.
            if (l2 == G - 1u && act2) {
                int ok = 0;
                if (!bad) {
                    const u32 tl = wf->tag_len;
                    const u64 at = wire_tag_place<WIREX>(p, wf, wx, pkt2);
                    const uint4 tag = be_to_mo(acc);                       // (tl is 8, 12 or 16: whole words)
                    if (DEC == 1) {
                        const uint4 e = wire_load_icv(p.in + at, tl);
                        ok = ((e.x ^ tag.x) | (e.y ^ tag.y) | (tl > 8u ? e.z ^ tag.z : 0u) | (tl > 12u ? e.w ^ tag.w : 0u)) == 0;
                        if (p.in != p.out) wire_store_icv(p.out + at, e, tl);
                    } else wire_store_icv(p.out + at, tag, tl);
                }
                if (DEC == 1) p.auth[pkt2] = ok;
            }
        } else
        if (l2 == G - 1u && act2) {
            const uint4 tag = bad ? make_uint4(0u, 0u, 0u, 0u) : be_to_mo(acc);
            store_block_bytes(p.tags + (size_t)pkt2 * 16, tag, 16);
            if (DEC == 1 && p.auth) {
                int ok = !bad;
                if (p.expect && !bad) {
                    const uint4 e = load_block_bytes(p.expect + (size_t)pkt2 * 16, 16);
                    ok = ((e.x ^ tag.x) | (e.y ^ tag.y) | (e.z ^ tag.z) | (e.w ^ tag.w)) == 0;
                }
                p.auth[pkt2] = ok;
            }
        }
    }
