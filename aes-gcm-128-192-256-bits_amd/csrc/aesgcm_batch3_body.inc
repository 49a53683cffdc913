// the body of k_batch3 (aesgcm_kernels.hip says what it computes and why its lanes are laid out so) and of k_kt_batch (aesgcm_keytab_kernels.hip).  Each kernel
// includes this file with `p` (BatchParams), `kt` (KtParams *) and the key source SLOTS, a constant: false, the packet's raw key (aes_kexp, H = E_K(0) beside
// E_K(J0), LG squarings of H; kt is null); true, its slot in the key table kt (round keys, H and H^(2^LG) as k_kt_setup stored them), and the checks that refuse
// a packet on its own.  WIRE (k_kt_wire, aesgcm_wire_kernels.hip; needs SLOTS): the packet is a FRAME in wire format, bytes [data_off[pkt], data_off[pkt + 1]) of
// p.in = header | payload | ICV as `wf` (aesgcm_wire_fmt) lays it out -- AAD range, payload range, nonce (the slot's salt, then header bytes) and the ICV's place all come
// from that one offset; p.aad is p.in, p.ivs / p.tags / p.expect / p.aad_off are unused.  WIREX (k_kt_wirex, aesgcm_wirex_kernels.hip; needs WIRE): `wx` (KtWireXParams) adds
// a 32-bit number per frame that is not on the wire, the upper half of its packet or sequence number; WIREX itself says whether it enters the nonce (AESGCM_WIREX_XPN,
// MACsec XPN) or the AAD (AESGCM_WIREX_ESN, ESP with extended sequence numbers), and is 0 in every other kernel.  KT_WIREX_TLS13 / KT_WIREX_TLS12 (k_kt_tls,
// aesgcm_tls_kernels.hip; internal values, aesgcm_keytab.h): the frame is a TLS record hdr[5] | (1.2: explicit nonce[8]) | payload | tag[16] and the number is its whole 64-bit
// sequence number, wx->seq[pkt]: 1.3 XORs it into the slot's 12-byte IV (KtSlot::xpn) and reads no nonce byte from the record, 1.2 puts it in front of the one AAD block.
// KT_WIREX_QUIC (k_kt_quic, aesgcm_quic_kernels.hip): the frame is a QUIC packet header | payload | tag[16] whose header ends behind its packet-number field, at
// wx->pn_off[pkt] + (first byte & 3) + 1 -- per packet, the first byte read through p.aad, where the header lies unprotected; nonce as TLS 1.3's from wx->seq[pkt], the full
// packet number.  The header itself is k_kt_quic_hp's business: it is not copied here.  KT_WIREX_DTLS13 / KT_WIREX_DTLS12 (k_kt_dtls, aesgcm_dtls_kernels.hip): the frame is a
// DTLS record.  1.3 (RFC 9147): unified_hdr | payload | tag[16], QUIC's structure -- the header ends behind the sequence-number field that starts at wx->pn_off[pkt], 1 or 2
// bytes by the first byte's S bit, and behind the 2 length bytes that its L bit announces; the first byte, which is never masked, is read through p.in; nonce as TLS 1.3's
// from wx->seq[pkt]; the header is k_kt_dtls_sn's business.  1.2 (RFC 6347): hdr[13] | explicit nonce[8] | payload | tag[16], TLS 1.2's structure with epoch and sequence
// number read from the record's bytes 3 .. 10 where TLS 1.2 takes wx->seq[pkt]; no number comes from outside the record.  KT_WIREX_SRTP / KT_WIREX_SRTCP (k_kt_srtp,
// aesgcm_srtp_kernels.hip; RFC 7714): the frame is an SRTP packet rtp_hdr | payload | tag[16] | mki or an SRTCP packet rtcp_hdr[8] | payload | tag[16] | W[4] | mki, the MKI
// wx->mki_len bytes.  The RTP header's length is parsed from the packet (CSRC count, X bit, the extension's length field); nonce = the slot's 12-byte salt (KtSlot::xpn) XOR
// SSRC, the rollover counter wx->hi[pkt] and the sequence number (SRTP) or SSRC and W's 31-bit index (SRTCP).  The tag is not the packet's last bytes, and SRTCP's AAD is in
// two pieces: the packet's front and W, the word behind the tag -- with W's E bit clear nothing is encrypted and everything in front of the tag is AAD.  Text, not a __device__ function: as one, even force-inlined, k_batch3 compiled to another instruction stream (aesgcm_pktg_body.inc:
// what that cost there).  For the same reason the two key sources read a packet's offsets in different orders: each keeps its kernel's instruction stream.
    static_assert(DEC == 0 || DEC == 1 || (DEC == 2 && !SLOTS), "the probe (DEC == 2) takes raw keys");
    static_assert(!WIRE || SLOTS, "frames in wire format name a slot each");
    static_assert(!WIREX || WIRE, "the number that is not on the wire belongs to a frame in wire format");
    static_assert(WIREX == 0u || WIREX == AESGCM_WIREX_XPN || WIREX == AESGCM_WIREX_ESN || WIREX == KT_WIREX_TLS13 || WIREX == KT_WIREX_TLS12 || WIREX == KT_WIREX_QUIC || WIREX == KT_WIREX_DTLS13 || WIREX == KT_WIREX_DTLS12 ||
                  WIREX == KT_WIREX_SRTP || WIREX == KT_WIREX_SRTCP, "one extension or none");
    constexpr bool x_xpn = WIREX == AESGCM_WIREX_XPN, x_esn = WIREX == AESGCM_WIREX_ESN, x_t13 = WIREX == KT_WIREX_TLS13, x_t12 = WIREX == KT_WIREX_TLS12, x_quic = WIREX == KT_WIREX_QUIC;
    constexpr bool x_d13 = WIREX == KT_WIREX_DTLS13, x_d12 = WIREX == KT_WIREX_DTLS12;
    constexpr bool x_srtp = WIREX == KT_WIREX_SRTP, x_rtcp = WIREX == KT_WIREX_SRTCP;
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
            const u32 slot = kt->slots[pkt];
            bad = slot >= kt->n_slots;
            ks = kt->tab + (bad ? 0u : slot);
        }
        const unsigned char *ivp = p.ivs + (size_t)pkt * 12;
        u32 pkt_len = p.pkt_len, aad_len = p.aad_len;
        u64 doff = (u64)pkt * p.pkt_len, aoff = (u64)pkt * p.aad_len;
        [[maybe_unused]] u64 qpn = 0;                    // QUIC: the packet's full number; DTLS 1.3: the record's
        if constexpr (x_quic) {
            // a QUIC packet (RFC 9001 5.3): AAD = the header up to and including the packet-number field, whose length is in the unprotected first byte; payload behind
            // it; the tag last.  Refused: what k_kt_quic_hp refuses (aesgcm_mask.h: mask_take, and the number's range) -- either slot, the offsets, more than 65535 bytes, pn_off 0,
            // the sample's 16 bytes at pn_off + 4 not inside the packet (so header and tag fit for every pn_len), and on encrypt a number of 2^62 or more.  A refused
            // packet's number and first byte are not read
            const u64 b = p.data_off[pkt], e = p.data_off[pkt + 1];
            const u32 hslot = wx->hp_slots[pkt], po = wx->pn_off[pkt];
            bad |= hslot >= kt->n_slots || e < b || e - b > 65535u || po == 0u || (u64)po + 20u > e - b;
            bad |= ks->set != KT_SET || kt->tab[bad ? 0u : hslot].set != KT_SET;
            qpn = bad ? (u64)0 : wx->seq[pkt];
            if (DEC == 0) bad |= (qpn >> 62) != 0;
            const u32 hdr = bad ? 0u : po + (p.aad[b] & 3u) + 1u;
            aoff = b;
            aad_len = hdr;
            pkt_len = bad ? 0u : (u32)(e - b) - 16u - hdr;
            doff = b + hdr;
        } else
        if constexpr (x_d13) {
            // a DTLS 1.3 record (RFC 9147 4): AAD = the unified header with the sequence-number bytes unprotected, read through p.aad; payload behind it; the tag last.
            // Refused: what k_kt_dtls_sn refuses, by the same tests in the same order -- either slot, the offsets, more than 65535 bytes, pn_off 0, fewer than 17 bytes
            // from the sequence-number field to the record's end (one sequence byte and the sample; only then is the first byte read, through p.in: it is never masked
            // and k_kt_dtls_sn writes nothing of a record it refuses), a first byte that is not 001xxxxx, the sample's 16 bytes at the header's end not inside the record
            // (so header and tag fit).  A refused record's number is not read
            const u64 b = p.data_off[pkt], e = p.data_off[pkt + 1];
            const u32 hslot = wx->hp_slots[pkt], po = wx->pn_off[pkt];
            bad |= hslot >= kt->n_slots || e < b || e - b > 65535u || po == 0u || (u64)po + 17u > e - b;
            bad |= ks->set != KT_SET || kt->tab[bad ? 0u : hslot].set != KT_SET;
            const u32 b0 = bad ? 0u : p.in[b];
            const u32 hdr = bad ? 0u : po + (b0 & 0x08u ? 2u : 1u) + (b0 & 0x04u ? 2u : 0u);
            bad |= (b0 & 0xE0u) != 0x20u || (u64)hdr + 16u > e - b;
            qpn = bad ? (u64)0 : wx->seq[pkt];
            aoff = b;
            aad_len = bad ? 0u : hdr;
            pkt_len = bad ? 0u : (u32)(e - b) - 16u - hdr;
            doff = b + (bad ? 0u : hdr);
        } else
        if constexpr (x_srtp || x_rtcp) {
            // an SRTP / SRTCP packet (RFC 7714; RFC 3711 3.1, 3.4).  `tail` = what follows the payload: the tag, SRTCP's word W, the MKI.  Refused, in this order: the slot,
            // the offsets, more than 65535 bytes, too short for the fixed header and the tail (only then is the first byte read), a version other than 2; RTP: the header
            // with its CSRCs does not fit, with the X bit the extension's four fixed bytes do not fit (only then is its length read), the extension does not fit.  A refused
            // packet's bytes are not read past the test that refuses it, its rollover counter never
            const u64 b = p.data_off[pkt], e = p.data_off[pkt + 1];
            const u32 tail = 16u + wx->mki_len + (x_rtcp ? 4u : 0u);
            bad |= ks->set != KT_SET;
            bad |= e < b || e - b > 65535u || e - b < (u64)((x_rtcp ? 8u : 12u) + tail);
            const u32 L = bad ? 0u : (u32)(e - b);
            const u32 b0 = bad ? 0x80u : p.in[b];
            bad |= (b0 & 0xC0u) != 0x80u;
            aoff = b;
            if constexpr (x_srtp) {
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
            } else {
                // SRTCP: W = E | index lies behind the tag.  E set: AAD = the 8 header bytes | W, payload behind the header.  E clear: nothing is encrypted, AAD = everything
                // in front of the tag | W, and all of it passes through (doff = where the tag starts, as an auth-only frame's)
                const u32 body = bad ? 0u : L - tail;                                // the bytes in front of the tag: 8 or more
                const bool enc = !bad && (p.in[b + body + 16u] & 0x80u) != 0;
                aad_len = bad ? 0u : enc ? 12u : body + 4u;
                pkt_len = enc ? body - 8u : 0u;
                doff = b + (enc ? 8u : body);
            }
        } else
        if constexpr (WIRE) {
            // the frame's one range: AAD from its first byte, payload behind the header, the ICV last; auth-only: everything in front of the ICV is AAD.  A frame too
            // short for header (nonce bytes included) and ICV is refused like a falling range
            const u64 b = p.data_off[pkt], e = p.data_off[pkt + 1];
            const bool auth_only = !x_esn && (wf->flags & AESGCM_WIRE_AUTH_ONLY) != 0;                   // (ESN: never -- aesgcm_wire_xfmt_check)
            const u32 nonce_end = wf->iv_off + 12u - wf->salt_len, front = auth_only && nonce_end > wf->hdr_len ? nonce_end : wf->hdr_len;
            bad |= e < b || e - b >= ((u64)1 << 28) || e - b < (u64)(front + wf->tag_len);
            if constexpr (x_t13 || x_t12) bad |= e - b > 5u + 65535u;                // a TLS record's length field says what follows its five header bytes
            if constexpr (x_d12) bad |= e - b > 13u + 65535u;                        // ... and a DTLS 1.2 record's what follows its thirteen
            const u32 body = bad ? 0u : (u32)(e - b) - wf->tag_len;                  // the bytes in front of the ICV
            aoff = b;
            aad_len = auth_only ? body : wf->aad_len;
            pkt_len = auth_only ? 0u : body - wf->hdr_len;
            doff = b + (auth_only ? body : wf->hdr_len);
            if constexpr (x_esn) aad_len = 12u;                                      // SPI | seq-hi | seq-lo (RFC 4303): the frame's first 8 bytes around hi[pkt]
            if constexpr (x_t12) aad_len = 13u;                                      // seq | type, version | payload length (RFC 5246 6.2.3.3): seq[pkt], three header bytes, pkt_len
            if constexpr (x_d12) aad_len = 13u;                                      // epoch, seq | type, version | payload length (RFC 6347 4.1.2.1): eleven header bytes, pkt_len
            ivp = p.in + b + wf->iv_off;
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
            // the nonce: salt_len (0, 4 or 8) bytes of the slot's salt, then header bytes -- whole words either way; a refused frame's header is not read
            const u32 sw = x_xpn ? 2u : x_t13 || x_quic || x_d13 || x_srtp || x_rtcp ? 3u : x_t12 || x_d12 ? 1u : wf->salt_len >> 2;                    // (XPN: salt_len is 8 -- aesgcm_wire_xfmt_check; TLS 1.3: no frame bytes)
            const u32 f0 = bad || x_t13 || x_quic || x_d13 || x_srtp || x_rtcp ? 0u : gload4_any(ivp), f1 = bad || sw > 1u ? 0u : gload4_any(ivp + 4), f2 = bad || sw > 0u ? 0u : gload4_any(ivp + 8);
            iv0 = sw ? ks->salt[0] : f0;
            iv1 = sw > 1u ? ks->salt[1] : sw ? f0 : f1;
            iv2 = sw > 1u ? f0 : sw ? f1 : f2;
            if constexpr (x_xpn) {
                // XPN (802.1AEbw): the slot's 12-byte salt XOR (SSCI | PN), big-endian: hi[pkt], then the four frame bytes at iv_off (f0: salt_len is 8).  The classic salt is
                // not used; a refused frame's hi is not read
                iv0 = ks->xpn[0] ^ ks->xpn[3]; iv1 = ks->xpn[1] ^ (bad ? 0u : bswap32(wx->hi[pkt])); iv2 = ks->xpn[2] ^ f0;
            }
            if constexpr (x_t12 || x_d12) iv0 = ks->xpn[0];           // TLS 1.2 (RFC 5288), and DTLS 1.2 the same: the slot IV's first four bytes (aesgcm_keytab_set_tls_iv), then the record's explicit eight (f0, f1)
            if constexpr (x_t13) {
                // TLS 1.3 (RFC 8446 5.3): the slot's 12-byte IV XOR the sequence number, big-endian, right-aligned.  A refused record's number is not read
                const u64 sq = bad ? (u64)0 : wx->seq[pkt];
                iv0 = ks->xpn[0]; iv1 = ks->xpn[1] ^ bswap32((u32)(sq >> 32)); iv2 = ks->xpn[2] ^ bswap32((u32)sq);
            }
            if constexpr (x_quic || x_d13) {
                // QUIC (RFC 9001 5.3): TLS 1.3's formula with the packet number; DTLS 1.3 (RFC 9147 4.2.1 -> RFC 8446 5.3): with the record's sequence number
                iv0 = ks->xpn[0]; iv1 = ks->xpn[1] ^ bswap32((u32)(qpn >> 32)); iv2 = ks->xpn[2] ^ bswap32((u32)qpn);
            }
            if constexpr (x_srtp) {
                // SRTP (RFC 7714 8.1): the slot's 12-byte salt XOR (00 00 | SSRC | ROC | SEQ) -- SSRC = the packet's bytes 8 .. 11, SEQ its bytes 2, 3, the rollover counter
                // hi[pkt], big-endian.  A refused packet's bytes and counter are not read
                const u32 ssrc = bad ? 0u : gload4_any(p.in + aoff + 8), sq = bad ? 0u : gload4_any(p.in + aoff) & 0xFFFF0000u, roc = bad ? 0u : bswap32(wx->hi[pkt]);
                iv0 = ks->xpn[0] ^ (ssrc << 16); iv1 = ks->xpn[1] ^ (ssrc >> 16) ^ (roc << 16); iv2 = ks->xpn[2] ^ (roc >> 16) ^ sq;
            }
            if constexpr (x_rtcp) {
                // SRTCP (RFC 7714 9.1): the salt XOR (00 00 | SSRC | 00 00 | 0, the 31-bit index) -- SSRC = the packet's bytes 4 .. 7, the index = W without its E bit (the
                // top bit of W's first byte).  W lies 16 bytes behind the payload, or behind the AAD's packet bytes when there is none
                const u32 ssrc = bad ? 0u : gload4_any(p.in + aoff + 4), w = bad ? 0u : gload4_any(in + pkt_len + 16u) & 0xFFFFFF7Fu;
                iv0 = ks->xpn[0] ^ (ssrc << 16); iv1 = ks->xpn[1] ^ (ssrc >> 16); iv2 = ks->xpn[2] ^ w;
            }
            // out of place: the bytes in front of the payload (header; auth-only: all but the ICV) pass through (QUIC: k_kt_quic_hp writes the header; DTLS 1.3: k_kt_dtls_sn)
            if constexpr (!x_quic && !x_d13)
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
                if constexpr (x_esn) {
                    // the one AAD block, built around the number that is not in the frame.  It is fetched here, once per frame on one lane, from a frame number worked out
                    // afresh: loaded in front of the loop it would be one more register across it.  (A refused frame has no AAD block.)
                    u32 xg, xl;
                    batch3_pos<LG>(lane_id_fresh(), xg, xl);
                    const u32 xpkt = batch_map(p, pk0 + xg < pk_end ? pk0 + xg : pk0);
                    gin = make_uint4(gload4_any(aad), bswap32(wx->hi[xpkt]), gload4_any(aad + 4), 0u);
                } else if constexpr (x_t12) {
                    // TLS 1.2's one AAD block, built the same way: be64(seq) | type, version (the record's first three bytes) | be16(payload length), the length from the
                    // offsets (pkt_len < 2^16: the check above), not from the header's own two bytes
                    u32 xg, xl;
                    batch3_pos<LG>(lane_id_fresh(), xg, xl);
                    const u32 xpkt = batch_map(p, pk0 + xg < pk_end ? pk0 + xg : pk0);
                    const u64 sq = wx->seq[xpkt];
                    gin = make_uint4(bswap32((u32)(sq >> 32)), bswap32((u32)sq), (gload4_any(aad) & 0x00FFFFFFu) | ((pkt_len >> 8) << 24), pkt_len & 0xFFu);
                } else if constexpr (x_d12) {
                    // DTLS 1.2's one AAD block: epoch | sequence number as the record's bytes 3 .. 10 carry them, then as TLS 1.2's -- type, version | be16(payload length),
                    // the length from the offsets (pkt_len < 2^16: the check above)
                    gin = make_uint4(gload4_any(aad + 3), gload4_any(aad + 7), (gload4_any(aad) & 0x00FFFFFFu) | ((pkt_len >> 8) << 24), pkt_len & 0xFFu);
                } else if constexpr (x_rtcp) {
                    // SRTCP's AAD is in two pieces: packet bytes, then W from behind the tag (in + pkt_len + 16: see the nonce), fetched here by the lane that needs it.
                    // 12 bytes (E set; E clear and a bare header): the one block header | W.  Longer (E clear): aad_len - 4 packet bytes; a block that lies inside them is a
                    // plain load, the others take what is left of the packet bytes and as much of W as fits -- W may split over the last two blocks
                    const u32 body = aad_len - 4u;
                    if (aad_len == 12u) gin = make_uint4(gload4_any(aad), gload4_any(aad + 4), gload4_any(in + pkt_len + 16u), 0u);
                    else if (off + 16u <= body) gin = gload16_any(aad + off);
                    else gin = load_block_split(aad + off, off < body ? body - off : 0u, in + pkt_len + 16u, off > body ? off - body : 0u);
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
            // the ICV = the tag's first tag_len bytes, the frame's last (SRTP / SRTCP: in front of the trail): written (encrypt) or compared (decrypt; copied when out of place) with stores that end at the
            // frame's end.  A refused frame: nothing but auth 0.
            if (l2 == G - 1u && act2) {
                int ok = 0;
                if (!bad) {
                    const u32 tl = wf->tag_len;
                    u64 at = p.data_off[pkt2 + 1] - tl;
                    if constexpr (x_srtp || x_rtcp) {
                        // the tag is not last: SRTCP's W and the MKI follow it, and pass through out of place, copied by this lane
                        const u32 trail = wx->mki_len + (x_rtcp ? 4u : 0u);
                        at -= trail;
                        if (p.in != p.out) wire_copy_front(p.out + at + tl, p.in + at + tl, trail, 0u, 1u);
                    }
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
