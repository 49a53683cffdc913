// aesgcm_mask.h -- what the two mask kernels share, a lane per packet each: k_kt_quic_hp (aesgcm_quic_kernels.hip: QUIC header protection, RFC 9001 5.4) and k_kt_dtls_sn
// (aesgcm_dtls_kernels.hip: DTLS 1.3 record-number encryption, RFC 9147 4.2.3).  Both protocols mask a truncated number in the header with AES-ECB of a 16-byte ciphertext
// sample under a second key, and both decode the full number from the truncated one and an expected one.  Here: a packet of the pass if the AEAD kernel takes it too
// (mask_take: the front tests of aesgcm_wirecut.h, the very function the AEAD's cut calls), the mask from a sample under the mask slot's round keys (mask_of_sample), and
// the decode (wire_decode_num).  Where the sample lies and which bytes the mask covers are the protocol's, and stay in its kernel.
#pragma once
#include "aesgcm_keytab.h"
#include "aesgcm_lanes.h"
#include "aesgcm_wirecut.h"

// RFC 9000 A.3 (DecodePacketNumber) on unsigned 64-bit values: the candidate closest to `expected` among those whose low nbits bits are `truncated`, a tie going upwards.
// The RFC's integers are unbounded, so each comparison is written so that it cannot wrap.  `last` is the largest number there is (QUIC: 2^62 - 1, the RFC's
// `candidate_pn < (1 << 62) - pn_win`; DTLS: 2^64 - 1): no candidate beyond it is chosen.  So at expected = 0 nothing is looked for below zero (the result is `truncated`),
// and at expected = last nothing above it (the result lies in the last window: (last & ~(2^nbits - 1)) | truncated).
HD u64 wire_decode_num(u64 expected, u32 truncated, u32 nbits, u64 last) {
    const u64 win = (u64)1 << nbits, hwin = win >> 1, mask = win - 1;
    const u64 cand = (expected & ~mask) | truncated;
    if (expected >= hwin && cand <= expected - hwin && cand <= last - win) return cand + win;
    if (expected <= ~(u64)0 - hwin && cand > expected + hwin && cand >= win) return cand - win;
    return cand;
}

// Packet i of a mask pass, if it passes wire_front with `tail` bytes from the number field's start to the packet's end.  -> false: refused, and nothing of the packet
// is read or written.
struct MaskPkt {
    const unsigned char *src;              // the packet in q.in
    unsigned char *dst;                    // ... and in q.out
    const KtSlot *ms;                      // the mask key's slot
    u32 po, len;                           // where the number field starts; the packet's length
};
HD bool mask_take(const KtQuicHpParams &q, u32 i, u32 tail, MaskPkt &m) {
    const u64 b = q.pkt_off[i], e = q.pkt_off[i + 1];
    const u32 po = q.pn_off[i];
    bool bad;
    const KtSlot *const ks = kt_slot(q.tab, q.n_slots, q.slots[i], bad);
    m.ms = wire_front(q.tab, q.n_slots, ks, q.hp_slots[i], po, b, e, tail, bad);
    if (bad) return false;
    m.src = q.in + b; m.dst = q.out + b; m.po = po; m.len = (u32)(e - b);
    return true;
}

// mask = AES-ECB(the slot's key, the 16 bytes at `sample`), as memory-order words: mask[0 .. 3] = the bytes of s0 from the lowest, mask[4] = the lowest of s1.
// smem holds T0 | T2 (main_fill_lds); lb = (lane & 31) << 2
template <int NR>
HD void mask_of_sample(const KtSlot *ms, const unsigned char *sample, const unsigned char *smem, u32 lb, u32 &s0, u32 &s1, u32 &s2, u32 &s3) {
    u32 rk[4 * (NR + 1)];
#pragma unroll
    for (int r = 0; r < NR + 1; r++) {
        const uint4 v = *reinterpret_cast<const uint4 *>(ms->rk + 4 * r);
        rk[4 * r] = v.x; rk[4 * r + 1] = v.y; rk[4 * r + 2] = v.z; rk[4 * r + 3] = v.w;
    }
    const uint4 x = gload16_any(sample);
    s0 = x.x ^ rk[0]; s1 = x.y ^ rk[1]; s2 = x.z ^ rk[2]; s3 = x.w ^ rk[3];
    aes_rounds_lds<NR>(s0, s1, s2, s3, rk, smem, lb);
}
