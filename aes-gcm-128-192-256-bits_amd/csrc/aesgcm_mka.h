// aesgcm_mka.h -- MACsec's MKA on the device (aesgcm_mka_*, include/aesgcm.h "MACSEC MKA"): a table of CAKs with their Keyids, the AES-CMAC KDF of IEEE 802.1X-2010 6.2
// (SAK and KEK from the CAK) and AES Key Wrap of RFC 3394 (the SAK under the KEK, both directions), a lane per entry.  Shared by the kernels (aesgcm_mka_kernels.hip),
// the host side (aesgcm_mka.hip) and the CPU harness tests/mka_emul, which runs the same CBC-MAC, the same wrap steps, the same inverse cipher and the same verdicts
// against an independent AES: everything a lane COMPUTES and DECIDES is here, HD.
//
// STATE.  n_caks records of MKA_REC_WORDS = KDF_REC_WORDS 32-bit words (64 bytes, as aesgcm_kdf.h): the CAK's cak_len bytes as they are (words 0 .. 7), the 16-byte
// Keyid in bytes 32 .. 47 (words 8 .. 11), zeros, and in the last word MKA_SET once the record holds a CAK (zero = unset or cleared).  No call copies a record out.
// The contexts are NOT state: they come per entry from the caller's buffer.
//
// THE PRF is AES-CMAC (RFC 4493): a CBC-MAC whose last block takes the subkey K1 (the message fills its last block) or K2 (it does not: 10* padding), K1 = 2 L,
// K2 = 4 L in GF(2^128) with 0x87, L = E(0^128).  Blocks, keys and outputs are memory-order words throughout (aesgcm_base.h), so the PRF's output words ARE the derived
// key's words: no byte swap between PRF and schedule; only the subkey doubling reads a block as a big-endian number.  The KDF's message is
//     ctr | label[12] | 0x00 | context | be16(bits)          (16 + len bytes)
// The CBC-MAC (mka_cmac) takes its message through a function of the byte position and runs its blocks in a loop that is not unrolled -- THE BLOCK COUNT IS A RUN-TIME
// VALUE, as aesgcm_prfplus.h's -- one AES in it.  The KDF's function (mka_prf) answers the first three words from constants (both labels differ in ONE word) and the
// rest from the context's bytes at any alignment (mka_ctx_word); the word in which the context ends carries its tail, the length field and the padding's 0x80.  No
// register array is indexed by a run-time value.
//
// KEY WRAP.  RFC 3394 2.2.1 / 2.2.2 with the index loop turned into a ROTATION of the register array: step t = n j + i works on the pair at the array's front (wrap) or
// brings the last pair to the front first (unwrap), so the loop over the 6 n steps is not unrolled, holds one cipher call, and indexes nothing by a run-time value.
//
// THE INVERSE CIPHER (unwrap only; the library's first) runs over the FORWARD round keys in FIPS-197 5.3's order: AddRoundKey(NR), then per round InvShiftRows,
// InvSubBytes, AddRoundKey, InvMixColumns.  InvSubBytes reads a 256-byte table in LDS (MKA_LDS_INV_OFF, behind T0 | T2) that the workgroup's 256 lanes build at kernel
// start from the S-box byte of the staged T0: inv[S[tid]] = tid (mka_fill_inv).  InvMixColumns is arithmetic on a whole column word: the circulant (5, 0, 4, 0) --
// w ^= 4 (w ^ rot16 w) -- then the forward MixColumns 2 (w ^ rotr8 w) ^ rotr8 w ^ rot16 w ^ rotr24 w, with xtime on four packed bytes.
#pragma once
#include "aesgcm_kdf_slot.h"
#include "aesgcm_kdf.h"

#define MKA_REC_WORDS KDF_REC_WORDS
#define MKA_SET 0x53454443u                /* "CDES": the record holds a CAK and its Keyid */
#define MKA_KEYID_WORD 8u                  /* the Keyid's first word in a record */
#define MKA_KEYID_LEN 16u
#define MKA_CTX_MAX 2048u                  /* KS-nonce | MI-value list | KN of the largest group a caller may bring */
#define MKA_IV_WORD 0xA6A6A6A6u            /* RFC 3394 2.2.3.1: the default initial value, as either memory-order word */
#define MKA_LDS_INV_OFF (AESGCM_LDS_AES_OFF + AESGCM_LDS_AES)       /* the inverse S-box: 256 bytes behind T0 | T2 */
#define MKA_LDS_BYTES (MKA_LDS_INV_OFF + 256u)
#define MKA_INSTALLED 0u                   /* a verdict byte of aesgcm_mka_unwrap_dev */
#define MKA_REFUSED 1u
#define MKA_BAD_ICV 2u
// "IEEE8021 KEK" / "IEEE8021 SAK" behind the counter byte, as the memory-order words of block 0: ctr I E E | E 8 0 2 | 1 ' ' K E or 1 ' ' S A | K 00 . .
#define MKA_W0 (((u32)'I' << 8) | ((u32)'E' << 16) | ((u32)'E' << 24))
#define MKA_W1 ((u32)'E' | ((u32)'8' << 8) | ((u32)'0' << 16) | ((u32)'2' << 24))
#define MKA_W2_KEK ((u32)'1' | ((u32)' ' << 8) | ((u32)'K' << 16) | ((u32)'E' << 24))
#define MKA_W2_SAK ((u32)'1' | ((u32)' ' << 8) | ((u32)'S' << 16) | ((u32)'A' << 24))
#define MKA_W3 ((u32)'K')

#if defined(__HIP_DEVICE_COMPILE__)
#define LDS_LD8(lds, off) ((u32) * (const __attribute__((address_space(3))) unsigned char *)(uintptr_t)(off))
#else
#define LDS_LD8(lds, off) ((u32)(lds)[off])
#endif

// ---------------------------------------------------------------- the inverse cipher
// what lane tid of the 256 writes, behind the barrier that follows main_fill_lds (T0's byte 1 is S[x], aesgcm_base.h te0_calc); a barrier behind it too
HD void mka_fill_inv(unsigned char *smem, u32 tid) {
    const u32 s = (LDS_LD32(smem, AESGCM_LDS_AES_OFF + (tid << 8)) >> 8) & 0xFFu;
    smem[MKA_LDS_INV_OFF + s] = (unsigned char)tid;
}
// xtime on the four bytes of a word
HD u32 mka_xt4(u32 w) { return ((w & 0x7F7F7F7Fu) << 1) ^ (((w >> 7) & 0x01010101u) * 0x1Bu); }
// InvMixColumns of one column (row 0 in the low byte)
HD u32 mka_inv_mix(u32 w) {
    w ^= mka_xt4(mka_xt4(w ^ rotl32(w, 16)));
    const u32 r8 = rotl32(w, 24);
    return mka_xt4(w ^ r8) ^ r8 ^ rotl32(w, 16) ^ rotl32(w, 8);
}
// InvShiftRows and InvSubBytes for one column: row q comes from the column q places to the LEFT (r0 .. r3: those columns' words)
HD u32 mka_inv_sub(const unsigned char *smem, u32 r0, u32 r1, u32 r2, u32 r3) {
    return LDS_LD8(smem, MKA_LDS_INV_OFF + (r0 & 0xFFu)) | (LDS_LD8(smem, MKA_LDS_INV_OFF + ((r1 >> 8) & 0xFFu)) << 8) |
           (LDS_LD8(smem, MKA_LDS_INV_OFF + ((r2 >> 16) & 0xFFu)) << 16) | (LDS_LD8(smem, MKA_LDS_INV_OFF + (r3 >> 24)) << 24);
}
// s = D_K(s): rk the FORWARD schedule, 4 * (NR + 1) memory-order words
template <int NR>
HD void mka_aes_inv(u32 &s0, u32 &s1, u32 &s2, u32 &s3, const u32 *__restrict__ rk, const unsigned char *smem) {
    s0 ^= rk[4 * NR]; s1 ^= rk[4 * NR + 1]; s2 ^= rk[4 * NR + 2]; s3 ^= rk[4 * NR + 3];
#pragma unroll
    for (int r = NR - 1; r >= 1; r--) {
        const u32 t0 = mka_inv_sub(smem, s0, s3, s2, s1) ^ rk[4 * r], t1 = mka_inv_sub(smem, s1, s0, s3, s2) ^ rk[4 * r + 1];
        const u32 t2 = mka_inv_sub(smem, s2, s1, s0, s3) ^ rk[4 * r + 2], t3 = mka_inv_sub(smem, s3, s2, s1, s0) ^ rk[4 * r + 3];
        s0 = mka_inv_mix(t0); s1 = mka_inv_mix(t1); s2 = mka_inv_mix(t2); s3 = mka_inv_mix(t3);
    }
    const u32 t0 = mka_inv_sub(smem, s0, s3, s2, s1) ^ rk[0], t1 = mka_inv_sub(smem, s1, s0, s3, s2) ^ rk[1];
    const u32 t2 = mka_inv_sub(smem, s2, s1, s0, s3) ^ rk[2], t3 = mka_inv_sub(smem, s3, s2, s1, s0) ^ rk[3];
    s0 = t0; s1 = t1; s2 = t2; s3 = t3;
}

// ---------------------------------------------------------------- AES-CMAC and the KDF
struct MkaSub { u32 k1[4], k2[4]; };
// out = 2 in in GF(2^128), the block read as a big-endian number (RFC 4493 2.3: shift left, 0x87 into the last byte where a bit fell out)
HD void mka_dbl(const u32 *in, u32 *out) {
    const u32 b0 = bswap32(in[0]), b1 = bswap32(in[1]), b2 = bswap32(in[2]), b3 = bswap32(in[3]);
    out[0] = bswap32((b0 << 1) | (b1 >> 31)); out[1] = bswap32((b1 << 1) | (b2 >> 31)); out[2] = bswap32((b2 << 1) | (b3 >> 31));
    out[3] = bswap32((b3 << 1) ^ ((b0 >> 31) * 0x87u));
}
template <int NR> HD void mka_subkeys(const u32 *rk, const unsigned char *smem, u32 lb, MkaSub &k) {
    u32 l[4] = {rk[0], rk[1], rk[2], rk[3]};
    aes_rounds_lds<NR>(l[0], l[1], l[2], l[3], rk, smem, lb);             // L = E_K(0^128)
    mka_dbl(l, k.k1);
    mka_dbl(k.k1, k.k2);
}
// Byte q of context | be16(bits) | 0x80 | zeros ..., the context = len bytes at c.  No byte at or behind c + len is read
HD u32 mka_ctx_byte(const unsigned char *c, u32 len, u32 q, u32 bits) {
    return q < len ? (u32)c[q] : q == len ? (bits >> 8) & 0xFFu : q == len + 1u ? bits & 0xFFu : q == len + 2u ? 0x80u : 0u;
}
// ... and its memory-order word at bytes q .. q + 3: a word inside the context is four byte loads
HD u32 mka_ctx_word(const unsigned char *c, u32 len, u32 q, u32 bits) {
    if (q < len && len - q >= 4u) return (u32)c[q] | ((u32)c[q + 1u] << 8) | ((u32)c[q + 2u] << 16) | ((u32)c[q + 3u] << 24);
    u32 w = 0u;
#pragma unroll
    for (u32 b = 0; b < 4u; b++) w |= mka_ctx_byte(c, len, q + b, bits) << (8u * b);
    return w;
}
// x = AES-CMAC(K, M) (RFC 4493 2.4): rk K's schedule, sub its subkeys, M of n bytes (0 too), word(q) its memory-order word at byte q = 0, 4, 8, ... WITH the padding's
// 0x80 at byte n and zeros behind it.  The last block takes K1 where M fills it and K2 where it does not (or M is empty).  One AES in a loop that is not unrolled
template <int NR, class Word>
HD void mka_cmac(const u32 *__restrict__ rk, const MkaSub &sub, const unsigned char *smem, u32 lb, u32 n, Word word, u32 *x) {
    const u32 nb = n ? (n + 15u) / 16u : 1u;
    const bool whole = n != 0u && (n & 15u) == 0u;
    u32 s0 = 0u, s1 = 0u, s2 = 0u, s3 = 0u;
#pragma nounroll
    for (u32 b = 0; b < nb; b++) {
        u32 m0 = word(16u * b), m1 = word(16u * b + 4u), m2 = word(16u * b + 8u), m3 = word(16u * b + 12u);
        if (b + 1u == nb) {
            m0 ^= whole ? sub.k1[0] : sub.k2[0]; m1 ^= whole ? sub.k1[1] : sub.k2[1]; m2 ^= whole ? sub.k1[2] : sub.k2[2]; m3 ^= whole ? sub.k1[3] : sub.k2[3];
        }
        s0 ^= m0 ^ rk[0]; s1 ^= m1 ^ rk[1]; s2 ^= m2 ^ rk[2]; s3 ^= m3 ^ rk[3];
        aes_rounds_lds<NR>(s0, s1, s2, s3, rk, smem, lb);
    }
    x[0] = s0; x[1] = s1; x[2] = s2; x[3] = s3;
}
// x = PRF(K, ctr | label | 0x00 | context | be16(bits)): 16 + len bytes.  w2 is the label's word that tells KEK from SAK; the context begins at byte 14, so the words
// 0 .. 2 are constants, word 3 holds the context's (or the length field's) first two bytes, and every word behind it is mka_ctx_word 14 bytes back
template <int NR>
HD void mka_prf(const u32 *__restrict__ rk, const MkaSub &sub, const unsigned char *smem, u32 lb, u32 ctr, u32 w2, const unsigned char *c, u32 len, u32 bits, u32 *x) {
    mka_cmac<NR>(rk, sub, smem, lb, 16u + len, [&](u32 q) {
        return q == 0u ? (ctr | MKA_W0) : q == 4u ? MKA_W1 : q == 8u ? w2 :
               q == 12u ? (MKA_W3 | (mka_ctx_byte(c, len, 0u, bits) << 16) | (mka_ctx_byte(c, len, 1u, bits) << 24)) : mka_ctx_word(c, len, q - 14u, bits);
    }, x);
}
// out[0 .. NKO - 1] = KDF(K, label, context, 32 NKO bits) as memory-order words: one iteration for 128 bits, two for 256
template <int NR, int NKO>
HD void mka_kdf(const u32 *__restrict__ rk, const MkaSub &sub, const unsigned char *smem, u32 lb, u32 w2, const unsigned char *c, u32 len, u32 *out) {
    static_assert(NKO == 4 || NKO == 8, "MACsec has AES-128 and AES-256");
#pragma nounroll
    for (u32 it = 0; it < (u32)(NKO / 4); it++) {
        u32 x[4];
        mka_prf<NR>(rk, sub, smem, lb, it + 1u, w2, c, len, 32u * (u32)NKO, x);
        if (it == 0u) { out[0] = x[0]; out[1] = x[1]; out[2] = x[2]; out[3] = x[3]; }
        else { out[NKO - 4] = x[0]; out[NKO - 3] = x[1]; out[NKO - 2] = x[2]; out[NKO - 1] = x[3]; }
    }
}

// ---------------------------------------------------------------- RFC 3394
// wrap: r[0 .. NK - 1] the key's words -> a | r the NK + 2 wrapped words.  rk: the KEK's schedule
template <int NR, int NK>
HD void mka_wrap(const u32 *__restrict__ rk, const unsigned char *smem, u32 lb, u32 *a, u32 *r) {
    a[0] = MKA_IV_WORD; a[1] = MKA_IV_WORD;
#pragma nounroll
    for (u32 t = 1; t <= 3u * (u32)NK; t++) {                             // 6 n steps, n = NK / 2
        u32 s0 = a[0] ^ rk[0], s1 = a[1] ^ rk[1], s2 = r[0] ^ rk[2], s3 = r[1] ^ rk[3];
        aes_rounds_lds<NR>(s0, s1, s2, s3, rk, smem, lb);
        a[0] = s0; a[1] = s1 ^ (t << 24);                                 // A = MSB64(B) ^ t: t < 256 meets the number's last byte
#pragma unroll
        for (int k = 0; k < NK - 2; k++) r[k] = r[k + 2];                 // the pair that was worked on goes to the back
        r[NK - 2] = s2; r[NK - 1] = s3;
    }
}
// unwrap: a | r the wrapped words -> a the recovered initial value, r the candidate key
template <int NR, int NK>
HD void mka_unwrap(const u32 *__restrict__ rk, const unsigned char *smem, u32 *a, u32 *r) {
#pragma nounroll
    for (u32 t = 3u * (u32)NK; t >= 1u; t--) {
        const u32 l0 = r[NK - 2], l1 = r[NK - 1];                         // the last pair comes to the front
#pragma unroll
        for (int k = NK - 1; k >= 2; k--) r[k] = r[k - 2];
        u32 s0 = a[0], s1 = a[1] ^ (t << 24), s2 = l0, s3 = l1;
        mka_aes_inv<NR>(s0, s1, s2, s3, rk, smem);
        a[0] = s0; a[1] = s1; r[0] = s2; r[1] = s3;
    }
}

// ---------------------------------------------------------------- the table and what a lane decides
struct MkaTable {
    u32 *rec;                              // n_caks records
    u32 *status;                           // lowest refused entry (atomic min, kdf_refuse), ~0 = none
    u32 n_caks, cak_len;
};
struct MkaInstallParams {
    MkaTable t;
    const u32 *idx, *slots;                // n each
    const unsigned char *ctx;              // entry i's context: bytes [ctx_off[i], ctx_off[i + 1])
    const u32 *ctx_off;                    // n + 1
    unsigned char *wrapped;                // n * (key_len + 8) bytes at any address, or NULL
    KtSlot *tab;
    u32 n, n_slots;
};
struct MkaUnwrapParams {
    MkaTable t;
    const u32 *idx, *slots;                // n each
    const unsigned char *wrapped;          // n * (key_len + 8) bytes at any address
    unsigned char *verdict;                // n bytes, or NULL
    KtSlot *tab;
    u32 n, n_slots;
};
struct MkaSetParams {
    MkaTable t;
    const u32 *idx;
    const unsigned char *caks, *keyids;    // n * cak_len and n * 16 bytes
    u32 n;
};

HD bool mka_rec_set(const MkaTable &t, u32 r) { return r < t.n_caks && t.rec[(size_t)r * MKA_REC_WORDS + MKA_REC_WORDS - 1u] == MKA_SET; }
// a whole record from a CAK and a 16-byte Keyid at any byte address: the marker last.  The host's set packs its copy with it, the set kernel's lane stores with it
HD void mka_store(const MkaTable &t, u32 r, const unsigned char *cak, const unsigned char *keyid) {
    u32 *rec = t.rec + (size_t)r * MKA_REC_WORDS;
    for (u32 k = 0; k < MKA_REC_WORDS - 1u; k++) {
        u32 w = 0;
        for (u32 b = 0; b < 4u; b++) {
            const u32 at = 4u * k + b;                                            // the byte's place in the record
            if (at < t.cak_len) w |= (u32)cak[at] << (8u * b);
            else if (at >= 4u * MKA_KEYID_WORD && at < 4u * MKA_KEYID_WORD + MKA_KEYID_LEN) w |= (u32)keyid[at - 4u * MKA_KEYID_WORD] << (8u * b);
        }
        rec[k] = w;
    }
    rec[MKA_REC_WORDS - 1u] = MKA_SET;
}
HD void mka_set_lane(const MkaSetParams &p, u32 i) {
    const u32 r = p.idx[i];
    if (r >= p.t.n_caks) { kdf_refuse(p.t.status, i); return; }
    mka_store(p.t, r, p.caks + (size_t)i * p.t.cak_len, p.keyids + (size_t)i * MKA_KEYID_LEN);
}
// the record's CAK into rk, its schedule in place, its CMAC subkeys
template <int NRC> HD void mka_cak(const MkaTable &t, u32 r, u32 *rk, const unsigned char *smem, u32 lb, MkaSub &sub) {
    const u32 *rec = t.rec + (size_t)r * MKA_REC_WORDS;
#pragma unroll
    for (int k = 0; k < NRC - 6; k++) rk[k] = rec[k];
    kdf_key_schedule<NRC>(rk, smem, lb);
    mka_subkeys<NRC>(rk, smem, lb, sub);
}
// rk (the CAK's schedule, sub its subkeys) -> the KEK's schedule: KEK = KDF(CAK, "IEEE8021 KEK", Keyid, 8 cak_len), the Keyid read from the record's own bytes
template <int NRC> HD void mka_kek(const MkaTable &t, u32 r, u32 *rk, const MkaSub &sub, const unsigned char *smem, u32 lb) {
    u32 kek[NRC - 6];
    mka_kdf<NRC, NRC - 6>(rk, sub, smem, lb, MKA_W2_KEK, reinterpret_cast<const unsigned char *>(t.rec + (size_t)r * MKA_REC_WORDS + MKA_KEYID_WORD), MKA_KEYID_LEN, kek);
#pragma unroll
    for (int k = 0; k < NRC - 6; k++) rk[k] = kek[k];
    kdf_key_schedule<NRC>(rk, smem, lb);
}
// Entry i of an install call (the key server).  The tests in this order: the record in range; the record set; the slot in range; the context's offsets rising (an empty
// context falls under this) and at most MKA_CTX_MAX apart.  A refused entry reports itself and NOTHING it names is written.  Otherwise: SAK = KDF(CAK, "IEEE8021 SAK",
// context, 8 key_len); where the call asked for wrapped output, the KEK's schedule takes the CAK's registers and entry i's key_len + 8 wrapped bytes are stored; then
// -> true, slot, and rk[0 .. NRS - 7] = the SAK's words for the slot build.  rk: 4 * (max(NRC, NRS) + 1) words of the lane's registers
template <int NRC, int NRS>
HD bool mka_install_lane(const MkaInstallParams &p, u32 i, const unsigned char *smem, u32 lb, u32 *rk, u32 &slot) {
    constexpr int NKS = NRS - 6;
    const u32 rec = p.idx[i];
    if (!mka_rec_set(p.t, rec)) { kdf_refuse(p.t.status, i); return false; }
    slot = p.slots[i];
    if (slot >= p.n_slots) { kdf_refuse(p.t.status, i); return false; }
    const u32 from = p.ctx_off[i], to = p.ctx_off[i + 1u];
    if (to <= from || to - from > MKA_CTX_MAX) { kdf_refuse(p.t.status, i); return false; }
    MkaSub sub;
    u32 sak[NKS];
    mka_cak<NRC>(p.t, rec, rk, smem, lb, sub);
    mka_kdf<NRC, NKS>(rk, sub, smem, lb, MKA_W2_SAK, p.ctx + from, to - from, sak);
    if (p.wrapped) {                                                      // (uniform: the call's)
        u32 a[2], r[NKS];
        mka_kek<NRC>(p.t, rec, rk, sub, smem, lb);
#pragma unroll
        for (int k = 0; k < NKS; k++) r[k] = sak[k];
        mka_wrap<NRC, NKS>(rk, smem, lb, a, r);
        unsigned char *w = p.wrapped + (size_t)i * (4u * NKS + 8u);
        gstore4_any(w, a[0]); gstore4_any(w + 4, a[1]);
#pragma unroll
        for (int k = 0; k < NKS; k++) gstore4_any(w + 8 + 4 * k, r[k]);
    }
#pragma unroll
    for (int k = 0; k < NKS; k++) rk[k] = sak[k];
    return true;
}
// Entry i of an unwrap call (any other station).  The tests in this order: the record in range; the record set; the slot in range (verdict MKA_REFUSED); then the KEK
// unwraps the entry's key_len + 8 bytes, and a recovered initial value other than A6 x 8 is MKA_BAD_ICV.  A refused entry reports itself, its verdict byte (where the
// call has them) is the only byte it gets.  Otherwise -> true, slot, verdict MKA_INSTALLED and rk[0 .. NRS - 7] = the SAK's words for the slot build
template <int NRC, int NRS>
HD bool mka_unwrap_lane(const MkaUnwrapParams &p, u32 i, const unsigned char *smem, u32 lb, u32 *rk, u32 &slot) {
    constexpr int NKS = NRS - 6;
    const u32 rec = p.idx[i];
    bool named = mka_rec_set(p.t, rec);
    if (named) { slot = p.slots[i]; named = slot < p.n_slots; }
    if (!named) {
        kdf_refuse(p.t.status, i);
        if (p.verdict) p.verdict[i] = (unsigned char)MKA_REFUSED;
        return false;
    }
    MkaSub sub;
    u32 a[2], r[NKS];
    mka_cak<NRC>(p.t, rec, rk, smem, lb, sub);
    mka_kek<NRC>(p.t, rec, rk, sub, smem, lb);
    const unsigned char *w = p.wrapped + (size_t)i * (4u * NKS + 8u);
    a[0] = gload4_any(w); a[1] = gload4_any(w + 4);
#pragma unroll
    for (int k = 0; k < NKS; k++) r[k] = gload4_any(w + 8 + 4 * k);
    mka_unwrap<NRC, NKS>(rk, smem, a, r);
    if (a[0] != MKA_IV_WORD || a[1] != MKA_IV_WORD) {
        kdf_refuse(p.t.status, i);
        if (p.verdict) p.verdict[i] = (unsigned char)MKA_BAD_ICV;
        return false;
    }
    if (p.verdict) p.verdict[i] = (unsigned char)MKA_INSTALLED;
#pragma unroll
    for (int k = 0; k < NKS; k++) rk[k] = r[k];
    return true;
}

// launchers (aesgcm_mka_kernels.hip)
struct DevTables;
hipError_t klaunch_mka_attributes();                                  // hipFuncSetAttribute(MaxDynamicSharedMemorySize) of the install and unwrap kernels' instances, on the current device
hipError_t klaunch_mka_install(int nr, hipStream_t st, const DevTables *tb, const MkaInstallParams &p);
hipError_t klaunch_mka_unwrap(int nr, hipStream_t st, const DevTables *tb, const MkaUnwrapParams &p);
hipError_t klaunch_mka_set(hipStream_t st, const MkaSetParams &p);
