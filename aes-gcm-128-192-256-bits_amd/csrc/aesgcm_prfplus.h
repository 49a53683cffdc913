// aesgcm_prfplus.h -- IKEv2's prf+ on the device (aesgcm_prfplus_*, include/aesgcm.h "IKEv2 PRF+"): a table of SK_d values, and the ESP AES-GCM keying material of
// Child SAs cut from prf+(SK_d, seed) of RFC 7296 2.13 over HMAC-SHA-256 / -384 / -512, a lane per direction.  Shared by the kernels (aesgcm_prfplus_kernels.hip), the
// host side (aesgcm_prfplus.hip) and the CPU harness tests/prfplus_emul, which runs the same HMACs and the same verdicts against hmac: everything a lane COMPUTES and
// DECIDES is here, HD.
//
// STATE.  n_keys records of PRFP_REC_WORDS = 32 32-bit words (128 bytes) for every hash: the 64 bytes of a SHA-512 SK_d and a marker do not fit the 64-byte record of
// aesgcm_kdf.h, and one record size serves the three hashes.  SK_d's hash_len bytes as they are (words 0 .. 7, 11 or 15), zeros, and in the LAST word PRFP_SET once the
// record holds an SK_d (zero = unset or cleared).  No call copies a record out.  The seeds are NOT state: they come per entry from the caller's buffer.
//
// THE SHAPE.  prf+(K, S) = T1 | T2 | ..., T1 = prf(K, S | 0x01), Tn = prf(K, T(n-1) | S | n).  K is hash_len bytes, less than a block, so the ipad and the opad state
// are ONE compression each, made once per lane (PrfpKey).  S is 1 .. PRFP_SEED_MAX bytes at any address, so -- unlike every other HMAC of the library -- the message's
// BLOCK COUNT IS A RUN-TIME VALUE (prfp_hmac): a loop over the blocks that is not unrolled, one compression in it.  T(n-1) lies at byte 0 of its message and is a
// multiple of four bytes, so its words have constant indices in block 0 and the seed's words stay whole words behind it.  A seed word is assembled from bytes inside
// the block loop (prfp_seed_word); the word in which the seed ends carries its tail bytes, the counter byte n and the padding's 0x80 (which may fall into the next
// word: the same function makes it), every word behind them is zero, and the last block's last word is the bit length.  No register array is indexed by a run-time
// value.  The pad states, the outer hash and the compressions are aesgcm_kdf.h's (kdf_hmac_pad, kdf_hmac_outer, KdfHash<HL>), as they are.
//
// WHAT A LANE TAKES.  KEYMAT = key_i2r | salt_i2r[4] | key_r2i | salt_r2i[4] (RFC 7296 2.17, RFC 4106 8.1): direction dir's NK + 1 words start at stream word
// dir * (NK + 1).  The T(n) come in a loop that is NOT unrolled and ends with the last T(n) the window needs; aesgcm_prf12.h's prf12_pick copies the words that fall
// into the window by compares with constants.  The r2i lane repeats the T(n) the i2r lane made (two or three HMACs): a lane per direction, never a lane for a salt.
#pragma once
#include "aesgcm_prf12.h"

#define PRFP_REC_WORDS 32u
#define PRFP_SET 0x53454449u               /* "IDES": the record holds an SK_d */
#define PRFP_SEED_MAX 2048u                /* g^ir of MODP-8192 and two 256-byte nonces */
#define PRFP_NONE 0xFFFFFFFFu              /* an entry of a slot array that installs nothing for that direction */
#define PRFP_I2R 0u                        /* a direction: the index into PrfpInstallParams::slots, blockIdx.y of the install kernel */
#define PRFP_R2I 1u

// ---------------------------------------------------------------- the HMAC whose block count is a run-time value
// the ipad and the opad state of SK_d (skd: HL / 4 big-endian words)
template <int HL> struct PrfpKey { typename KdfHash<HL>::word in[8], out[8]; };
template <int HL> HD void prfp_key(const u32 *skd, PrfpKey<HL> &k) {
    kdf_hmac_pad<HL, HL / 4>(skd, KDF_IPAD, k.in);
    kdf_hmac_pad<HL, HL / 4>(skd, KDF_OPAD, k.out);
}
// Big-endian word j of S | ctr | 0x80 | zeros ..., S = len bytes at s (any alignment).  A word that lies inside the seed is four byte loads; the others take each byte
// by its place: the seed's, the counter behind its last, the 0x80 behind that, zero from there on.  No byte at or behind s + len is read
HD u32 prfp_seed_word(const unsigned char *s, u32 len, u32 j, u32 ctr) {
    const u32 o = 4u * j;
    if (o < len && len - o >= 4u) return ((u32)s[o] << 24) | ((u32)s[o + 1u] << 16) | ((u32)s[o + 2u] << 8) | s[o + 3u];
    u32 w = 0u;
#pragma unroll
    for (u32 b = 0; b < 4u; b++) {
        const u32 q = o + b;
        w = (w << 8) | (q < len ? (u32)s[q] : q == len ? ctr : q == len + 1u ? 0x80u : 0u);
    }
    return w;
}
// how many blocks the message T | S | n takes behind the ipad block: tw = T's words (0 for T1), len = the seed's bytes; the counter, the 0x80 and the length field go in
template <int HL> HD u32 prfp_blocks(u32 tw, u32 len) { return (4u * tw + len + 2u + KdfHash<HL>::LEN_BYTES + KdfHash<HL>::BLOCK - 1u) / KdfHash<HL>::BLOCK; }
// t = HMAC(K, t[0 .. tw - 1] | S | ctr): tw = 0 (T1: t is not read) or HL / 4; t: HL / 4 big-endian words, in and out
template <int HL> HD void prfp_hmac(const PrfpKey<HL> &key, u32 *t, u32 tw, const unsigned char *s, u32 len, u32 ctr) {
    typedef KdfHash<HL> H;
    constexpr int WPB = (int)(H::BLOCK / 4u);                          // 32-bit message words per block
    typename H::word st[8];
#pragma unroll
    for (int k = 0; k < 8; k++) st[k] = key.in[k];
    const u32 nb = prfp_blocks<HL>(tw, len), bits = (H::BLOCK + 4u * tw + len + 1u) * 8u;
#pragma nounroll
    for (u32 b = 0; b < nb; b++) {
        u32 m[WPB];
#pragma unroll
        for (int k = 0; k < WPB; k++) {
            const bool of_t = k < HL / 4 && b == 0u && (u32)k < tw;     // (only block 0 holds T, at the words k themselves)
            m[k] = of_t ? t[k < HL / 4 ? k : 0] : prfp_seed_word(s, len, b * (u32)WPB + (u32)k - tw, ctr);
        }
        typename H::word w[16];
#pragma unroll
        for (int k = 0; k < 16; k++) w[k] = H::template at<WPB>(m, k);
        if (b + 1u == nb) w[15] = bits;
        H::block(st, w);
    }
    kdf_hmac_outer<HL>(key.out, st, t);
}
// prf+(skd, S): take(j, t) sees T(j + 1) for j = 0 .. n_t - 1 (n_t <= 255: the counter is a byte; the callers here need at most three)
template <int HL, class Take> HD void prfp_plus(const u32 *skd, const unsigned char *s, u32 len, u32 n_t, Take take) {
    PrfpKey<HL> key;
    u32 t[HL / 4];
    prfp_key(skd, key);
#pragma unroll
    for (int k = 0; k < HL / 4; k++) t[k] = 0u;
#pragma nounroll
    for (u32 j = 0; j < n_t; j++) {
        prfp_hmac<HL>(key, t, j ? (u32)(HL / 4) : 0u, s, len, j + 1u);
        take(j, t);
    }
}

// ---------------------------------------------------------------- the table and what a lane decides
struct PrfpTable {
    u32 *rec;                              // n_keys records
    u32 *status;                           // lowest refused entry (atomic min, kdf_refuse), ~0 = none
    u32 n_keys, hash_len;
};
struct PrfpInstallParams {
    PrfpTable t;
    const u32 *idx;                        // n
    const unsigned char *seed;             // entry i's seed: bytes [seed_off[i], seed_off[i + 1])
    const u32 *seed_off;                   // n + 1
    const u32 *slots[2];                   // by direction: n each, or NULL (not both)
    KtSlot *tab;
    u32 n, n_slots;
};
struct PrfpSetParams {
    PrfpTable t;
    const u32 *idx;
    const unsigned char *keys;             // n * hash_len bytes
    u32 n;
};

HD bool prfp_rec_set(const PrfpTable &t, u32 r) { return r < t.n_keys && t.rec[(size_t)r * PRFP_REC_WORDS + PRFP_REC_WORDS - 1u] == PRFP_SET; }
// a whole record from bytes at any address: the marker last.  The host's set packs its copy with it, the set kernel's lane stores with it
HD void prfp_store(const PrfpTable &t, u32 r, const unsigned char *key) {
    u32 *rec = t.rec + (size_t)r * PRFP_REC_WORDS;
    for (u32 k = 0; k < PRFP_REC_WORDS - 1u; k++) {
        u32 w = 0u;
        if (4u * k < t.hash_len) {                                    // (no pointer is formed behind the key's hash_len bytes)
            const unsigned char *b = key + 4u * k;
            w = (u32)b[0] | ((u32)b[1] << 8) | ((u32)b[2] << 16) | ((u32)b[3] << 24);
        }
        rec[k] = w;
    }
    rec[PRFP_REC_WORDS - 1u] = PRFP_SET;
}
// the record's SK_d as big-endian words
template <int HL> HD void prfp_load(const PrfpTable &t, u32 r, u32 *skd) {
    const u32 *rec = t.rec + (size_t)r * PRFP_REC_WORDS;
#pragma unroll
    for (int k = 0; k < HL / 4; k++) skd[k] = bswap32(rec[k]);
}
// Entry i of an install call: both lanes of the entry come to the same verdict from the same words, so an entry is written whole or not at all.  The tests in this
// order: the record in range; the record set; the i2r slot, where the call has that array and the entry names one, below n_slots; the r2i slot; the seed's offsets
// rising (an empty seed falls under this) and at most PRFP_SEED_MAX apart.  -> s, len: the entry's seed
HD bool prfp_entry(const PrfpInstallParams &p, u32 i, u32 &rec, u32 *slot, const unsigned char *&s, u32 &len) {
    rec = p.idx[i];
    if (!prfp_rec_set(p.t, rec)) return false;
    slot[PRFP_I2R] = p.slots[PRFP_I2R] ? p.slots[PRFP_I2R][i] : PRFP_NONE;
    if (slot[PRFP_I2R] != PRFP_NONE && slot[PRFP_I2R] >= p.n_slots) return false;
    slot[PRFP_R2I] = p.slots[PRFP_R2I] ? p.slots[PRFP_R2I][i] : PRFP_NONE;
    if (slot[PRFP_R2I] != PRFP_NONE && slot[PRFP_R2I] >= p.n_slots) return false;
    const u32 from = p.seed_off[i], to = p.seed_off[i + 1u];
    if (to <= from || to - from > PRFP_SEED_MAX) return false;
    s = p.seed + from; len = to - from;
    return true;
}
// What the lane of direction dir derives: out[0 .. NK - 1] = the key, out[NK] = the salt's four bytes, as big-endian words.  Nothing is stored
template <int HL, int NK> HD void prfp_install_derive(const PrfpInstallParams &p, u32 rec, u32 dir, const unsigned char *s, u32 len, u32 *out) {
    u32 skd[HL / 4];
    prfp_load<HL>(p.t, rec, skd);
    const u32 first = dir * (u32)(NK + 1);
#pragma unroll
    for (int k = 0; k < NK + 1; k++) out[k] = 0u;
    prfp_plus<HL>(skd, s, len, prf12_count<HL>(first + (u32)(NK + 1)), [&](u32 j, const u32 *t) { prf12_pick<HL, NK + 1>(j, t, first, out); });
}
HD void prfp_set_lane(const PrfpSetParams &p, u32 i) {
    const u32 r = p.idx[i];
    if (r >= p.t.n_keys) { kdf_refuse(p.t.status, i); return; }
    prfp_store(p.t, r, p.keys + (size_t)i * p.t.hash_len);
}

// launchers (aesgcm_prfplus_kernels.hip)
struct DevTables;
hipError_t klaunch_prfp_attributes();                                 // hipFuncSetAttribute(MaxDynamicSharedMemorySize) of the install kernel's instances, on the current device
hipError_t klaunch_prfp_install(int nr, hipStream_t st, const DevTables *tb, const PrfpInstallParams &p);      // grid: entries x 2 directions
hipError_t klaunch_prfp_set(hipStream_t st, const PrfpSetParams &p);
