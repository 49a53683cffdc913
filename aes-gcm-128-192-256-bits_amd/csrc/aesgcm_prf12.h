// aesgcm_prf12.h -- the TLS 1.2 PRF on the device (aesgcm_prf12_*, include/aesgcm.h "TLS 1.2 PRF"): a table of master secrets with their connection's two randoms, and
// P_hash of RFC 5246 section 5 over HMAC-SHA-256 / HMAC-SHA-384, a lane per derived value.  Shared by the kernels (aesgcm_prf12_kernels.hip), the host side
// (aesgcm_prf12.hip) and the CPU harness tests/prf12_emul, which runs the same HMACs and the same verdicts against hmac: everything a lane COMPUTES and DECIDES is here, HD.
//
// STATE.  n_masters records of PRF12_REC_WORDS 32-bit words (128 bytes): the 48-byte master secret as it is (words 0 .. 11), the client random (words 12 .. 19), the
// server random (words 20 .. 27), zeros, and in the last word PRF12_SET once the record holds a master (zero = unset or cleared).  No call copies a record out.
//
// THE SHAPE.  P_hash(secret, seed) = T(1) | T(2) | ..., A(1) = HMAC(secret, seed), A(j) = HMAC(secret, A(j - 1)), T(j) = HMAC(secret, A(j) | seed), with
// seed = label | random | random.  The secret is 48 bytes, less than a block of either hash, so the ipad and the opad state are ONE compression each, made once per
// lane (Prf12Key).  With a label of 1 .. PRF12_LABEL_MAX = 20 bytes the seed is 65 .. 84 bytes and every message has a block count that no datum changes: the seed
// two blocks of SHA-256 and one of SHA-384, A(j) one, A(j) | seed two (the static_asserts under "the three HMACs" compute them; a label bound that breaks one fails the
// compile), plus one compression for the outer hash of each HMAC.  The label's LENGTH is a template argument: where the randoms fall in the blocks is known to the compiler, so
// no lane indexes its message schedule by a length.  The label's bytes are made into words on the HOST (prf12_label: a Prf12Label, passed by value), the randoms are
// shifted in behind them by constant amounts (prf12_seed), and the seed with its padding bit is 22 words in registers.  The compressions and the HMAC's pieces (kdf_hmac_pad, kdf_hmac_msg, kdf_hmac_outer) are aesgcm_kdf.h's, as they are.
//
// WHAT A LANE TAKES.  A lane wants some 32-bit words of the output stream (a key: words first .. first + NK - 1; an IV: one word; a salt: three).  The T(j) come in a
// loop that is NOT unrolled; inside it prf12_pick copies the words of T(j) that fall into the lane's window by compares of the loop counter with constants -- selects,
// no indexed register array -- and the loop ends with the last T(j) the window needs.  No derived byte is stored anywhere but in its slot field or master record.
#pragma once
#include "aesgcm_srtp_kdf.h"

#define PRF12_REC_WORDS 32u
#define PRF12_SET 0x53454450u              /* "PDES": the record holds a master secret and the randoms */
#define PRF12_MASTER_LEN 48u
#define PRF12_RANDOM_LEN 32u
#define PRF12_CR_WORD 12u                  /* the client random's first word in a record */
#define PRF12_SR_WORD 20u                  /* the server random's */
#define PRF12_LABEL_MAX 20u
#define PRF12_SEED_WORDS 22                /* 84 bytes of seed and the padding's 0x80: 85 bytes */
#define PRF12_NONE 0xFFFFFFFFu             /* an entry of a slot / record array that installs nothing for that direction */
#define PRF12_CLIENT 0u                    /* a direction: the index into Prf12InstallParams::slots and Prf12ExportParams::recs */
#define PRF12_SERVER 1u
#define PRF12_ROLE_IV 2u                   /* blockIdx.y of the install kernel = (what << 1) | direction: 0, 1 the client's and server's key; 2, 3 their IVs */
#define PRF12_LL_KEY_EXPANSION 13          /* strlen("key expansion"), RFC 5246 6.3 */
#define PRF12_LL_EXPORTER 19               /* strlen("EXTRACTOR-dtls_srtp"), RFC 5764 4.2 */

// ---------------------------------------------------------------- the label and the seed
// the label as big-endian words, zeros behind it
struct Prf12Label { u32 w[5]; };
HD void prf12_label(const unsigned char *label, u32 label_len, Prf12Label &m) {
    unsigned char b[20] = {0};
    if (label_len > PRF12_LABEL_MAX) label_len = PRF12_LABEL_MAX;      // (never: the host unit's labels are the two constants, the harness checks its own)
    for (u32 k = 0; k < label_len; k++) b[k] = label[k];
    for (u32 k = 0; k < 5u; k++) m.w[k] = ((u32)b[4 * k] << 24) | ((u32)b[4 * k + 1] << 16) | ((u32)b[4 * k + 2] << 8) | b[4 * k + 3];
}
// sw = label | r[0 .. 7] | r[8 .. 15] | 0x80 | zeros as big-endian words: LL bytes of label, r the two randoms as big-endian words in the seed's order
template <int LL> HD void prf12_seed(const Prf12Label &m, const u32 *r, u32 *sw) {
    static_assert(LL >= 1 && LL <= (int)PRF12_LABEL_MAX, "the block counts above hold for labels of 1 .. 20 bytes");
    constexpr int q = LL / 4, s = LL % 4;
#pragma unroll
    for (int k = 0; k < PRF12_SEED_WORDS; k++) sw[k] = k < 5 ? m.w[k] : 0u;
#pragma unroll
    for (int k = 0; k <= 16; k++) {
        if constexpr (s == 0) { if (k < 16) sw[q + k] |= r[k]; }
        else sw[q + k] |= (k > 0 ? r[k - 1] << (32 - 8 * s) : 0u) | (k < 16 ? r[k] >> (8 * s) : 0u);
    }
    sw[q + 16] |= 0x80000000u >> (8 * s);
}
template <int LL> constexpr u32 prf12_seed_len() { return (u32)LL + 2u * PRF12_RANDOM_LEN; }

// ---------------------------------------------------------------- the three HMACs of fixed shape
// the block counts of THE SHAPE, from the hashes' own block and length-field sizes: no label of 1 .. PRF12_LABEL_MAX bytes changes one
template <int HL> constexpr bool prf12_shapes_fixed() {
    return kdf_blocks<HL>(1u + 2u * PRF12_RANDOM_LEN) == kdf_blocks<HL>(PRF12_LABEL_MAX + 2u * PRF12_RANDOM_LEN) && kdf_blocks<HL>(HL) == 1u &&
           kdf_blocks<HL>(HL + 1u + 2u * PRF12_RANDOM_LEN) == 2u && kdf_blocks<HL>(HL + PRF12_LABEL_MAX + 2u * PRF12_RANDOM_LEN) == 2u;
}
static_assert(prf12_shapes_fixed<32>() && kdf_blocks<32>(PRF12_LABEL_MAX + 2u * PRF12_RANDOM_LEN) == 2u, "SHA-256: seed 2 blocks, A(j) 1, A(j) | seed 2");
static_assert(prf12_shapes_fixed<48>() && kdf_blocks<48>(PRF12_LABEL_MAX + 2u * PRF12_RANDOM_LEN) == 1u, "SHA-384: seed 1 block, A(j) 1, A(j) | seed 2");
static_assert(4u * PRF12_SEED_WORDS >= PRF12_LABEL_MAX + 2u * PRF12_RANDOM_LEN + 1u, "the longest seed and its 0x80");

// the ipad and the opad state of the 48-byte secret (ms: twelve big-endian words)
template <int HL> struct Prf12Key { typename KdfHash<HL>::word in[8], out[8]; };
template <int HL> HD void prf12_key(const u32 *ms, Prf12Key<HL> &k) {
    kdf_hmac_pad<HL, (int)PRF12_MASTER_LEN / 4>(ms, KDF_IPAD, k.in);
    kdf_hmac_pad<HL, (int)PRF12_MASTER_LEN / 4>(ms, KDF_OPAD, k.out);
}
// HMAC(secret, message): m = the message of len bytes with its KDF_PAD_BIT, NW big-endian words -> res, HL / 4 words
template <int HL, int NW> HD void prf12_hmac(const Prf12Key<HL> &k, const u32 *m, u32 len, u32 *res) {
    typename KdfHash<HL>::word st[8];
#pragma unroll
    for (int j = 0; j < 8; j++) st[j] = k.in[j];
    kdf_hmac_msg<HL, (int)kdf_blocks<HL>(4u * NW - 1u), NW>(st, m, len);                    // (4 NW - 1 bytes: the longest message whose 0x80 is in word NW - 1)
    kdf_hmac_outer<HL>(k.out, st, res);
}
// HMAC(secret, seed): sw from prf12_seed, SL = the seed's bytes
template <int HL> HD void prf12_hmac_seed(const Prf12Key<HL> &k, const u32 *sw, u32 SL, u32 *res) { prf12_hmac<HL, PRF12_SEED_WORDS>(k, sw, SL, res); }
// HMAC(secret, A): a = HL / 4 big-endian words
template <int HL> HD void prf12_hmac_a(const Prf12Key<HL> &k, const u32 *a, u32 *res) {
    u32 m[HL / 4 + 1];
#pragma unroll
    for (int j = 0; j < HL / 4; j++) m[j] = a[j];
    m[HL / 4] = KDF_PAD_BIT;
    prf12_hmac<HL, HL / 4 + 1>(k, m, (u32)HL, res);
}
// HMAC(secret, A | seed)
template <int HL> HD void prf12_hmac_a_seed(const Prf12Key<HL> &k, const u32 *a, const u32 *sw, u32 SL, u32 *res) {
    u32 m[HL / 4 + PRF12_SEED_WORDS];
#pragma unroll
    for (int j = 0; j < HL / 4 + PRF12_SEED_WORDS; j++) m[j] = j < HL / 4 ? a[j] : sw[j - HL / 4];
    prf12_hmac<HL, HL / 4 + PRF12_SEED_WORDS>(k, m, (u32)HL + SL, res);
}

// ---------------------------------------------------------------- P_hash, and what a lane takes of it
// the words of T(j + 1) (t: HL / 4 big-endian words, stream words j * HL / 4 ...) that fall into the window [first, first + N): out[k] = stream word first + k
template <int HL, int N> HD void prf12_pick(u32 j, const u32 *t, u32 first, u32 *out) {
    const u32 base = j * (u32)(HL / 4);
#pragma unroll
    for (int k = 0; k < N; k++)
#pragma unroll
        for (int m = 0; m < HL / 4; m++) out[k] = base + (u32)m == first + (u32)k ? t[m] : out[k];
}
// how many T(j) cover the stream's first n_words 32-bit words
template <int HL> HD u32 prf12_count(u32 n_words) { return (n_words + (u32)(HL / 4) - 1u) / (u32)(HL / 4); }
// P_hash(ms, label | r): take(j, t) sees T(j + 1) for j = 0 .. n_t - 1.  ms: the master secret as twelve big-endian words; r: the two randoms in the seed's order
template <int HL, int LL, class Take> HD void prf12_phash(const u32 *ms, const Prf12Label &label, const u32 *r, u32 n_t, Take take) {
    Prf12Key<HL> key;
    u32 sw[PRF12_SEED_WORDS], a[HL / 4], t[HL / 4];
    constexpr u32 SL = prf12_seed_len<LL>();
    prf12_key(ms, key);
    prf12_seed<LL>(label, r, sw);
    prf12_hmac_seed(key, sw, SL, a);                                   // A(1)
#pragma nounroll
    for (u32 j = 0; j < n_t; j++) {
        prf12_hmac_a_seed(key, a, sw, SL, t);                          // T(j + 1)
        take(j, t);
        if (j + 1u < n_t) {
            u32 next[HL / 4];
            prf12_hmac_a(key, a, next);                                // A(j + 2)
#pragma unroll
            for (int k = 0; k < HL / 4; k++) a[k] = next[k];
        }
    }
}

// ---------------------------------------------------------------- the table and what a lane decides
struct Prf12Table {
    u32 *rec;                              // n_masters records
    u32 *status;                           // lowest refused entry (atomic min, kdf_refuse), ~0 = none
    u32 n_masters, hash_len;
};
struct KtSlot;
struct Prf12InstallParams {
    Prf12Table t;
    Prf12Label label;                      // "key expansion"
    const u32 *idx;                        // n
    const u32 *slots[2];                   // by direction: n each, or NULL (not both)
    KtSlot *tab;
    u32 n, n_slots;
};
struct Prf12ExportParams {
    Prf12Table t;
    Prf12Label label;                      // "EXTRACTOR-dtls_srtp"
    const u32 *idx;
    const u32 *recs[2];                    // by direction: n each, or NULL (not both)
    SkdfTable m;                           // the SRTP master table (its status word is not touched); m.key_len 16 or 32
    u32 n;
};
struct Prf12SetParams {
    Prf12Table t;
    const u32 *idx;
    const unsigned char *masters, *client_randoms, *server_randoms;      // n * 48, n * 32, n * 32 bytes
    u32 n;
};

HD bool prf12_rec_set(const Prf12Table &t, u32 r) { return r < t.n_masters && t.rec[(size_t)r * PRF12_REC_WORDS + PRF12_REC_WORDS - 1u] == PRF12_SET; }
// a whole record from bytes at any address: the marker last.  The host's set packs its copy with it, the set kernel's lane stores with it
HD void prf12_store(const Prf12Table &t, u32 r, const unsigned char *master, const unsigned char *cr, const unsigned char *sr) {
    u32 *rec = t.rec + (size_t)r * PRF12_REC_WORDS;
    for (u32 k = 0; k < PRF12_REC_WORDS - 1u; k++) {
        const unsigned char *b = k < PRF12_CR_WORD ? master + 4u * k : k < PRF12_SR_WORD ? cr + 4u * (k - PRF12_CR_WORD) : sr + 4u * (k - PRF12_SR_WORD);
        rec[k] = k < PRF12_SR_WORD + PRF12_RANDOM_LEN / 4u ? (u32)b[0] | ((u32)b[1] << 8) | ((u32)b[2] << 16) | ((u32)b[3] << 24) : 0u;
    }
    rec[PRF12_REC_WORDS - 1u] = PRF12_SET;
}
// the record as big-endian words: the master secret, and the two randoms in the seed's order (server_first: key expansion; client first: the exporter)
HD void prf12_load(const Prf12Table &t, u32 r, bool server_first, u32 *ms, u32 *rnd) {
    const u32 *rec = t.rec + (size_t)r * PRF12_REC_WORDS;
    const u32 *first = rec + (server_first ? PRF12_SR_WORD : PRF12_CR_WORD), *second = rec + (server_first ? PRF12_CR_WORD : PRF12_SR_WORD);
#pragma unroll
    for (int k = 0; k < 12; k++) ms[k] = bswap32(rec[k]);
#pragma unroll
    for (int k = 0; k < 8; k++) { rnd[k] = bswap32(first[k]); rnd[8 + k] = bswap32(second[k]); }
}
// Entry i of an install or export call: every lane of the entry comes to the same verdict from the same words, so an entry is written whole or not at all.  The tests
// in this order: the record in range; the record set; the client's slot / record, where the call has that array and the entry names one, below n_dst; the server's
HD bool prf12_entry(const Prf12Table &t, const u32 *idx, const u32 *const *dst, u32 n_dst, u32 i, u32 &rec, u32 *d) {
    rec = idx[i];
    if (!prf12_rec_set(t, rec)) return false;
    d[PRF12_CLIENT] = dst[PRF12_CLIENT] ? dst[PRF12_CLIENT][i] : PRF12_NONE;
    if (d[PRF12_CLIENT] != PRF12_NONE && d[PRF12_CLIENT] >= n_dst) return false;
    d[PRF12_SERVER] = dst[PRF12_SERVER] ? dst[PRF12_SERVER][i] : PRF12_NONE;
    return d[PRF12_SERVER] == PRF12_NONE || d[PRF12_SERVER] < n_dst;
}

// key_block = client_write_key | server_write_key | client_write_IV[4] | server_write_IV[4] (RFC 5246 6.3, RFC 5288 3), as stream words: where a role's words start
HD u32 prf12_block_first(u32 role, u32 key_words) { return role < PRF12_ROLE_IV ? role * key_words : 2u * key_words + (role - PRF12_ROLE_IV); }
// What an install lane derives: out[0 .. NK - 1] = a key lane's key, out[0] = an IV lane's four bytes, as big-endian words.  Nothing is stored
template <int HL, int NK> HD void prf12_install_derive(const Prf12InstallParams &p, u32 rec, u32 role, u32 *out) {
    u32 ms[12], rnd[16];
    prf12_load(p.t, rec, true, ms, rnd);
    const u32 first = prf12_block_first(role, (u32)NK);
#pragma unroll
    for (int k = 0; k < NK; k++) out[k] = 0u;
    if (role < PRF12_ROLE_IV) {
        prf12_phash<HL, PRF12_LL_KEY_EXPANSION>(ms, p.label, rnd, prf12_count<HL>(first + (u32)NK), [&](u32 j, const u32 *t) { prf12_pick<HL, NK>(j, t, first, out); });
    } else {
        prf12_phash<HL, PRF12_LL_KEY_EXPANSION>(ms, p.label, rnd, prf12_count<HL>(first + 1u), [&](u32 j, const u32 *t) { prf12_pick<HL, 1>(j, t, first, out); });
    }
}
// out = client key | server key | client salt[12] | server salt[12] (RFC 5764 4.2 with the AEAD profiles' 12-byte salts, RFC 7714 12): what an export lane of
// direction dir derives -- key[0 .. 7] (zeros behind the key's words) and salt[0 .. 2], big-endian words
template <int HL> HD void prf12_export_derive(const Prf12ExportParams &p, u32 rec, u32 dir, u32 *key, u32 *salt) {
    u32 ms[12], rnd[16];
    prf12_load(p.t, rec, false, ms, rnd);
    const u32 kw = p.m.key_len / 4u, kfirst = dir * kw, sfirst = 2u * kw + 3u * dir;
#pragma unroll
    for (int k = 0; k < 8; k++) key[k] = 0u;
    salt[0] = salt[1] = salt[2] = 0u;
    prf12_phash<HL, PRF12_LL_EXPORTER>(ms, p.label, rnd, prf12_count<HL>(sfirst + 3u), [&](u32 j, const u32 *t) {
        prf12_pick<HL, 8>(j, t, kfirst, key);
        prf12_pick<HL, 3>(j, t, sfirst, salt);
    });
#pragma unroll
    for (int k = 0; k < 8; k++) key[k] = (u32)k < kw ? key[k] : 0u;         // a 16-byte key's window ran on into the next key: those words are not this record's
}
// skdf_store's twin for a key and a salt that lie in registers as big-endian words: record r of the SRTP master table becomes what aesgcm_srtp_kdf_set_dev makes of
// the key and of the 12-byte salt with two zero bytes appended; the marker last
HD void prf12_store_master(const SkdfTable &m, u32 r, const u32 *key, const u32 *salt) {
    u32 *rec = m.rec + (size_t)r * KDF_REC_WORDS;
#pragma unroll
    for (int k = 0; k < (int)KDF_REC_WORDS - 1; k++)
        rec[k] = k < 8 ? bswap32(key[k]) : (k >= (int)SKDF_SALT_WORD && k < (int)SKDF_SALT_WORD + 3) ? bswap32(salt[k - (int)SKDF_SALT_WORD]) : 0u;
    rec[KDF_REC_WORDS - 1u] = SKDF_SET;
}
HD void prf12_set_lane(const Prf12SetParams &p, u32 i) {
    const u32 r = p.idx[i];
    if (r >= p.t.n_masters) { kdf_refuse(p.t.status, i); return; }
    prf12_store(p.t, r, p.masters + (size_t)i * PRF12_MASTER_LEN, p.client_randoms + (size_t)i * PRF12_RANDOM_LEN, p.server_randoms + (size_t)i * PRF12_RANDOM_LEN);
}

// launchers (aesgcm_prf12_kernels.hip)
struct DevTables;
hipError_t klaunch_prf12_attributes();                                // hipFuncSetAttribute(MaxDynamicSharedMemorySize) of the install kernel's instances, on the current device
hipError_t klaunch_prf12_install(int nr, hipStream_t st, const DevTables *tb, const Prf12InstallParams &p);      // grid: entries x 4 roles
hipError_t klaunch_prf12_export(hipStream_t st, const Prf12ExportParams &p);                                      // grid: entries x 2 directions
hipError_t klaunch_prf12_set(hipStream_t st, const Prf12SetParams &p);
