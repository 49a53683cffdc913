// aesgcm_kdf.h -- on-device key derivation (aesgcm_kdf_*, include/aesgcm.h "ON-DEVICE KEY DERIVATION"): a table of traffic secrets and HKDF-Expand-Label over
// HMAC-SHA-256 / HMAC-SHA-384, a lane per derived value.  Shared by the kernels (aesgcm_kdf_kernels.hip), the host side (aesgcm_kdf.hip) and the CPU harness
// tests/kdf_emul, which runs the same compressions and the same expansion against hashlib and hmac: everything a lane COMPUTES and DECIDES is here, HD.
//
// STATE.  n_secrets records of KDF_REC_WORDS 32-bit words (64 bytes): the secret's hash_len bytes as they are (words 0 .. 7 or 0 .. 11), zeros, and in the last word
// KDF_SET once the record holds a secret (zero = unset or cleared).  No call copies a record out of the table.
//
// THE ONE CASE.  HKDF-Expand-Label(secret, label, "", L) with L <= hash_len is T(1) = HMAC(secret, HkdfLabel | 0x01), HkdfLabel = be16(L) | len | label | 0x00
// (RFC 8446 7.1, RFC 5869 2.3).  With a full label of at most KDF_LABEL_MAX = 20 bytes the message is at most 25 bytes, and the key (the secret: hash_len bytes) is at
// most one block.  So EVERY HMAC HERE IS EXACTLY FOUR COMPRESSIONS: the ipad block, one message block (message | 0x80 | zeros | bit length), the opad block, one
// digest block (kdf_hmac_pad, kdf_hmac_msg, kdf_hmac_outer: each shape written once, over KdfHash<HL>; aesgcm_prf12.h builds its HMACs from the same three).  There is no multi-block and no multi-T(i) path; aesgcm_kdf_fmt_check holds the labels to the bound, the kernels do not look at it again.  The message
// block's first 32 bytes are made on the HOST (kdf_msg: a KdfMsg per label, passed by value), so no lane indexes its message schedule by a length.
//
// The rounds are fully unrolled (by template recursion) over a 16-word rolling schedule with constant indices (registers, no private memory); rotates are funnel shifts (v_alignbit_b32; a 64-bit
// rotate is two); the round constants lie in __constant__ memory, their index uniform once unrolled.
#pragma once
#include "aesgcm_base.h"
#include "../../include/aesgcm.h"

#define KDF_REC_WORDS 16u
#define KDF_SET 0x5345444Bu                /* "KDES": the record holds a secret */
#define KDF_LABEL_MAX 20u
#define KDF_WG 256u
#define KDF_ROLE_KEY 0u                    /* blockIdx.y of k_kdf_install = the label's index in aesgcm_kdf_fmt: uniform per workgroup */
#define KDF_ROLE_IV 1u
#define KDF_ROLE_AUX 2u
#define KDF_LABEL_UPDATE 3u
#define KDF_NO_SLOT 0xFFFFFFFFu

#if defined(__HIP_DEVICE_COMPILE__)
#define KDF_CONST __constant__
#else
#define KDF_CONST
#endif
// FIPS 180-4 4.2.2 / 4.2.3: the fractional parts of the cube roots of the first 64 / 80 primes
static KDF_CONST const u32 kdf_k256[64] = {
    0x428a2f98u, 0x71374491u, 0xb5c0fbcfu, 0xe9b5dba5u, 0x3956c25bu, 0x59f111f1u, 0x923f82a4u, 0xab1c5ed5u,
    0xd807aa98u, 0x12835b01u, 0x243185beu, 0x550c7dc3u, 0x72be5d74u, 0x80deb1feu, 0x9bdc06a7u, 0xc19bf174u,
    0xe49b69c1u, 0xefbe4786u, 0x0fc19dc6u, 0x240ca1ccu, 0x2de92c6fu, 0x4a7484aau, 0x5cb0a9dcu, 0x76f988dau,
    0x983e5152u, 0xa831c66du, 0xb00327c8u, 0xbf597fc7u, 0xc6e00bf3u, 0xd5a79147u, 0x06ca6351u, 0x14292967u,
    0x27b70a85u, 0x2e1b2138u, 0x4d2c6dfcu, 0x53380d13u, 0x650a7354u, 0x766a0abbu, 0x81c2c92eu, 0x92722c85u,
    0xa2bfe8a1u, 0xa81a664bu, 0xc24b8b70u, 0xc76c51a3u, 0xd192e819u, 0xd6990624u, 0xf40e3585u, 0x106aa070u,
    0x19a4c116u, 0x1e376c08u, 0x2748774cu, 0x34b0bcb5u, 0x391c0cb3u, 0x4ed8aa4au, 0x5b9cca4fu, 0x682e6ff3u,
    0x748f82eeu, 0x78a5636fu, 0x84c87814u, 0x8cc70208u, 0x90befffau, 0xa4506cebu, 0xbef9a3f7u, 0xc67178f2u,
};
static KDF_CONST const u64 kdf_k512[80] = {
    0x428a2f98d728ae22ull, 0x7137449123ef65cdull, 0xb5c0fbcfec4d3b2full, 0xe9b5dba58189dbbcull,
    0x3956c25bf348b538ull, 0x59f111f1b605d019ull, 0x923f82a4af194f9bull, 0xab1c5ed5da6d8118ull,
    0xd807aa98a3030242ull, 0x12835b0145706fbeull, 0x243185be4ee4b28cull, 0x550c7dc3d5ffb4e2ull,
    0x72be5d74f27b896full, 0x80deb1fe3b1696b1ull, 0x9bdc06a725c71235ull, 0xc19bf174cf692694ull,
    0xe49b69c19ef14ad2ull, 0xefbe4786384f25e3ull, 0x0fc19dc68b8cd5b5ull, 0x240ca1cc77ac9c65ull,
    0x2de92c6f592b0275ull, 0x4a7484aa6ea6e483ull, 0x5cb0a9dcbd41fbd4ull, 0x76f988da831153b5ull,
    0x983e5152ee66dfabull, 0xa831c66d2db43210ull, 0xb00327c898fb213full, 0xbf597fc7beef0ee4ull,
    0xc6e00bf33da88fc2ull, 0xd5a79147930aa725ull, 0x06ca6351e003826full, 0x142929670a0e6e70ull,
    0x27b70a8546d22ffcull, 0x2e1b21385c26c926ull, 0x4d2c6dfc5ac42aedull, 0x53380d139d95b3dfull,
    0x650a73548baf63deull, 0x766a0abb3c77b2a8ull, 0x81c2c92e47edaee6ull, 0x92722c851482353bull,
    0xa2bfe8a14cf10364ull, 0xa81a664bbc423001ull, 0xc24b8b70d0f89791ull, 0xc76c51a30654be30ull,
    0xd192e819d6ef5218ull, 0xd69906245565a910ull, 0xf40e35855771202aull, 0x106aa07032bbd1b8ull,
    0x19a4c116b8d2d0c8ull, 0x1e376c085141ab53ull, 0x2748774cdf8eeb99ull, 0x34b0bcb5e19b48a8ull,
    0x391c0cb3c5c95a63ull, 0x4ed8aa4ae3418acbull, 0x5b9cca4f7763e373ull, 0x682e6ff3d6b2b8a3ull,
    0x748f82ee5defb2fcull, 0x78a5636f43172f60ull, 0x84c87814a1f0ab72ull, 0x8cc702081a6439ecull,
    0x90befffa23631e28ull, 0xa4506cebde82bde9ull, 0xbef9a3f7b2c67915ull, 0xc67178f2e372532bull,
    0xca273eceea26619cull, 0xd186b8c721c0c207ull, 0xeada7dd6cde0eb1eull, 0xf57d4f7fee6ed178ull,
    0x06f067aa72176fbaull, 0x0a637dc5a2c898a6ull, 0x113f9804bef90daeull, 0x1b710b35131c471bull,
    0x28db77f523047d84ull, 0x32caab7b40c72493ull, 0x3c9ebe0a15c9bebcull, 0x431d67c49c100d4cull,
    0x4cc5d4becb3e42b6ull, 0x597f299cfc657e2aull, 0x5fcb6fab3ad6faecull, 0x6c44198c4a475817ull,
};

// ---------------------------------------------------------------- the compressions
// rotate right by a constant 0 < n < 32 (64-bit: 0 < n < 64, n != 32)
HD u32 kdf_rotr32(u32 x, u32 n) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_alignbit(x, x, n);
#else
    return (x >> n) | (x << (32u - n));
#endif
}
HD u64 kdf_rotr64(u64 x, u32 n) {
#if defined(__HIP_DEVICE_COMPILE__)
    const u32 lo = n < 32u ? (u32)x : (u32)(x >> 32), hi = n < 32u ? (u32)(x >> 32) : (u32)x, m = n & 31u;      // n >= 32: the halves swap first
    return ((u64)__builtin_amdgcn_alignbit(lo, hi, m) << 32) | __builtin_amdgcn_alignbit(hi, lo, m);
#else
    return (x >> n) | (x << (64u - n));
#endif
}

// One round with the compile-time index I: the schedule word w[I & 15] (rolling, from round 16 on), then d += T1, h = T1 + T2 in place -- the caller turns the
// eight working variables by passing them one place on (KDF_ROUNDS8), so nothing is moved.  The rounds are unrolled by template recursion and not by a loop
// pragma: at 80 rounds of 64-bit words the compiler's unroller gives up and indexes the schedule by a register.
template <int I> HD void kdf_round256(u32 a, u32 b, u32 c, u32 &d, u32 e, u32 f, u32 g, u32 &h, u32 *w) {
    if constexpr (I >= 16) {
        const u32 x = w[(I - 15) & 15], y = w[(I - 2) & 15];
        w[I & 15] += (kdf_rotr32(x, 7) ^ kdf_rotr32(x, 18) ^ (x >> 3)) + w[(I - 7) & 15] + (kdf_rotr32(y, 17) ^ kdf_rotr32(y, 19) ^ (y >> 10));
    }
    const u32 t1 = h + (kdf_rotr32(e, 6) ^ kdf_rotr32(e, 11) ^ kdf_rotr32(e, 25)) + (g ^ (e & (f ^ g))) + kdf_k256[I] + w[I & 15];
    const u32 t2 = (kdf_rotr32(a, 2) ^ kdf_rotr32(a, 13) ^ kdf_rotr32(a, 22)) + ((a & b) | (c & (a | b)));
    d += t1; h = t1 + t2;
}
template <int I> HD void kdf_round512(u64 a, u64 b, u64 c, u64 &d, u64 e, u64 f, u64 g, u64 &h, u64 *w) {
    if constexpr (I >= 16) {
        const u64 x = w[(I - 15) & 15], y = w[(I - 2) & 15];
        w[I & 15] += (kdf_rotr64(x, 1) ^ kdf_rotr64(x, 8) ^ (x >> 7)) + w[(I - 7) & 15] + (kdf_rotr64(y, 19) ^ kdf_rotr64(y, 61) ^ (y >> 6));
    }
    const u64 t1 = h + (kdf_rotr64(e, 14) ^ kdf_rotr64(e, 18) ^ kdf_rotr64(e, 41)) + (g ^ (e & (f ^ g))) + kdf_k512[I] + w[I & 15];
    const u64 t2 = (kdf_rotr64(a, 28) ^ kdf_rotr64(a, 34) ^ kdf_rotr64(a, 39)) + ((a & b) | (c & (a | b)));
    d += t1; h = t1 + t2;
}
#define KDF_ROUNDS8(R, I) \
    R<I>(a, b, c, d, e, f, g, h, w); R<I + 1>(h, a, b, c, d, e, f, g, w); R<I + 2>(g, h, a, b, c, d, e, f, w); R<I + 3>(f, g, h, a, b, c, d, e, w); \
    R<I + 4>(e, f, g, h, a, b, c, d, w); R<I + 5>(d, e, f, g, h, a, b, c, w); R<I + 6>(c, d, e, f, g, h, a, b, w); R<I + 7>(b, c, d, e, f, g, h, a, w);
template <int I> HD void kdf_rounds256(u32 &a, u32 &b, u32 &c, u32 &d, u32 &e, u32 &f, u32 &g, u32 &h, u32 *w) {
    KDF_ROUNDS8(kdf_round256, I)
    if constexpr (I + 8 < 64) kdf_rounds256<I + 8>(a, b, c, d, e, f, g, h, w);
}
template <int I> HD void kdf_rounds512(u64 &a, u64 &b, u64 &c, u64 &d, u64 &e, u64 &f, u64 &g, u64 &h, u64 *w) {
    KDF_ROUNDS8(kdf_round512, I)
    if constexpr (I + 8 < 80) kdf_rounds512<I + 8>(a, b, c, d, e, f, g, h, w);
}
// st: the eight state words; w: the block as sixteen big-endian words, overwritten by the rolling schedule
HD void kdf_sha256_block(u32 *st, u32 *w) {
    u32 a = st[0], b = st[1], c = st[2], d = st[3], e = st[4], f = st[5], g = st[6], h = st[7];
    kdf_rounds256<0>(a, b, c, d, e, f, g, h, w);
    st[0] += a; st[1] += b; st[2] += c; st[3] += d; st[4] += e; st[5] += f; st[6] += g; st[7] += h;
}
HD void kdf_sha512_block(u64 *st, u64 *w) {
    u64 a = st[0], b = st[1], c = st[2], d = st[3], e = st[4], f = st[5], g = st[6], h = st[7];
    kdf_rounds512<0>(a, b, c, d, e, f, g, h, w);
    st[0] += a; st[1] += b; st[2] += c; st[3] += d; st[4] += e; st[5] += f; st[6] += g; st[7] += h;
}
// FIPS 180-4 5.3.3 / 5.3.4
HD void kdf_sha256_init(u32 *st) {
    st[0] = 0x6a09e667u; st[1] = 0xbb67ae85u; st[2] = 0x3c6ef372u; st[3] = 0xa54ff53au; st[4] = 0x510e527fu; st[5] = 0x9b05688cu; st[6] = 0x1f83d9abu; st[7] = 0x5be0cd19u;
}
HD void kdf_sha384_init(u64 *st) {
    st[0] = 0xcbbb9d5dc1059ed8ull; st[1] = 0x629a292a367cd507ull; st[2] = 0x9159015a3070dd17ull; st[3] = 0x152fecd8f70e5939ull;
    st[4] = 0x67332667ffc00b31ull; st[5] = 0x8eb44a8768581511ull; st[6] = 0xdb0c2e0d64f98fa7ull; st[7] = 0x47b5481dbefa4fa4ull;
}
HD void kdf_sha512_init(u64 *st) {
    st[0] = 0x6a09e667f3bcc908ull; st[1] = 0xbb67ae8584caa73bull; st[2] = 0x3c6ef372fe94f82bull; st[3] = 0xa54ff53a5f1d36f1ull;
    st[4] = 0x510e527fade682d1ull; st[5] = 0x9b05688c2b3e6c1full; st[6] = 0x1f83d9abfb41bd6bull; st[7] = 0x5be0cd19137e2179ull;
}

// ---------------------------------------------------------------- the hashes by digest length, and the shapes of an HMAC
// HL = 32: SHA-256, HL = 48: SHA-384, HL = 64: SHA-512 (aesgcm_prfplus.h only: SHA-384's compression from its own initial state, all eight state words out).  A message is handed over as big-endian 32-bit words (NW of them, zeros behind); at(m, k) is word k of the block's sixteen
// in the state's width: m[k] itself, or m[2k] | m[2k + 1].  A block is BLOCK bytes and ends with the message's bit length in LEN_BYTES bytes, of which all but the
// low word -- w[15] in either width -- are zero here; the padding's 0x80 is KDF_PAD_BIT in the 32-bit word behind the message's last
template <int HL> struct KdfHash;
template <> struct KdfHash<32> {
    typedef u32 word;
    static constexpr u32 BLOCK = 64u, LEN_BYTES = 8u;
    static HD void init(word *st) { kdf_sha256_init(st); }
    static HD void block(word *st, word *w) { kdf_sha256_block(st, w); }
    template <int NW> static HD word at(const u32 *m, int k) { return k < NW ? m[k] : 0u; }
    static HD void digest(const word *st, u32 *out) {
#pragma unroll
        for (int k = 0; k < 8; k++) out[k] = st[k];
    }
};
template <> struct KdfHash<48> {
    typedef u64 word;
    static constexpr u32 BLOCK = 128u, LEN_BYTES = 16u;
    static HD void init(word *st) { kdf_sha384_init(st); }
    static HD void block(word *st, word *w) { kdf_sha512_block(st, w); }
    template <int NW> static HD word at(const u32 *m, int k) { return ((u64)(2 * k < NW ? m[2 * k] : 0u) << 32) | (2 * k + 1 < NW ? m[2 * k + 1] : 0u); }
    static HD void digest(const word *st, u32 *out) {
#pragma unroll
        for (int k = 0; k < 6; k++) { out[2 * k] = (u32)(st[k] >> 32); out[2 * k + 1] = (u32)st[k]; }
    }
};
template <> struct KdfHash<64> {
    typedef u64 word;
    static constexpr u32 BLOCK = 128u, LEN_BYTES = 16u;
    static HD void init(word *st) { kdf_sha512_init(st); }
    static HD void block(word *st, word *w) { kdf_sha512_block(st, w); }
    template <int NW> static HD word at(const u32 *m, int k) { return KdfHash<48>::at<NW>(m, k); }
    static HD void digest(const word *st, u32 *out) {
#pragma unroll
        for (int k = 0; k < 8; k++) { out[2 * k] = (u32)(st[k] >> 32); out[2 * k + 1] = (u32)st[k]; }
    }
};
#define KDF_IPAD 0x3636363636363636ull     /* RFC 2104; cut to the state's width */
#define KDF_OPAD 0x5c5c5c5c5c5c5c5cull
#define KDF_PAD_BIT 0x80000000u
// how many blocks a message of len bytes takes behind whole blocks: the 0x80 and the length field go in with it
template <int HL> constexpr u32 kdf_blocks(u32 len) { return (len + 1u + KdfHash<HL>::LEN_BYTES + KdfHash<HL>::BLOCK - 1u) / KdfHash<HL>::BLOCK; }

// st = the state behind the pad block of a key of KW 32-bit words (at most one block): one compression from init; pad = KDF_IPAD or KDF_OPAD
template <int HL, int KW> HD void kdf_hmac_pad(const u32 *key, u64 pad, typename KdfHash<HL>::word *st) {
    typedef KdfHash<HL> H;
    static_assert(4u * KW <= H::BLOCK, "a longer key would have to be hashed first");
    typename H::word w[16];
#pragma unroll
    for (int k = 0; k < 16; k++) w[k] = H::template at<KW>(key, k) ^ (typename H::word)pad;
    H::init(st);
    H::block(st, w);
}
// st, which stands behind ONE block (a pad state), takes the NB blocks of a message of len bytes: m = the message with its KDF_PAD_BIT, NW words.  Block B of NB, by
// recursion: every index is a constant
template <int HL, int NB, int NW, int B = 0> HD void kdf_hmac_msg(typename KdfHash<HL>::word *st, const u32 *m, u32 len) {
    typedef KdfHash<HL> H;
    static_assert(4u * NW + H::LEN_BYTES <= NB * H::BLOCK, "the message and its 0x80 must end before the length field of block NB");
    typename H::word w[16];
#pragma unroll
    for (int k = 0; k < 16; k++) w[k] = H::template at<NW>(m, 16 * B + k);
    if constexpr (B + 1 == NB) w[15] = (H::BLOCK + len) * 8u;
    H::block(st, w);
    if constexpr (B + 1 < NB) kdf_hmac_msg<HL, NB, NW, B + 1>(st, m, len);
}
// the outer hash: opad = the opad state, in = the inner hash's final state -> res, the HMAC as HL / 4 big-endian 32-bit words
template <int HL> HD void kdf_hmac_outer(const typename KdfHash<HL>::word *opad, const typename KdfHash<HL>::word *in, u32 *res) {
    typename KdfHash<HL>::word o[8];
    u32 d[HL / 4 + 1];
#pragma unroll
    for (int k = 0; k < 8; k++) o[k] = opad[k];
    KdfHash<HL>::digest(in, d);
    d[HL / 4] = KDF_PAD_BIT;
    kdf_hmac_msg<HL, 1, HL / 4 + 1>(o, d, (u32)HL);
    KdfHash<HL>::digest(o, res);
}

// ---------------------------------------------------------------- HKDF-Expand-Label, the one case
// The message of the HMAC, HkdfLabel | 0x01, with the padding's 0x80 behind it, as eight big-endian words, and its length.  Made on the host from a full label of at
// most KDF_LABEL_MAX bytes (len <= 25: the 0x80 is byte 25 at the latest, inside the 32)
struct KdfMsg { u32 w[8]; u32 len; };
HD void kdf_msg(const unsigned char *label, u32 label_len, u32 L, KdfMsg &m) {
    unsigned char b[32] = {0};
    if (label_len > KDF_LABEL_MAX) label_len = KDF_LABEL_MAX;          // (never: aesgcm_kdf_fmt_check)
    b[0] = (unsigned char)(L >> 8); b[1] = (unsigned char)L; b[2] = (unsigned char)label_len;
    for (u32 k = 0; k < label_len; k++) b[3 + k] = label[k];
    m.len = label_len + 5u;                      // be16(L) | len | label | 0x00 (no context) | 0x01 (the counter of T(1))
    b[m.len - 1u] = 0x01; b[m.len] = 0x80;
    for (u32 k = 0; k < 8u; k++) m.w[k] = ((u32)b[4 * k] << 24) | ((u32)b[4 * k + 1] << 16) | ((u32)b[4 * k + 2] << 8) | b[4 * k + 3];
}

// sec: the secret as HL / 4 big-endian 32-bit words -> out: T(1), HL / 4 big-endian 32-bit words, of which the caller takes the first L bytes.  The compressions in
// this order -- ipad, message, opad, digest -- so that only the inner digest is live across the opad block
template <int HL> HD void kdf_expand(const u32 *sec, const KdfMsg &m, u32 *out) {
    typename KdfHash<HL>::word st[8], in[8];
    kdf_hmac_pad<HL, HL / 4>(sec, KDF_IPAD, st);
    kdf_hmac_msg<HL, 1, 8>(st, m.w, m.len);
#pragma unroll
    for (int k = 0; k < 8; k++) in[k] = st[k];
    kdf_hmac_pad<HL, HL / 4>(sec, KDF_OPAD, st);
    kdf_hmac_outer<HL>(st, in, out);
}

// ---------------------------------------------------------------- the table and what a lane decides
struct KdfTable {
    u32 *rec;                              // n_secrets records
    u32 *status;                           // lowest refused entry (atomic min), ~0 = none
    u32 n_secrets, hash_len;
};
struct KtSlot;
struct KdfInstallParams {
    KdfTable t;
    KdfMsg msg[3];                         // by role: key (L = key_len), iv (L = 12), aux (L = key_len)
    const u32 *idx, *slots, *aux_slots;    // n each; aux_slots or NULL (then the grid has no aux row)
    KtSlot *tab;
    u32 n, n_slots;
};
struct KdfUpdateParams {
    KdfTable t;
    KdfMsg msg;                            // L = hash_len
    const u32 *from, *to;
    u32 n;
};
struct KdfSetParams {
    KdfTable t;
    const u32 *idx;
    const unsigned char *secrets;          // n * hash_len bytes
    u32 n;
};

HD void kdf_refuse(u32 *status, u32 i) {
#if defined(__HIP_DEVICE_COMPILE__)
    atomicMin(status, i);
#else
    if (i < *status) *status = i;
#endif
}
HD bool kdf_rec_set(const KdfTable &t, u32 r) { return r < t.n_secrets && t.rec[(size_t)r * KDF_REC_WORDS + KDF_REC_WORDS - 1u] == KDF_SET; }
// the record's secret as big-endian words
template <int HL> HD void kdf_load(const KdfTable &t, u32 r, u32 *sec) {
    const u32 *rec = t.rec + (size_t)r * KDF_REC_WORDS;
#pragma unroll
    for (int k = 0; k < HL / 4; k++) sec[k] = bswap32(rec[k]);
}
// ... and a whole record from big-endian words: the marker last
template <int HL> HD void kdf_store(const KdfTable &t, u32 r, const u32 *sec) {
    u32 *rec = t.rec + (size_t)r * KDF_REC_WORDS;
#pragma unroll
    for (int k = 0; k < (int)KDF_REC_WORDS - 1; k++) rec[k] = k < HL / 4 ? bswap32(sec[k]) : 0u;
    rec[KDF_REC_WORDS - 1u] = KDF_SET;
}
// Entry i of an install call: every lane of the entry (one per role) comes to the same verdict from the same words, so an entry is installed whole or not at all.
// The tests in this order: the record in range; the record set; the slot in range; the aux slot, where the call has them and the entry names one, in range
HD bool kdf_install_entry(const KdfInstallParams &p, u32 i, u32 &rec, u32 &slot, u32 &aux) {
    rec = p.idx[i];
    if (!kdf_rec_set(p.t, rec)) return false;
    slot = p.slots[i];
    if (slot >= p.n_slots) return false;
    aux = p.aux_slots ? p.aux_slots[i] : KDF_NO_SLOT;
    return aux == KDF_NO_SLOT || aux < p.n_slots;
}
// Entry i of an update call: both records in range, the source set.  The lane holds the whole source secret in registers before it stores (to == from is in place)
template <int HL> HD void kdf_update_lane(const KdfUpdateParams &p, u32 i) {
    const u32 from = p.from[i], to = p.to[i];
    if (to >= p.t.n_secrets || !kdf_rec_set(p.t, from)) { kdf_refuse(p.t.status, i); return; }
    u32 sec[HL / 4], out[HL / 4];
    kdf_load<HL>(p.t, from, sec);
    kdf_expand<HL>(sec, p.msg, out);
    kdf_store<HL>(p.t, to, out);
}
HD void kdf_set_lane(const KdfSetParams &p, u32 i) {
    const u32 r = p.idx[i];
    if (r >= p.t.n_secrets) { kdf_refuse(p.t.status, i); return; }
    const unsigned char *s = p.secrets + (size_t)i * p.t.hash_len;
    u32 *rec = p.t.rec + (size_t)r * KDF_REC_WORDS;
    for (u32 k = 0; k < KDF_REC_WORDS - 1u; k++) {
        const unsigned char *b = s + 4u * k;                                  // (bytes: d_secrets has no alignment to keep)
        rec[k] = 4u * k < p.t.hash_len ? (u32)b[0] | ((u32)b[1] << 8) | ((u32)b[2] << 16) | ((u32)b[3] << 24) : 0u;
    }
    rec[KDF_REC_WORDS - 1u] = KDF_SET;
}

// launchers (aesgcm_kdf_kernels.hip)
struct DevTables;
hipError_t klaunch_kdf_attributes();                                  // hipFuncSetAttribute(MaxDynamicSharedMemorySize) of k_kdf_install's instances, on the current device
hipError_t klaunch_kdf_install(int nr, hipStream_t st, const DevTables *tb, const KdfInstallParams &p);      // grid: entries x (2 or 3 roles)
hipError_t klaunch_kdf_update(hipStream_t st, const KdfUpdateParams &p);
hipError_t klaunch_kdf_set(hipStream_t st, const KdfSetParams &p);
