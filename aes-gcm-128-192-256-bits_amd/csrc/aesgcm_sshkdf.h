// aesgcm_sshkdf.h -- SSH's key derivation on the device (aesgcm_sshkdf_*, include/aesgcm.h "SSH KEY DERIVATION"): a table of key-exchange outputs, and the AES-GCM
// keys and initial IVs of both directions by RFC 4253 7.2 over SHA-256 / SHA-384 / SHA-512, a lane per derived value.  Shared by the kernels
// (aesgcm_sshkdf_kernels.hip), the host side (aesgcm_sshkdf.hip) and the CPU harness tests/sshkdf_emul, which runs the same hash and the same verdicts against
// hashlib: everything a lane COMPUTES and DECIDES is here, HD.
//
// STATE.  n_recs records of rec_words 32-bit words, rec_words = SSHK_SID_WORDS + ceil(max_secret_len / 4) + 2, fixed at create: the session identifier's hash_len
// bytes as they are (words 0 .. 15, zeros behind them), the secret K_enc | H as the caller handed it over (zeros behind it), the secret's length in bytes, and in the
// LAST word SSHK_SET once the record holds a secret (zero = unset or cleared).  No call copies a record out.
//
// THE SHAPE.  RFC 4253 7.2: value = HASH(K | H | letter | session_id), a PLAIN hash and no HMAC -- there is no pad block and no outer hash.  The message is
// secret | letter | session_id: 1 .. 2048 bytes of secret, so -- as in aesgcm_prfplus.h -- the BLOCK COUNT IS A RUN-TIME VALUE: one loop over the blocks that is not
// unrolled, one compression in it (sshk_hash).  A message word that lies inside the secret is four byte loads at any address; the others take each byte by its place
// (sshk_msg_word): the secret's tail, the letter, the session identifier, the padding's 0x80, zero from there on; the last block's last word is the bit length.  No
// register array is indexed by a run-time value.  The compressions are aesgcm_kdf.h's (KdfHash<HL>), as they are.
// RFC 4253's extension K2 = HASH(K | H | K1) is needed where a value is longer than the digest.  The longest value here is an AES-256 key, 32 bytes, and the shortest
// digest SHA-256's 32: it is never needed and NOT BUILT.
//
// WHAT A LANE TAKES.  Letter 'A' / 'B': the initial IV client to server / server to client, the digest's first 12 bytes.  'C' / 'D': the encryption key of the same
// directions, the digest's first key_len bytes.  'E' / 'F' (integrity keys) have no use under AES-GCM.
#pragma once
#include "aesgcm_kdf.h"

#define SSHK_SID_WORDS 16u                 /* room for a SHA-512 session identifier */
#define SSHK_SET 0x4853534Bu               /* "KSSH": the record holds a secret */
#define SSHK_SECRET_MAX 2048u              /* the most that create takes for max_secret_len */
#define SSHK_NONE 0xFFFFFFFFu              /* an entry of a slot array that installs nothing for that direction */
#define SSHK_C2S 0u                        /* a direction: the index into SshkInstallParams::slots */
#define SSHK_S2C 1u
#define SSHK_ROLE_IV 0u                    /* blockIdx.y of the install kernel = 2 * role + direction = the letter behind 'A' */
#define SSHK_ROLE_KEY 1u

// ---------------------------------------------------------------- the hash whose block count is a run-time value
// Big-endian word j of secret | letter | session_id | 0x80 | zeros ...: s = len bytes at any address, sid = hl bytes.  No byte at or behind s + len or sid + hl is read
HD u32 sshk_msg_word(const unsigned char *s, u32 len, const unsigned char *sid, u32 hl, u32 letter, u32 j) {
    const u32 o = 4u * j;
    if (o < len && len - o >= 4u) return ((u32)s[o] << 24) | ((u32)s[o + 1u] << 16) | ((u32)s[o + 2u] << 8) | s[o + 3u];
    u32 w = 0u;
#pragma unroll
    for (u32 b = 0; b < 4u; b++) {
        const u32 q = o + b, r = q - len - 1u;             // r: the byte's place in the session identifier, where q is behind the letter
        w = (w << 8) | (q < len ? (u32)s[q] : q == len ? letter : r < hl ? (u32)sid[r] : r == hl ? 0x80u : 0u);
    }
    return w;
}
// how many blocks the message takes: the letter, the session identifier, the 0x80 and the length field go in with the secret
template <int HL> HD u32 sshk_blocks(u32 len) { return (len + 1u + (u32)HL + 1u + KdfHash<HL>::LEN_BYTES + KdfHash<HL>::BLOCK - 1u) / KdfHash<HL>::BLOCK; }
// out = HASH(s[0 .. len) | letter | sid[0 .. HL)) as HL / 4 big-endian words
template <int HL> HD void sshk_hash(const unsigned char *s, u32 len, const unsigned char *sid, u32 letter, u32 *out) {
    typedef KdfHash<HL> H;
    constexpr int WPB = (int)(H::BLOCK / 4u);                          // 32-bit message words per block
    typename H::word st[8];
    H::init(st);
    const u32 nb = sshk_blocks<HL>(len), bits = (len + 1u + (u32)HL) * 8u;
#pragma nounroll
    for (u32 b = 0; b < nb; b++) {
        u32 m[WPB];
#pragma unroll
        for (int k = 0; k < WPB; k++) m[k] = sshk_msg_word(s, len, sid, (u32)HL, letter, b * (u32)WPB + (u32)k);
        typename H::word w[16];
#pragma unroll
        for (int k = 0; k < 16; k++) w[k] = H::template at<WPB>(m, k);
        if (b + 1u == nb) w[15] = bits;
        H::block(st, w);
    }
    H::digest(st, out);
}

// ---------------------------------------------------------------- the table and what a lane decides
struct SshkTable {
    u32 *rec;                              // n_recs records
    u32 *status;                           // lowest refused entry (atomic min, kdf_refuse), ~0 = none
    u32 n_recs, hash_len, max_secret_len, rec_words;
};
struct KtSlot;
struct SshkInstallParams {
    SshkTable t;
    const u32 *idx;                        // n
    const u32 *slots[2];                   // by direction: n each, or NULL (not both)
    KtSlot *tab;
    u32 n, n_slots;
};
struct SshkSetParams {
    SshkTable t;
    const u32 *idx;
    const unsigned char *secrets;          // entry i's secret: bytes [secret_off[i], secret_off[i + 1])
    const u32 *secret_off;                 // n + 1
    const unsigned char *sids;             // n * hash_len bytes
    u32 n;
};

HD u32 sshk_rec_words(u32 max_secret_len) { return SSHK_SID_WORDS + (max_secret_len + 3u) / 4u + 2u; }
HD bool sshk_rec_set(const SshkTable &t, u32 r) { return r < t.n_recs && t.rec[(size_t)r * t.rec_words + t.rec_words - 1u] == SSHK_SET; }
// a record's parts for a lane that hashes: the secret's bytes and length, the session identifier's bytes
HD void sshk_load(const SshkTable &t, u32 r, const unsigned char *&s, u32 &len, const unsigned char *&sid) {
    const u32 *rec = t.rec + (size_t)r * t.rec_words;
    sid = (const unsigned char *)rec;
    s = (const unsigned char *)(rec + SSHK_SID_WORDS);
    len = rec[t.rec_words - 2u];
    if (len > t.max_secret_len) len = t.max_secret_len;                 // (never: both setters test it; no lane reads past its record whatever the word holds)
}
// a whole record from bytes at any address (1 <= len <= max_secret_len: the caller's test): the marker last.  The host's set packs its copy with it, the set kernel's
// lane stores with it.  No byte at or behind secret + len or sid + hash_len is read
HD void sshk_store(const SshkTable &t, u32 r, const unsigned char *secret, u32 len, const unsigned char *sid) {
    u32 *rec = t.rec + (size_t)r * t.rec_words;
    for (u32 k = 0; k < t.rec_words - 2u; k++) {
        const bool of_sid = k < SSHK_SID_WORDS;
        const unsigned char *src = of_sid ? sid : secret;
        const u32 o = 4u * (of_sid ? k : k - SSHK_SID_WORDS), n = of_sid ? t.hash_len : len;
        u32 w = 0u;
        for (u32 b = 0; b < 4u; b++) if (o + b < n) w |= (u32)src[o + b] << (8u * b);
        rec[k] = w;
    }
    rec[t.rec_words - 2u] = len;
    rec[t.rec_words - 1u] = SSHK_SET;
}
// Entry i of an install call: every lane of the entry (one per letter) comes to the same verdict from the same words, so an entry is written whole or not at all.
// The tests in this order: the record in range; the record set; the client-to-server slot, where the call has that array and the entry names one, below n_slots;
// the server-to-client slot
HD bool sshk_entry(const SshkInstallParams &p, u32 i, u32 &rec, u32 *slot) {
    rec = p.idx[i];
    if (!sshk_rec_set(p.t, rec)) return false;
    slot[SSHK_C2S] = p.slots[SSHK_C2S] ? p.slots[SSHK_C2S][i] : SSHK_NONE;
    if (slot[SSHK_C2S] != SSHK_NONE && slot[SSHK_C2S] >= p.n_slots) return false;
    slot[SSHK_S2C] = p.slots[SSHK_S2C] ? p.slots[SSHK_S2C][i] : SSHK_NONE;
    return slot[SSHK_S2C] == SSHK_NONE || slot[SSHK_S2C] < p.n_slots;
}
// What the lane of (role, dir) derives: out = the digest of the record's message under its letter, HL / 4 big-endian words; the IV is its first 3, the key its first
// key_len / 4.  Nothing is stored
template <int HL> HD void sshk_derive(const SshkTable &t, u32 rec, u32 role, u32 dir, u32 *out) {
    const unsigned char *s, *sid;
    u32 len;
    sshk_load(t, rec, s, len, sid);
    sshk_hash<HL>(s, len, sid, (u32)'A' + 2u * role + dir, out);
}
// Entry i of a set_dev call.  Refused: the record out of range; the secret's offsets falling, the secret empty or longer than max_secret_len
HD void sshk_set_lane(const SshkSetParams &p, u32 i) {
    const u32 r = p.idx[i], from = p.secret_off[i], to = p.secret_off[i + 1u];
    if (r >= p.t.n_recs || to <= from || to - from > p.t.max_secret_len) { kdf_refuse(p.t.status, i); return; }
    sshk_store(p.t, r, p.secrets + from, to - from, p.sids + (size_t)i * p.t.hash_len);
}

// launchers (aesgcm_sshkdf_kernels.hip)
struct DevTables;
hipError_t klaunch_sshk_attributes();                                 // hipFuncSetAttribute(MaxDynamicSharedMemorySize) of the install kernel's instances, on the current device
hipError_t klaunch_sshk_install(int nr, hipStream_t st, const DevTables *tb, const SshkInstallParams &p);      // grid: entries x 4 letters
hipError_t klaunch_sshk_set(hipStream_t st, const SshkSetParams &p);
