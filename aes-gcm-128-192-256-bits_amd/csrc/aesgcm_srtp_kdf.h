// aesgcm_srtp_kdf.h -- SRTP / SRTCP session keys derived on the device (aesgcm_srtp_kdf_*, include/aesgcm.h "SRTP KEY DERIVATION"): a table of master keys and salts and
// the AES-CM PRF of RFC 3711 4.3.1 (RFC 6188 for AES-192 / AES-256 master keys), a lane per derived value.  Shared by the kernels (aesgcm_srtp_kdf_kernels.hip), the
// host side (aesgcm_srtp_kdf.hip) and the CPU harness tests/srtp_kdf_emul, which runs the same schedule and the same blocks against an independent AES: everything a lane
// COMPUTES and DECIDES is here, HD.
//
// STATE.  n_masters records of KDF_REC_WORDS 32-bit words (64 bytes, as aesgcm_kdf.h): the master key's key_len bytes as they are (words 0 .. 7), the 14-byte master
// salt in bytes 32 .. 45 (words 8 .. 11, the upper half of word 11 zero), zeros, and in the last word SKDF_SET once the record holds a master (zero = unset or
// cleared).  No call copies a record out of the table.
//
// THE PRF.  x = salt XOR (0^56 | label | be48(r)), 14 bytes: the label in byte 7, r = index DIV key_derivation_rate in bytes 8 .. 13.  The output is
// E_mk(x | be16(0)) | E_mk(x | be16(1)) | ..., of which a session key takes key_len bytes (two blocks for AES-192 / AES-256) and a session salt the first 12 (what the
// slot's TLS-IV field holds).  An AEAD profile's 12-byte master salt enters with two zero bytes appended (the caller's padding: the ABI takes 14 bytes always).
// Blocks and keys are memory-order words throughout (aesgcm_base.h), so the PRF's output words ARE the session key's words: no byte swap between PRF and schedule.
#pragma once
#include "aesgcm_kdf_slot.h"
#include "aesgcm_kdf.h"

#define SKDF_SET 0x5345444Du               /* "MDES": the record holds a master key and salt */
#define SKDF_SALT_WORD 8u                  /* the salt's first word in a record */
#define SKDF_SALT_LEN 14u
#define SKDF_ROLE_KEY 0u                   /* blockIdx.y of the install kernel: uniform per workgroup */
#define SKDF_ROLE_SALT 1u
#define SKDF_R_END (1ull << 48)            /* r is 48 bits */

struct SkdfTable {
    u32 *rec;                              // n_masters records
    u32 *status;                           // lowest refused entry (atomic min, kdf_refuse), ~0 = none
    u32 n_masters, key_len;
};
// a table's records for the units that fill them without going through aesgcm_srtp_kdf_set* (aesgcm_prf12.hip: the DTLS-SRTP exporter); defined in aesgcm_srtp_kdf.hip
struct aesgcm_srtp_kdf;
struct SkdfView { SkdfTable t; int device; };
SkdfView skdf_view(const aesgcm_srtp_kdf *k);
struct KtSlot;
struct SkdfInstallParams {
    SkdfTable t;
    const u32 *idx, *slots;                // n each
    const u64 *r;                          // n, or NULL = all 0
    KtSlot *tab;
    u32 n, n_slots;
    u32 label[2];                          // by role: the key's and the salt's label byte
};
struct SkdfSetParams {
    SkdfTable t;
    const u32 *idx;
    const unsigned char *keys, *salts;     // n * key_len and n * 14 bytes
    u32 n;
};

// RFC 3711 4.3.1 with RFC 7714 11 (the GCM transforms have no authentication key): SRTP key 0x00, salt 0x02; SRTCP key 0x03, salt 0x05
HD u32 skdf_label(u32 kind, u32 role) { return (kind == AESGCM_SRTP_RTCP ? 3u : 0u) + 2u * role; }

HD bool skdf_rec_set(const SkdfTable &t, u32 r) { return r < t.n_masters && t.rec[(size_t)r * KDF_REC_WORDS + KDF_REC_WORDS - 1u] == SKDF_SET; }
// a whole record from a key and a 14-byte salt at any byte address: the marker last
HD void skdf_store(const SkdfTable &t, u32 r, const unsigned char *key, const unsigned char *salt) {
    u32 *rec = t.rec + (size_t)r * KDF_REC_WORDS;
    for (u32 k = 0; k < KDF_REC_WORDS - 1u; k++) {
        u32 w = 0;
        for (u32 b = 0; b < 4u; b++) {
            const u32 at = 4u * k + b;                                            // the byte's place in the record
            if (at < t.key_len) w |= (u32)key[at] << (8u * b);
            else if (at >= 4u * SKDF_SALT_WORD && at < 4u * SKDF_SALT_WORD + SKDF_SALT_LEN) w |= (u32)salt[at - 4u * SKDF_SALT_WORD] << (8u * b);
        }
        rec[k] = w;
    }
    rec[KDF_REC_WORDS - 1u] = SKDF_SET;
}
// the record's master key as NK memory-order words
template <int NK> HD void skdf_load_key(const SkdfTable &t, u32 r, u32 *rk) {
    const u32 *rec = t.rec + (size_t)r * KDF_REC_WORDS;
#pragma unroll
    for (int k = 0; k < NK; k++) rk[k] = rec[k];
}
// x | be16(0) as four memory-order words: byte 7 is the top of word 1, bytes 8 .. 11 = be32(r >> 16), bytes 12, 13 = be16(r), bytes 14, 15 the block counter
HD void skdf_x(const SkdfTable &t, u32 r_rec, u32 label, u64 r, u32 *x) {
    const u32 *s = t.rec + (size_t)r_rec * KDF_REC_WORDS + SKDF_SALT_WORD;
    x[0] = s[0];
    x[1] = s[1] ^ (label << 24);
    x[2] = s[2] ^ bswap32((u32)(r >> 16));
    x[3] = (s[3] & 0xFFFFu) ^ bswap32((u32)r << 16);
}
// block j of the PRF's output: E_mk(x | be16(j)), rk the master key's schedule
template <int NR> HD void skdf_prf_block(const u32 *x, u32 j, const u32 *rk, const unsigned char *smem, u32 lb, u32 *out) {
    u32 s0 = x[0] ^ rk[0], s1 = x[1] ^ rk[1], s2 = x[2] ^ rk[2], s3 = x[3] ^ bswap32(j) ^ rk[3];
    aes_rounds_lds<NR>(s0, s1, s2, s3, rk, smem, lb);
    out[0] = s0; out[1] = s1; out[2] = s2; out[3] = s3;
}
// Entry i of an install call: both lanes of the entry (key, salt) come to the same verdict from the same words, so an entry is installed whole or not at all.
// The tests in this order: the record in range; the record set; the slot in range; r below 2^48
HD bool skdf_install_entry(const SkdfInstallParams &p, u32 i, u32 &rec, u32 &slot, u64 &r) {
    rec = p.idx[i];
    if (!skdf_rec_set(p.t, rec)) return false;
    slot = p.slots[i];
    if (slot >= p.n_slots) return false;
    r = p.r ? p.r[i] : 0ull;
    return r < SKDF_R_END;
}
// What a lane derives: the master key into rk, its schedule in place (kdf_key_schedule, aesgcm_kdf_slot.h), then the PRF's blocks -- a key lane the first NR - 6 words of the output (out[0 .. NR - 7]),
// a salt lane one block (out[0 .. 3], of which the slot takes three words).  rk: 4 * (NR + 1) words of the lane's registers; nothing is stored
template <int NR> HD void skdf_derive(const SkdfTable &t, u32 role, u32 label, u32 rec, u64 r, u32 *rk, const unsigned char *smem, u32 lb, u32 *out) {
    constexpr int NK = NR - 6;
    u32 x[4];
    skdf_load_key<NK>(t, rec, rk);
    kdf_key_schedule<NR>(rk, smem, lb);
    skdf_x(t, rec, label, r, x);
    skdf_prf_block<NR>(x, 0u, rk, smem, lb, out);
    if (NK > 4 && role == SKDF_ROLE_KEY) {
        u32 more[4];
        skdf_prf_block<NR>(x, 1u, rk, smem, lb, more);
#pragma unroll
        for (int k = 4; k < NK; k++) out[k] = more[k - 4];
    }
}
HD void skdf_set_lane(const SkdfSetParams &p, u32 i) {
    const u32 r = p.idx[i];
    if (r >= p.t.n_masters) { kdf_refuse(p.t.status, i); return; }
    skdf_store(p.t, r, p.keys + (size_t)i * p.t.key_len, p.salts + (size_t)i * SKDF_SALT_LEN);
}

// launchers (aesgcm_srtp_kdf_kernels.hip)
struct DevTables;
hipError_t klaunch_srtp_kdf_attributes();                             // hipFuncSetAttribute(MaxDynamicSharedMemorySize) of the install kernel's instances, on the current device
hipError_t klaunch_srtp_kdf_install(int nr, hipStream_t st, const DevTables *tb, const SkdfInstallParams &p);      // grid: entries x 2 roles
hipError_t klaunch_srtp_kdf_set(hipStream_t st, const SkdfSetParams &p);
