// aesgcm_keytab.h -- key tables (aesgcm_keytab_*): device-resident slots of key material that a batch call names per packet.
// Shared by the kernels -- aesgcm_keytab_kernels.hip: k_kt_setup, and k_kt_batch, which runs k_batch3's body (aesgcm_batch3_body.inc) with the key material read from
// slots; aesgcm_wire_kernels.hip, aesgcm_wirex_kernels.hip, aesgcm_tls_kernels.hip, aesgcm_quic_kernels.hip, aesgcm_dtls_kernels.hip, aesgcm_srtp_kernels.hip, aesgcm_ssh_kernels.hip: the same body on packets in wire format, one source per
// family (aesgcm_keytab.hip lists them), what each format decides in aesgcm_wirecut.h -- and the host (aesgcm_keytab.hip, which launches each as aesgcm_host.hip's batch_plan plans k_batch3).  Every launcher below
// picks its instance by aesgcm_dispatch.h.
#pragma once
#include "aesgcm_internal.h"
#include <stddef.h>

// One slot: everything k_batch3 rebuilds per packet from a raw key, built once by k_kt_setup.  384 bytes = three 128-byte lines; `set` is written last.
#define KT_SET 0x5345544Bu                 /* "KTES": the slot holds key material (zero = unset or cleared) */
#define KT_HPOW 7                          /* H^(2^j), j = 0 .. 6: the Horner stride of every shape (8, 16, 64 lanes per packet) and the closing's constants */
struct __attribute__((aligned(128))) KtSlot {
    u32 rk[60];                            // round keys in memory-order words (KeyMaterial::rk); AES-128 / 192 use the first 44 / 52
    u32 nr;
    u32 set;                               // KT_SET once the rest is written
    u32 salt[2];                           // the first bytes of a wire-format frame's nonce (aesgcm_keytab_set_salt), as two memory-order words; k_kt_setup leaves them alone
    uint4 hpow[KT_HPOW];                   // BE words (G128)
    u32 xpn[4];                            // MACsec XPN (aesgcm_keytab_set_xpn): the 12-byte salt as three memory-order words, then the SSCI; apart from `salt`, and k_kt_setup leaves them alone too.
                                           // A TLS connection direction instead (aesgcm_keytab_set_tls_iv): its 12-byte write IV as three memory-order words, then 0 -- either setter overwrites the other
};
static_assert(offsetof(KtSlot, xpn) == 368, "the XPN state fills what was padding: the slot's other fields stay where they were");
static_assert(sizeof(KtSlot) == 384, "a slot is three 128-byte lines");

// a table's slots for the units that fill them without going through aesgcm_keytab_set* (aesgcm_kdf.hip); defined in aesgcm_keytab.hip
struct aesgcm_keytab;
struct KtView { KtSlot *tab; u32 n_slots; int nr, device; };
KtView kt_view(const aesgcm_keytab *t);

struct KtSetupParams {
    const unsigned char *keys;             // n * key_len bytes
    const u32 *slots;                      // n slot numbers, or NULL = first, first + 1, ...
    u32 first, n, n_slots;
    KtSlot *tab;
    u32 *status;                           // lowest refused index (atomicMin), ~0 = none
};

struct KtParams {
    BatchParams b;                         // keys unused; the rest as the batch path
    const u32 *slots;                      // n_pkts slot numbers
    const KtSlot *tab;
    u32 n_slots;
    u32 *status;
};

// A call of frames in wire format (k_kt_wire): b.data_off = the frame offsets, b.in = b.aad = the frames, b.ivs / b.tags / b.expect / b.aad_off unused
struct KtWireParams {
    KtParams k;
    aesgcm_wire_fmt f;                     // checked by aesgcm_wire_fmt_check
};

// ... with an extension (k_kt_wirex): hi[p] = the upper half of frame p's 64-bit packet / sequence number, which is not in the frame
// The body's WIREX modes that the ABI does not name (aesgcm_wire_xfmt_check refuses them as it refuses every unknown bit): TLS records, aesgcm_keytab_records_crypt_dev;
// QUIC packets, aesgcm_keytab_quic_crypt_dev; DTLS records, aesgcm_keytab_dtls_crypt_dev; SRTP and SRTCP packets, aesgcm_keytab_srtp_crypt_dev; SSH binary packets, aesgcm_keytab_ssh_crypt_dev
#define KT_WIREX_TLS13 0x10u
#define KT_WIREX_TLS12 0x20u
#define KT_WIREX_QUIC  0x40u
#define KT_WIREX_DTLS13 0x80u
#define KT_WIREX_DTLS12 0x100u
#define KT_WIREX_SRTP 0x200u
#define KT_WIREX_SRTCP 0x400u
#define KT_WIREX_SSH 0x800u
struct KtWireXParams {
    KtWireParams w;
    union {
        const u32 *hi;                     // n_pkts numeric values (k_kt_srtp, SRTP: the rollover counters; SRTCP: unused); k_kt_srtp: w.f = {0, 0, 0, 0, 16, 0}
        const u64 *seq;                    // k_kt_tls: n_pkts whole 64-bit record sequence numbers; w.f = {5, 5, 5, 0, 16, 0} (1.3) or {13, 13, 5, 4, 16, 0} (1.2)
                                           // k_kt_quic: n_pkts full packet numbers (decrypt: as k_kt_quic_hp decoded them); w.f = {0, 0, 0, 0, 16, 0}, the header's length is per packet
                                           // k_kt_dtls, 1.3: n_pkts full record sequence numbers (decrypt: as k_kt_dtls_sn decoded them); w.f as k_kt_quic's.  1.2: unused;
                                           // w.f = {13, 21, 13, 4, 16, 0}
                                           // k_kt_ssh: n_pkts counts of the packets sent under the slot's key before this one; w.f = {4, 4, 4, 0, 16, 0}
    };
    union {
        u32 mki_len;                       // k_kt_srtp only, in the place of a pointer it does not use: the bytes of MKI that end every packet (the parameters' size stays what it was)
            const u32 *pn_off;                 // k_kt_quic and k_kt_dtls 1.3 only (behind everything the other kernels read): where packet p's packet-number / sequence-number field starts, n_pkts values
    };
    const u32 *hp_slots;                   // ... and its header-protection / record-number slot: the AEAD and the mask kernel refuse a packet by the same function (aesgcm_wirecut.h: wire_front)
};

// A QUIC call's header-protection pass (k_kt_quic_hp, a lane per packet): packet p = bytes [pkt_off[p], pkt_off[p + 1]) of in / out.  A DTLS 1.3 call's record-number
// pass (k_kt_dtls_sn) takes the same: pn_off = where the sequence-number field starts, hp_slots = the `sn` key's slots, pn / pn_out = the record sequence numbers
struct KtQuicHpParams {
    const unsigned char *in;
    unsigned char *out;
    const u64 *pkt_off;
    const u32 *slots, *hp_slots, *pn_off;
    const u64 *pn;                         // encrypt: the full numbers (only their range is checked here); decrypt: the expected ones
    u64 *pn_out;                           // decrypt: the decoded numbers (may be pn)
    const KtSlot *tab;
    u32 n_pkts, n_slots;
};

// per family: klaunch_*_attributes = hipFuncSetAttribute(MaxDynamicSharedMemorySize) of every instance, on the current device (klaunch_set_attributes calls them all)
hipError_t klaunch_kt_attributes();
hipError_t klaunch_kt_setup(int nr, hipStream_t st, const DevTables *tb, const KtSetupParams &s);
hipError_t klaunch_kt_batch(int nr, int dec, int lg, unsigned wgs, hipStream_t st, const DevTables *tb, const KtParams &p);
hipError_t klaunch_wire_attributes();
hipError_t klaunch_kt_wire(int nr, int dec, int lg, unsigned wgs, hipStream_t st, const DevTables *tb, const KtWireParams &p);
hipError_t klaunch_wirex_attributes();
hipError_t klaunch_kt_wirex(unsigned ext, int nr, int dec, int lg, unsigned wgs, hipStream_t st, const DevTables *tb, const KtWireXParams &p);     // ext: AESGCM_WIREX_XPN or _ESN
hipError_t klaunch_tls_attributes();
hipError_t klaunch_kt_tls(unsigned version, int nr, int dec, int lg, unsigned wgs, hipStream_t st, const DevTables *tb, const KtWireXParams &p);   // version: AESGCM_TLS_13 or _12
hipError_t klaunch_quic_attributes();      // k_kt_quic and k_kt_quic_hp
hipError_t klaunch_kt_quic(int nr, int dec, int lg, unsigned wgs, hipStream_t st, const DevTables *tb, const KtWireXParams &p);
hipError_t klaunch_kt_quic_hp(int nr, int dec, hipStream_t st, const DevTables *tb, const KtQuicHpParams &p);
hipError_t klaunch_dtls_attributes();      // k_kt_dtls and k_kt_dtls_sn
hipError_t klaunch_kt_dtls(unsigned version, int nr, int dec, int lg, unsigned wgs, hipStream_t st, const DevTables *tb, const KtWireXParams &p);  // version: AESGCM_DTLS_13 or _12
hipError_t klaunch_kt_dtls_sn(int nr, int dec, hipStream_t st, const DevTables *tb, const KtQuicHpParams &p);
hipError_t klaunch_srtp_attributes();
hipError_t klaunch_kt_srtp(unsigned kind, int nr, int dec, int lg, unsigned wgs, hipStream_t st, const DevTables *tb, const KtWireXParams &p);  // kind: AESGCM_SRTP_RTP or _RTCP
hipError_t klaunch_ssh_attributes();
hipError_t klaunch_kt_ssh(int nr, int dec, int lg, unsigned wgs, hipStream_t st, const DevTables *tb, const KtWireXParams &p);
