// aesgcm_keytab.h -- key tables (aesgcm_keytab_*): device-resident slots of key material that a batch call names per packet.
// Shared by the kernels (aesgcm_keytab_kernels.hip: k_kt_setup; k_kt_batch runs k_batch3's body, aesgcm_batch3_body.inc, which names the slots) and the host
// (aesgcm_keytab.hip, which launches k_kt_batch as aesgcm_host.hip's batch_plan plans it for k_batch3).
#pragma once
#include "aesgcm_internal.h"

// One slot: everything k_batch3 rebuilds per packet from a raw key, built once by k_kt_setup.  384 bytes = three 128-byte lines; `set` is written last.
#define KT_SET 0x5345544Bu                 /* "KTES": the slot holds key material (zero = unset or cleared) */
#define KT_HPOW 7                          /* H^(2^j), j = 0 .. 6: the Horner stride of every shape (8, 16, 64 lanes per packet) and the closing's constants */
struct __attribute__((aligned(128))) KtSlot {
    u32 rk[60];                            // round keys in memory-order words (KeyMaterial::rk); AES-128 / 192 use the first 44 / 52
    u32 nr;
    u32 set;                               // KT_SET once the rest is written
    u32 pad0[2];
    uint4 hpow[KT_HPOW];                   // BE words (G128)
    u32 pad1[4];
};
static_assert(sizeof(KtSlot) == 384, "a slot is three 128-byte lines");

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

hipError_t klaunch_kt_attributes();        // hipFuncSetAttribute(MaxDynamicSharedMemorySize) of every keytab instance, on the current device (klaunch_set_attributes)
hipError_t klaunch_kt_setup(int nr, hipStream_t st, const DevTables *tb, const KtSetupParams &s);
hipError_t klaunch_kt_batch(int nr, int dec, int lg, unsigned wgs, hipStream_t st, const DevTables *tb, const KtParams &p);
