// aesgcm_prfplus.hip -- IKEv2's prf+ on the device (include/aesgcm.h "IKEv2 PRF+"): the host side of aesgcm_prfplus_*.  The kernels are in aesgcm_prfplus_kernels.hip,
// the lane code and the layout of the state in aesgcm_prfplus.h.  A table is a DevTable (aesgcm_internal.h; defined in aesgcm_host.hip) whose state is n_keys records
// of 128 bytes.  Host SK_d values reach the records through the staging buffer (devtab_put), zeroed behind its use as aesgcm_kdf_set zeroes its secrets; the host's
// own copy is wiped before the call returns (SecretWords); clear is devtab_clear; destroy wipes the records and the stage.  install is ONE launch on the caller's
// stream: it neither synchronises nor allocates nor records an event nor reads anything back -- capture-safe (include/aesgcm.h, CAPTURE).  The key table is reached
// through kt_view (aesgcm_keytab.h) and nothing else.
// THIS FILE IS PART OF THE UNIT aesgcm_prf12: aesgcm_prf12.hip includes it at its end.  A library made of the host units alone (tests/fake_hip links a fixed list of
// them against a fake runtime) gets these entry points with a unit it already links.  Such a library has no launchers for this family: the ones below are the weak
// ones, and every call that would launch fails with AESGCM_EHIP; in the product the kernels' object defines the strong ones.
#include "aesgcm_internal.h"
#include "aesgcm_keytab.h"
#include "aesgcm_prfplus.h"

#include <string.h>

__attribute__((weak)) hipError_t klaunch_prfp_attributes() { return hipErrorNotSupported; }
__attribute__((weak)) hipError_t klaunch_prfp_install(int, hipStream_t, const DevTables *, const PrfpInstallParams &) { return hipErrorNotSupported; }
__attribute__((weak)) hipError_t klaunch_prfp_set(hipStream_t, const PrfpSetParams &) { return hipErrorNotSupported; }

struct aesgcm_prfplus {
    DevTable base;                     // base.stage: host SK_d values wait there for their copy into the records, zeroed behind it; base.stage_done: behind that zeroing
    PrfpTable t = {};                  // t.status == base.status: the kernels' copy of the pointer
};

int aesgcm_prfplus_create(aesgcm_prfplus **out, int device, size_t hash_len, size_t n_keys) {
    if (!out) return AESGCM_EARG;
    *out = nullptr;
    if ((hash_len != 32 && hash_len != 48 && hash_len != 64) || !n_keys || n_keys >= ((size_t)1 << 31)) return AESGCM_EARG;
    aesgcm_prfplus *k = new aesgcm_prfplus();
    k->t.n_keys = (u32)n_keys; k->t.hash_len = (u32)hash_len;
    int rc = devtab_create(&k->base, device, n_keys * PRFP_REC_WORDS * sizeof(u32), (void **)&k->t.rec, "aesgcm_prfplus_create");
    if (rc) { delete k; return rc; }
    k->t.status = k->base.status;
    const hipError_t e = klaunch_prfp_attributes();                       // (the device is current: devtab_create)
    if (e != hipSuccess) { rc = hip_fail(e, "aesgcm_prfplus_create: klaunch_prfp_attributes"); aesgcm_prfplus_destroy(k); return rc; }
    *out = k;
    return AESGCM_OK;
}

int aesgcm_prfplus_set(aesgcm_prfplus *k, size_t first, size_t n, const uint8_t *keys, void *stream) {
    if (!k) return AESGCM_EARG;
    if (!n) return AESGCM_OK;
    if (!keys || !devtab_in_range(first, n, k->t.n_keys)) return AESGCM_EARG;
    SecretWords rec(n * PRFP_REC_WORDS, 0);                                                 // (wiped on every return path)
    PrfpTable host = k->t;                                                                  // the same record layout, by the same function, over the host's copy
    host.rec = rec.data();
    for (size_t i = 0; i < n; i++) prfp_store(host, (u32)i, keys + i * k->t.hash_len);
    return devtab_put(&k->base, k->t.rec + first * PRFP_REC_WORDS, rec.data(), rec.size() * sizeof(u32), (hipStream_t)stream, true);
}

int aesgcm_prfplus_set_dev(aesgcm_prfplus *k, size_t n, const uint32_t *d_idx, const void *d_keys, void *stream) {
    if (!k) return AESGCM_EARG;
    if (!n) return AESGCM_OK;
    if (!d_idx || !d_keys || n >= ((size_t)1 << 31)) return AESGCM_EARG;
    PrfpSetParams p;
    p.t = k->t; p.idx = d_idx; p.keys = (const unsigned char *)d_keys; p.n = (u32)n;
    HIPCHK(hipSetDevice(k->base.device));
    HIPCHK(klaunch_prfp_set((hipStream_t)stream, p));
    return AESGCM_OK;
}

int aesgcm_prfplus_clear(aesgcm_prfplus *k, size_t first, size_t n, void *stream) {
    if (!k) return AESGCM_EARG;
    if (!n) return AESGCM_OK;
    if (!devtab_in_range(first, n, k->t.n_keys)) return AESGCM_EARG;
    return devtab_clear(&k->base, k->t.rec + first * PRFP_REC_WORDS, n * PRFP_REC_WORDS * sizeof(u32), (hipStream_t)stream);
}

int aesgcm_prfplus_install_dev(aesgcm_prfplus *k, aesgcm_keytab *keytab, size_t n, const uint32_t *d_idx, const void *d_seed, const uint32_t *d_seed_off,
                               const uint32_t *d_i2r_slots, const uint32_t *d_r2i_slots, void *stream) {
    if (!k || !keytab) return AESGCM_EARG;
    if (!n) return AESGCM_OK;
    if (!d_idx || !d_seed || !d_seed_off || (!d_i2r_slots && !d_r2i_slots) || n >= ((size_t)1 << 31)) return AESGCM_EARG;
    const KtView kv = kt_view(keytab);
    if (kv.device != k->base.device) return AESGCM_EARG;
    PrfpInstallParams p;
    memset(&p, 0, sizeof p);
    p.t = k->t; p.idx = d_idx; p.seed = (const unsigned char *)d_seed; p.seed_off = d_seed_off; p.slots[PRFP_I2R] = d_i2r_slots; p.slots[PRFP_R2I] = d_r2i_slots;
    p.tab = kv.tab; p.n = (u32)n; p.n_slots = kv.n_slots;
    DeviceState *ds;
    const int rc = device_state(kv.device, &ds);                          // (made on first use: the ordinary call before a capture)
    if (rc) return rc;
    HIPCHK(hipSetDevice(kv.device));
    HIPCHK(klaunch_prfp_install(kv.nr, (hipStream_t)stream, ds->tables, p));
    return AESGCM_OK;
}

int aesgcm_prfplus_status(aesgcm_prfplus *k, int *code, uint64_t *detail) {
    if (!k || !code) return AESGCM_EARG;
    return devtab_status(&k->base, code, detail);
}

int aesgcm_prfplus_destroy(aesgcm_prfplus *k) {
    if (!k) return AESGCM_OK;
    const int rc = devtab_destroy(&k->base, k->t.rec, (size_t)k->t.n_keys * PRFP_REC_WORDS * sizeof(u32), "aesgcm_prfplus_destroy");      // the records and the stage wiped: both held SK_d values
    delete k;
    return rc;
}

#include "aesgcm_mka.hip"
