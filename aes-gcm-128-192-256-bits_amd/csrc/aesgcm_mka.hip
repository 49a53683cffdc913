// aesgcm_mka.hip -- MACsec's MKA on the device (include/aesgcm.h "MACSEC MKA"): the host side of aesgcm_mka_*.  The kernels are in aesgcm_mka_kernels.hip, the lane code
// and the layout of the state in aesgcm_mka.h.  A table is a DevTable (aesgcm_internal.h; defined in aesgcm_host.hip) whose state is n_caks records of 64 bytes.  Host
// CAKs reach the records through the staging buffer (devtab_put), zeroed behind its use as aesgcm_kdf_set zeroes its secrets; the host's own copy is wiped before the
// call returns (SecretWords); clear is devtab_clear; destroy wipes the records and the stage.  install and unwrap are ONE launch each on the caller's stream: they
// neither synchronise nor allocate nor record an event nor read anything back -- capture-safe (include/aesgcm.h, CAPTURE).  The key table is reached through kt_view
// (aesgcm_keytab.h) and nothing else.
// THIS FILE IS PART OF THE UNIT aesgcm_prf12: aesgcm_prfplus.hip, which aesgcm_prf12.hip includes at its end, includes it at its own.  A library made of the host units
// alone (tests/fake_hip links a fixed list of them against a fake runtime) gets these entry points with a unit it already links.  Such a library has no launchers for
// this family: the ones below are the weak ones, and every call that would launch fails with AESGCM_EHIP; in the product the kernels' object defines the strong ones.
#include "aesgcm_internal.h"
#include "aesgcm_keytab.h"
#include "aesgcm_mka.h"

#include <string.h>

__attribute__((weak)) hipError_t klaunch_mka_attributes() { return hipErrorNotSupported; }
__attribute__((weak)) hipError_t klaunch_mka_install(int, hipStream_t, const DevTables *, const MkaInstallParams &) { return hipErrorNotSupported; }
__attribute__((weak)) hipError_t klaunch_mka_unwrap(int, hipStream_t, const DevTables *, const MkaUnwrapParams &) { return hipErrorNotSupported; }
__attribute__((weak)) hipError_t klaunch_mka_set(hipStream_t, const MkaSetParams &) { return hipErrorNotSupported; }

struct aesgcm_mka {
    DevTable base;                     // base.stage: host CAKs wait there for their copy into the records, zeroed behind it; base.stage_done: behind that zeroing
    MkaTable t = {};                   // t.status == base.status: the kernels' copy of the pointer
};

int aesgcm_mka_create(aesgcm_mka **out, int device, size_t cak_len, size_t n_caks) {
    if (!out) return AESGCM_EARG;
    *out = nullptr;
    if ((cak_len != 16 && cak_len != 32) || !n_caks || n_caks >= ((size_t)1 << 31)) return AESGCM_EARG;
    aesgcm_mka *m = new aesgcm_mka();
    m->t.n_caks = (u32)n_caks; m->t.cak_len = (u32)cak_len;
    int rc = devtab_create(&m->base, device, n_caks * MKA_REC_WORDS * sizeof(u32), (void **)&m->t.rec, "aesgcm_mka_create");
    if (rc) { delete m; return rc; }
    m->t.status = m->base.status;
    const hipError_t e = klaunch_mka_attributes();                        // (the device is current: devtab_create)
    if (e != hipSuccess) { rc = hip_fail(e, "aesgcm_mka_create: klaunch_mka_attributes"); aesgcm_mka_destroy(m); return rc; }
    *out = m;
    return AESGCM_OK;
}

int aesgcm_mka_set(aesgcm_mka *m, size_t first, size_t n, const uint8_t *caks, const uint8_t *keyids, void *stream) {
    if (!m) return AESGCM_EARG;
    if (!n) return AESGCM_OK;
    if (!caks || !keyids || !devtab_in_range(first, n, m->t.n_caks)) return AESGCM_EARG;
    SecretWords rec(n * MKA_REC_WORDS, 0);                                                  // (wiped on every return path)
    MkaTable host = m->t;                                                                   // the same record layout, by the same function, over the host's copy
    host.rec = rec.data();
    for (size_t i = 0; i < n; i++) mka_store(host, (u32)i, caks + i * m->t.cak_len, keyids + i * MKA_KEYID_LEN);
    return devtab_put(&m->base, m->t.rec + first * MKA_REC_WORDS, rec.data(), rec.size() * sizeof(u32), (hipStream_t)stream, true);
}

int aesgcm_mka_set_dev(aesgcm_mka *m, size_t n, const uint32_t *d_idx, const void *d_caks, const void *d_keyids, void *stream) {
    if (!m) return AESGCM_EARG;
    if (!n) return AESGCM_OK;
    if (!d_idx || !d_caks || !d_keyids || n >= ((size_t)1 << 31)) return AESGCM_EARG;
    MkaSetParams p;
    p.t = m->t; p.idx = d_idx; p.caks = (const unsigned char *)d_caks; p.keyids = (const unsigned char *)d_keyids; p.n = (u32)n;
    HIPCHK(hipSetDevice(m->base.device));
    HIPCHK(klaunch_mka_set((hipStream_t)stream, p));
    return AESGCM_OK;
}

int aesgcm_mka_clear(aesgcm_mka *m, size_t first, size_t n, void *stream) {
    if (!m) return AESGCM_EARG;
    if (!n) return AESGCM_OK;
    if (!devtab_in_range(first, n, m->t.n_caks)) return AESGCM_EARG;
    return devtab_clear(&m->base, m->t.rec + first * MKA_REC_WORDS, n * MKA_REC_WORDS * sizeof(u32), (hipStream_t)stream);
}

// what install and unwrap share behind their NULL checks: the key table's view, held to this table's device and to MACsec's two key sizes
static int mka_keytab(const aesgcm_mka *m, const aesgcm_keytab *keytab, KtView &kv, DeviceState **ds) {
    kv = kt_view(keytab);
    if (kv.device != m->base.device || (kv.nr != 10 && kv.nr != 14)) return AESGCM_EARG;
    return device_state(kv.device, ds);                                   // (made on first use: the ordinary call before a capture)
}

int aesgcm_mka_install_dev(aesgcm_mka *m, aesgcm_keytab *keytab, size_t n, const uint32_t *d_idx, const void *d_ctx, const uint32_t *d_ctx_off, const uint32_t *d_slots,
                           void *d_wrapped, void *stream) {
    if (!m || !keytab) return AESGCM_EARG;
    if (!n) return AESGCM_OK;
    if (!d_idx || !d_ctx || !d_ctx_off || !d_slots || n >= ((size_t)1 << 31)) return AESGCM_EARG;
    KtView kv;
    DeviceState *ds;
    const int rc = mka_keytab(m, keytab, kv, &ds);
    if (rc) return rc;
    MkaInstallParams p;
    memset(&p, 0, sizeof p);
    p.t = m->t; p.idx = d_idx; p.slots = d_slots; p.ctx = (const unsigned char *)d_ctx; p.ctx_off = d_ctx_off; p.wrapped = (unsigned char *)d_wrapped;
    p.tab = kv.tab; p.n = (u32)n; p.n_slots = kv.n_slots;
    HIPCHK(hipSetDevice(kv.device));
    HIPCHK(klaunch_mka_install(kv.nr, (hipStream_t)stream, ds->tables, p));
    return AESGCM_OK;
}

int aesgcm_mka_unwrap_dev(aesgcm_mka *m, aesgcm_keytab *keytab, size_t n, const uint32_t *d_idx, const void *d_wrapped, const uint32_t *d_slots, uint8_t *d_verdict,
                          void *stream) {
    if (!m || !keytab) return AESGCM_EARG;
    if (!n) return AESGCM_OK;
    if (!d_idx || !d_wrapped || !d_slots || n >= ((size_t)1 << 31)) return AESGCM_EARG;
    KtView kv;
    DeviceState *ds;
    const int rc = mka_keytab(m, keytab, kv, &ds);
    if (rc) return rc;
    MkaUnwrapParams p;
    memset(&p, 0, sizeof p);
    p.t = m->t; p.idx = d_idx; p.slots = d_slots; p.wrapped = (const unsigned char *)d_wrapped; p.verdict = d_verdict;
    p.tab = kv.tab; p.n = (u32)n; p.n_slots = kv.n_slots;
    HIPCHK(hipSetDevice(kv.device));
    HIPCHK(klaunch_mka_unwrap(kv.nr, (hipStream_t)stream, ds->tables, p));
    return AESGCM_OK;
}

int aesgcm_mka_status(aesgcm_mka *m, int *code, uint64_t *detail) {
    if (!m || !code) return AESGCM_EARG;
    return devtab_status(&m->base, code, detail);
}

int aesgcm_mka_destroy(aesgcm_mka *m) {
    if (!m) return AESGCM_OK;
    const int rc = devtab_destroy(&m->base, m->t.rec, (size_t)m->t.n_caks * MKA_REC_WORDS * sizeof(u32), "aesgcm_mka_destroy");      // the records and the stage wiped: both held CAKs
    delete m;
    return rc;
}

#include "aesgcm_sshkdf.hip"
