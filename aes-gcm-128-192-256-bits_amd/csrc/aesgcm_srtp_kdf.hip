// aesgcm_srtp_kdf.hip -- SRTP / SRTCP session keys derived on the device (include/aesgcm.h "SRTP KEY DERIVATION"): the host side of aesgcm_srtp_kdf_*.  The kernels are in
// aesgcm_srtp_kdf_kernels.hip, the lane code and the layout of the state in aesgcm_srtp_kdf.h.  A table is a DevTable (aesgcm_internal.h; defined in aesgcm_host.hip)
// whose state is n_masters records of 64 bytes.  Host masters reach the records through the staging buffer (devtab_put), zeroed behind its use as aesgcm_kdf_set zeroes
// its secrets; the host's own copy is wiped before the call returns (SecretWords); clear is devtab_clear; destroy wipes the records and the stage.  install is ONE launch on the caller's stream: it neither synchronises
// nor allocates nor records an event nor reads anything back -- capture-safe (include/aesgcm.h, CAPTURE).  The key table is reached through kt_view (aesgcm_keytab.h) and
// nothing else.
#include "aesgcm_internal.h"
#include "aesgcm_keytab.h"
#include "aesgcm_srtp_kdf.h"

#include <string.h>

struct aesgcm_srtp_kdf {
    DevTable base;                     // base.stage: host masters wait there for their copy into the records, zeroed behind it; base.stage_done: behind that zeroing
    SkdfTable t = {};                  // t.status == base.status: the kernels' copy of the pointer
};

SkdfView skdf_view(const aesgcm_srtp_kdf *k) { return SkdfView{k->t, k->base.device}; }

int aesgcm_srtp_kdf_create(aesgcm_srtp_kdf **out, int device, size_t key_len, size_t n_masters) {
    if (!out) return AESGCM_EARG;
    *out = nullptr;
    if ((key_len != 16 && key_len != 24 && key_len != 32) || !n_masters || n_masters >= ((size_t)1 << 31)) return AESGCM_EARG;
    aesgcm_srtp_kdf *k = new aesgcm_srtp_kdf();
    k->t.n_masters = (u32)n_masters; k->t.key_len = (u32)key_len;
    int rc = devtab_create(&k->base, device, n_masters * KDF_REC_WORDS * sizeof(u32), (void **)&k->t.rec, "aesgcm_srtp_kdf_create");
    if (rc) { delete k; return rc; }
    k->t.status = k->base.status;
    const hipError_t e = klaunch_srtp_kdf_attributes();                   // (the device is current: devtab_create)
    if (e != hipSuccess) { rc = hip_fail(e, "aesgcm_srtp_kdf_create: klaunch_srtp_kdf_attributes"); aesgcm_srtp_kdf_destroy(k); return rc; }
    *out = k;
    return AESGCM_OK;
}

int aesgcm_srtp_kdf_set(aesgcm_srtp_kdf *k, size_t first, size_t n, const uint8_t *keys, const uint8_t *salts, void *stream) {
    if (!k) return AESGCM_EARG;
    if (!n) return AESGCM_OK;
    if (!keys || !salts || !devtab_in_range(first, n, k->t.n_masters)) return AESGCM_EARG;
    SecretWords rec(n * KDF_REC_WORDS, 0);                                                  // (wiped on every return path)
    SkdfTable host = k->t;                                                                  // the same record layout, by the same function, over the host's copy
    host.rec = rec.data();
    for (size_t i = 0; i < n; i++) skdf_store(host, (u32)i, keys + i * k->t.key_len, salts + i * SKDF_SALT_LEN);
    return devtab_put(&k->base, k->t.rec + first * KDF_REC_WORDS, rec.data(), rec.size() * sizeof(u32), (hipStream_t)stream, true);
}

int aesgcm_srtp_kdf_set_dev(aesgcm_srtp_kdf *k, size_t n, const uint32_t *d_idx, const void *d_keys, const void *d_salts, void *stream) {
    if (!k) return AESGCM_EARG;
    if (!n) return AESGCM_OK;
    if (!d_idx || !d_keys || !d_salts || n >= ((size_t)1 << 31)) return AESGCM_EARG;
    SkdfSetParams p;
    p.t = k->t; p.idx = d_idx; p.keys = (const unsigned char *)d_keys; p.salts = (const unsigned char *)d_salts; p.n = (u32)n;
    HIPCHK(hipSetDevice(k->base.device));
    HIPCHK(klaunch_srtp_kdf_set((hipStream_t)stream, p));
    return AESGCM_OK;
}

int aesgcm_srtp_kdf_clear(aesgcm_srtp_kdf *k, size_t first, size_t n, void *stream) {
    if (!k) return AESGCM_EARG;
    if (!n) return AESGCM_OK;
    if (!devtab_in_range(first, n, k->t.n_masters)) return AESGCM_EARG;
    return devtab_clear(&k->base, k->t.rec + first * KDF_REC_WORDS, n * KDF_REC_WORDS * sizeof(u32), (hipStream_t)stream);
}

int aesgcm_srtp_kdf_install_dev(aesgcm_srtp_kdf *k, uint32_t kind, aesgcm_keytab *keytab, size_t n, const uint32_t *d_idx, const uint32_t *d_slots, const uint64_t *d_r,
                                void *stream) {
    if (kind != AESGCM_SRTP_RTP && kind != AESGCM_SRTP_RTCP) return AESGCM_EARG;
    if (!k || !keytab) return AESGCM_EARG;
    if (!n) return AESGCM_OK;
    if (!d_idx || !d_slots || n >= ((size_t)1 << 31)) return AESGCM_EARG;
    const KtView kv = kt_view(keytab);
    if (kv.device != k->base.device || 4u * (u32)(kv.nr - 6) != k->t.key_len) return AESGCM_EARG;      // the PRF's AES size is the key table's
    SkdfInstallParams p;
    memset(&p, 0, sizeof p);
    p.t = k->t; p.idx = d_idx; p.slots = d_slots; p.r = d_r; p.tab = kv.tab; p.n = (u32)n; p.n_slots = kv.n_slots;
    p.label[SKDF_ROLE_KEY] = skdf_label(kind, SKDF_ROLE_KEY); p.label[SKDF_ROLE_SALT] = skdf_label(kind, SKDF_ROLE_SALT);
    DeviceState *ds;
    const int rc = device_state(kv.device, &ds);                          // (made on first use: the ordinary call before a capture)
    if (rc) return rc;
    HIPCHK(hipSetDevice(kv.device));
    HIPCHK(klaunch_srtp_kdf_install(kv.nr, (hipStream_t)stream, ds->tables, p));
    return AESGCM_OK;
}

int aesgcm_srtp_kdf_status(aesgcm_srtp_kdf *k, int *code, uint64_t *detail) {
    if (!k || !code) return AESGCM_EARG;
    return devtab_status(&k->base, code, detail);
}

int aesgcm_srtp_kdf_destroy(aesgcm_srtp_kdf *k) {
    if (!k) return AESGCM_OK;
    const int rc = devtab_destroy(&k->base, k->t.rec, (size_t)k->t.n_masters * KDF_REC_WORDS * sizeof(u32), "aesgcm_srtp_kdf_destroy");      // the records and the stage wiped: both held master keys
    delete k;
    return rc;
}
