// aesgcm_kdf.hip -- on-device key derivation (include/aesgcm.h "ON-DEVICE KEY DERIVATION"): the host side of aesgcm_kdf_*.  The kernels are in aesgcm_kdf_kernels.hip,
// the lane code and the layout of the state in aesgcm_kdf.h.  A table is a DevTable (aesgcm_internal.h; defined in aesgcm_host.hip) whose state is n_secrets records of
// 64 bytes.  Host secrets reach the records through the staging buffer (devtab_put), zeroed behind its use as aesgcm_keytab_set zeroes its keys; the host's own copy
// is wiped before the call returns (SecretWords); clear is devtab_clear; destroy wipes the records and the stage.  install and update are ONE launch each on the caller's stream: they neither synchronise nor allocate nor
// record an event nor read anything back -- capture-safe (include/aesgcm.h, CAPTURE).  The key table is reached through kt_view (aesgcm_keytab.h) and nothing else.
#include "aesgcm_internal.h"
#include "aesgcm_keytab.h"
#include "aesgcm_kdf.h"

#include <string.h>

struct aesgcm_kdf {
    DevTable base;                     // base.stage: host secrets wait there for their copy into the records, zeroed behind it; base.stage_done: behind that zeroing
    KdfTable t = {};                   // t.status == base.status: the kernels' copy of the pointer
};

int aesgcm_kdf_create(aesgcm_kdf **out, int device, size_t hash_len, size_t n_secrets) {
    if (!out) return AESGCM_EARG;
    *out = nullptr;
    if ((hash_len != 32 && hash_len != 48) || !n_secrets || n_secrets >= ((size_t)1 << 31)) return AESGCM_EARG;
    aesgcm_kdf *k = new aesgcm_kdf();
    k->t.n_secrets = (u32)n_secrets; k->t.hash_len = (u32)hash_len;
    int rc = devtab_create(&k->base, device, n_secrets * KDF_REC_WORDS * sizeof(u32), (void **)&k->t.rec, "aesgcm_kdf_create");
    if (rc) { delete k; return rc; }
    k->t.status = k->base.status;
    const hipError_t e = klaunch_kdf_attributes();                        // (the device is current: devtab_create)
    if (e != hipSuccess) { rc = hip_fail(e, "aesgcm_kdf_create: klaunch_kdf_attributes"); aesgcm_kdf_destroy(k); return rc; }
    *out = k;
    return AESGCM_OK;
}

int aesgcm_kdf_set(aesgcm_kdf *k, size_t first, size_t n, const uint8_t *secrets, void *stream) {
    if (!k) return AESGCM_EARG;
    if (!n) return AESGCM_OK;
    if (!secrets || !devtab_in_range(first, n, k->t.n_secrets)) return AESGCM_EARG;
    const size_t hl = k->t.hash_len;
    SecretWords rec(n * KDF_REC_WORDS, 0);                                                  // (wiped on every return path)
    for (size_t i = 0; i < n; i++) { memcpy(&rec[i * KDF_REC_WORDS], secrets + i * hl, hl); rec[i * KDF_REC_WORDS + KDF_REC_WORDS - 1u] = KDF_SET; }
    return devtab_put(&k->base, k->t.rec + first * KDF_REC_WORDS, rec.data(), rec.size() * sizeof(u32), (hipStream_t)stream, true);
}

int aesgcm_kdf_set_dev(aesgcm_kdf *k, size_t n, const uint32_t *d_idx, const void *d_secrets, void *stream) {
    if (!k) return AESGCM_EARG;
    if (!n) return AESGCM_OK;
    if (!d_idx || !d_secrets || n >= ((size_t)1 << 31)) return AESGCM_EARG;
    KdfSetParams p;
    p.t = k->t; p.idx = d_idx; p.secrets = (const unsigned char *)d_secrets; p.n = (u32)n;
    HIPCHK(hipSetDevice(k->base.device));
    HIPCHK(klaunch_kdf_set((hipStream_t)stream, p));
    return AESGCM_OK;
}

int aesgcm_kdf_clear(aesgcm_kdf *k, size_t first, size_t n, void *stream) {
    if (!k) return AESGCM_EARG;
    if (!n) return AESGCM_OK;
    if (!devtab_in_range(first, n, k->t.n_secrets)) return AESGCM_EARG;
    return devtab_clear(&k->base, k->t.rec + first * KDF_REC_WORDS, n * KDF_REC_WORDS * sizeof(u32), (hipStream_t)stream);
}

// label 0 (the key) is what every format has; a label is at most KDF_LABEL_MAX bytes -- the bound under which an HMAC is four compressions (aesgcm_kdf.h)
int aesgcm_kdf_fmt_check(const aesgcm_kdf_fmt *f) {
    if (!f || !f->len[0]) return AESGCM_EARG;
    for (int j = 0; j < 4; j++) if (f->len[j] > KDF_LABEL_MAX) return AESGCM_EARG;
    return AESGCM_OK;
}

int aesgcm_kdf_install_dev(aesgcm_kdf *k, const aesgcm_kdf_fmt *fmt, aesgcm_keytab *keytab, size_t n, const uint32_t *d_idx, const uint32_t *d_slots,
                           const uint32_t *d_aux_slots, void *stream) {
    const int frc = aesgcm_kdf_fmt_check(fmt);
    if (frc) return frc;
    if (!fmt->len[KDF_ROLE_IV] || (d_aux_slots && !fmt->len[KDF_ROLE_AUX])) return AESGCM_EARG;       // a slot is a key and an IV; aux slots need their label
    if (!k || !keytab) return AESGCM_EARG;
    if (!n) return AESGCM_OK;
    if (!d_idx || !d_slots || n >= ((size_t)1 << 31)) return AESGCM_EARG;
    const KtView kv = kt_view(keytab);
    if (kv.device != k->base.device) return AESGCM_EARG;
    const u32 key_len = 4u * (u32)(kv.nr - 6);
    KdfInstallParams p;
    memset(&p, 0, sizeof p);
    p.t = k->t; p.idx = d_idx; p.slots = d_slots; p.aux_slots = d_aux_slots; p.tab = kv.tab; p.n = (u32)n; p.n_slots = kv.n_slots;
    kdf_msg(fmt->label[KDF_ROLE_KEY], fmt->len[KDF_ROLE_KEY], key_len, p.msg[KDF_ROLE_KEY]);
    kdf_msg(fmt->label[KDF_ROLE_IV], fmt->len[KDF_ROLE_IV], 12u, p.msg[KDF_ROLE_IV]);
    if (d_aux_slots) kdf_msg(fmt->label[KDF_ROLE_AUX], fmt->len[KDF_ROLE_AUX], key_len, p.msg[KDF_ROLE_AUX]);
    DeviceState *ds;
    const int rc = device_state(kv.device, &ds);                          // (made on first use: the ordinary call before a capture)
    if (rc) return rc;
    HIPCHK(hipSetDevice(kv.device));
    HIPCHK(klaunch_kdf_install(kv.nr, (hipStream_t)stream, ds->tables, p));
    return AESGCM_OK;
}

int aesgcm_kdf_update_dev(aesgcm_kdf *k, const aesgcm_kdf_fmt *fmt, size_t n, const uint32_t *d_from, const uint32_t *d_to, void *stream) {
    const int frc = aesgcm_kdf_fmt_check(fmt);
    if (frc) return frc;
    if (!fmt->len[KDF_LABEL_UPDATE] || !k) return AESGCM_EARG;
    if (!n) return AESGCM_OK;
    if (!d_from || !d_to || n >= ((size_t)1 << 31)) return AESGCM_EARG;
    KdfUpdateParams p;
    memset(&p, 0, sizeof p);
    p.t = k->t; p.from = d_from; p.to = d_to; p.n = (u32)n;
    kdf_msg(fmt->label[KDF_LABEL_UPDATE], fmt->len[KDF_LABEL_UPDATE], k->t.hash_len, p.msg);
    HIPCHK(hipSetDevice(k->base.device));
    HIPCHK(klaunch_kdf_update((hipStream_t)stream, p));
    return AESGCM_OK;
}

int aesgcm_kdf_status(aesgcm_kdf *k, int *code, uint64_t *detail) {
    if (!k || !code) return AESGCM_EARG;
    return devtab_status(&k->base, code, detail);
}

int aesgcm_kdf_destroy(aesgcm_kdf *k) {
    if (!k) return AESGCM_OK;
    const int rc = devtab_destroy(&k->base, k->t.rec, (size_t)k->t.n_secrets * KDF_REC_WORDS * sizeof(u32), "aesgcm_kdf_destroy");      // the records and the stage wiped: both held secrets
    delete k;
    return rc;
}
