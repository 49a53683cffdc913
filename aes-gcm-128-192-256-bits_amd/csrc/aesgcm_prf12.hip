// aesgcm_prf12.hip -- the TLS 1.2 PRF on the device (include/aesgcm.h "TLS 1.2 PRF"): the host side of aesgcm_prf12_*.  The kernels are in aesgcm_prf12_kernels.hip, the
// lane code and the layout of the state in aesgcm_prf12.h.  A table is a DevTable (aesgcm_internal.h; defined in aesgcm_host.hip) whose state is n_masters records of
// 128 bytes.  Host masters reach the records through the staging buffer (devtab_put), zeroed behind its use as aesgcm_kdf_set zeroes its secrets; the host's own copy
// is wiped before the call returns (SecretWords); clear is devtab_clear; destroy wipes the records and the stage.  install and export are ONE launch each on the
// caller's stream: they neither synchronise nor allocate nor record an event nor read anything back -- capture-safe (include/aesgcm.h, CAPTURE).  The key table is
// reached through kt_view (aesgcm_keytab.h), the SRTP master table that the exporter fills through skdf_view (aesgcm_srtp_kdf.h), and nothing else.
#include "aesgcm_internal.h"
#include "aesgcm_keytab.h"
#include "aesgcm_prf12.h"

#include <string.h>

struct aesgcm_prf12 {
    DevTable base;                     // base.stage: host masters wait there for their copy into the records, zeroed behind it; base.stage_done: behind that zeroing
    Prf12Table t = {};                 // t.status == base.status: the kernels' copy of the pointer
};
static const unsigned char PRF12_KEY_EXPANSION[] = "key expansion";             // RFC 5246 6.3
static const unsigned char PRF12_EXPORTER[] = "EXTRACTOR-dtls_srtp";            // RFC 5764 4.2
static_assert(sizeof PRF12_KEY_EXPANSION - 1 == PRF12_LL_KEY_EXPANSION && sizeof PRF12_EXPORTER - 1 == PRF12_LL_EXPORTER, "the kernels are compiled for these label lengths");

int aesgcm_prf12_create(aesgcm_prf12 **out, int device, size_t hash_len, size_t n_masters) {
    if (!out) return AESGCM_EARG;
    *out = nullptr;
    if ((hash_len != 32 && hash_len != 48) || !n_masters || n_masters >= ((size_t)1 << 31)) return AESGCM_EARG;
    aesgcm_prf12 *k = new aesgcm_prf12();
    k->t.n_masters = (u32)n_masters; k->t.hash_len = (u32)hash_len;
    int rc = devtab_create(&k->base, device, n_masters * PRF12_REC_WORDS * sizeof(u32), (void **)&k->t.rec, "aesgcm_prf12_create");
    if (rc) { delete k; return rc; }
    k->t.status = k->base.status;
    const hipError_t e = klaunch_prf12_attributes();                      // (the device is current: devtab_create)
    if (e != hipSuccess) { rc = hip_fail(e, "aesgcm_prf12_create: klaunch_prf12_attributes"); aesgcm_prf12_destroy(k); return rc; }
    *out = k;
    return AESGCM_OK;
}

int aesgcm_prf12_set(aesgcm_prf12 *k, size_t first, size_t n, const uint8_t *masters, const uint8_t *client_randoms, const uint8_t *server_randoms, void *stream) {
    if (!k) return AESGCM_EARG;
    if (!n) return AESGCM_OK;
    if (!masters || !client_randoms || !server_randoms || !devtab_in_range(first, n, k->t.n_masters)) return AESGCM_EARG;
    SecretWords rec(n * PRF12_REC_WORDS, 0);                                                // (wiped on every return path)
    Prf12Table host = k->t;                                                                 // the same record layout, by the same function, over the host's copy
    host.rec = rec.data();
    for (size_t i = 0; i < n; i++) prf12_store(host, (u32)i, masters + i * PRF12_MASTER_LEN, client_randoms + i * PRF12_RANDOM_LEN, server_randoms + i * PRF12_RANDOM_LEN);
    return devtab_put(&k->base, k->t.rec + first * PRF12_REC_WORDS, rec.data(), rec.size() * sizeof(u32), (hipStream_t)stream, true);
}

int aesgcm_prf12_set_dev(aesgcm_prf12 *k, size_t n, const uint32_t *d_idx, const void *d_masters, const void *d_client_randoms, const void *d_server_randoms, void *stream) {
    if (!k) return AESGCM_EARG;
    if (!n) return AESGCM_OK;
    if (!d_idx || !d_masters || !d_client_randoms || !d_server_randoms || n >= ((size_t)1 << 31)) return AESGCM_EARG;
    Prf12SetParams p;
    p.t = k->t; p.idx = d_idx; p.masters = (const unsigned char *)d_masters; p.client_randoms = (const unsigned char *)d_client_randoms;
    p.server_randoms = (const unsigned char *)d_server_randoms; p.n = (u32)n;
    HIPCHK(hipSetDevice(k->base.device));
    HIPCHK(klaunch_prf12_set((hipStream_t)stream, p));
    return AESGCM_OK;
}

int aesgcm_prf12_clear(aesgcm_prf12 *k, size_t first, size_t n, void *stream) {
    if (!k) return AESGCM_EARG;
    if (!n) return AESGCM_OK;
    if (!devtab_in_range(first, n, k->t.n_masters)) return AESGCM_EARG;
    return devtab_clear(&k->base, k->t.rec + first * PRF12_REC_WORDS, n * PRF12_REC_WORDS * sizeof(u32), (hipStream_t)stream);
}

int aesgcm_prf12_install_dev(aesgcm_prf12 *k, aesgcm_keytab *keytab, size_t n, const uint32_t *d_idx, const uint32_t *d_client_slots, const uint32_t *d_server_slots,
                             void *stream) {
    if (!k || !keytab) return AESGCM_EARG;
    if (!n) return AESGCM_OK;
    if (!d_idx || (!d_client_slots && !d_server_slots) || n >= ((size_t)1 << 31)) return AESGCM_EARG;
    const KtView kv = kt_view(keytab);
    if (kv.device != k->base.device) return AESGCM_EARG;
    Prf12InstallParams p;
    memset(&p, 0, sizeof p);
    p.t = k->t; p.idx = d_idx; p.slots[PRF12_CLIENT] = d_client_slots; p.slots[PRF12_SERVER] = d_server_slots; p.tab = kv.tab; p.n = (u32)n; p.n_slots = kv.n_slots;
    prf12_label(PRF12_KEY_EXPANSION, PRF12_LL_KEY_EXPANSION, p.label);
    DeviceState *ds;
    const int rc = device_state(kv.device, &ds);                          // (made on first use: the ordinary call before a capture)
    if (rc) return rc;
    HIPCHK(hipSetDevice(kv.device));
    HIPCHK(klaunch_prf12_install(kv.nr, (hipStream_t)stream, ds->tables, p));
    return AESGCM_OK;
}

int aesgcm_prf12_export_srtp_dev(aesgcm_prf12 *k, aesgcm_srtp_kdf *masters, size_t n, const uint32_t *d_idx, const uint32_t *d_client_recs, const uint32_t *d_server_recs,
                                 void *stream) {
    if (!k || !masters) return AESGCM_EARG;
    if (!n) return AESGCM_OK;
    if (!d_idx || (!d_client_recs && !d_server_recs) || n >= ((size_t)1 << 31)) return AESGCM_EARG;
    const SkdfView mv = skdf_view(masters);
    if (mv.device != k->base.device || mv.t.key_len == 24u) return AESGCM_EARG;      // DTLS-SRTP has AEAD_AES_128_GCM and AEAD_AES_256_GCM (RFC 7714 14.2)
    Prf12ExportParams p;
    memset(&p, 0, sizeof p);
    p.t = k->t; p.idx = d_idx; p.recs[PRF12_CLIENT] = d_client_recs; p.recs[PRF12_SERVER] = d_server_recs; p.m = mv.t; p.n = (u32)n;
    prf12_label(PRF12_EXPORTER, PRF12_LL_EXPORTER, p.label);
    HIPCHK(hipSetDevice(k->base.device));
    HIPCHK(klaunch_prf12_export((hipStream_t)stream, p));
    return AESGCM_OK;
}

int aesgcm_prf12_status(aesgcm_prf12 *k, int *code, uint64_t *detail) {
    if (!k || !code) return AESGCM_EARG;
    return devtab_status(&k->base, code, detail);
}

int aesgcm_prf12_destroy(aesgcm_prf12 *k) {
    if (!k) return AESGCM_OK;
    const int rc = devtab_destroy(&k->base, k->t.rec, (size_t)k->t.n_masters * PRF12_REC_WORDS * sizeof(u32), "aesgcm_prf12_destroy");      // the records and the stage wiped: both held master secrets
    delete k;
    return rc;
}

// IKEv2's prf+ (aesgcm_prfplus_*): its host side is compiled here, inside this unit (aesgcm_prfplus.hip says why)
#include "aesgcm_prfplus.hip"
