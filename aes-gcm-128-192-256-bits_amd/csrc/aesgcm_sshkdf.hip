// aesgcm_sshkdf.hip -- SSH's key derivation on the device (include/aesgcm.h "SSH KEY DERIVATION"): the host side of aesgcm_sshkdf_*.  The kernels are in
// aesgcm_sshkdf_kernels.hip, the lane code and the layout of the state in aesgcm_sshkdf.h.  A table is a DevTable (aesgcm_internal.h; defined in aesgcm_host.hip)
// whose state is n_recs records of a size fixed at create.  Host secrets reach the records through the staging buffer (devtab_put), zeroed behind its use as
// aesgcm_kdf_set zeroes its secrets; the host's own copy is wiped before the call returns (SecretWords); clear is devtab_clear; destroy wipes the records and the
// stage.  install is ONE launch on the caller's stream: it neither synchronises nor allocates nor records an event nor reads anything back -- capture-safe
// (include/aesgcm.h, CAPTURE).  The key table is reached through kt_view (aesgcm_keytab.h) and nothing else.
// THIS FILE IS PART OF THE UNIT aesgcm_prf12: aesgcm_mka.hip, the last of the chain that aesgcm_prf12.hip starts, includes it at its end.  A library made of the host
// units alone (tests/fake_hip links a fixed list of them against a fake runtime) gets these entry points with a unit it already links.  Such a library has no launchers
// for this family: the ones below are the weak ones, and every call that would launch fails with AESGCM_EHIP; in the product the kernels' object defines the strong ones.
#include "aesgcm_internal.h"
#include "aesgcm_keytab.h"
#include "aesgcm_sshkdf.h"

#include <string.h>

__attribute__((weak)) hipError_t klaunch_sshk_attributes() { return hipErrorNotSupported; }
__attribute__((weak)) hipError_t klaunch_sshk_install(int, hipStream_t, const DevTables *, const SshkInstallParams &) { return hipErrorNotSupported; }
__attribute__((weak)) hipError_t klaunch_sshk_set(hipStream_t, const SshkSetParams &) { return hipErrorNotSupported; }

struct aesgcm_sshkdf {
    DevTable base;                     // base.stage: host secrets wait there for their copy into the records, zeroed behind it; base.stage_done: behind that zeroing
    SshkTable t = {};                  // t.status == base.status: the kernels' copy of the pointer
};

static size_t sshk_state_bytes(const SshkTable &t) { return (size_t)t.n_recs * t.rec_words * sizeof(u32); }

int aesgcm_sshkdf_create(aesgcm_sshkdf **out, int device, size_t hash_len, size_t max_secret_len, size_t n_recs) {
    if (!out) return AESGCM_EARG;
    *out = nullptr;
    if ((hash_len != 32 && hash_len != 48 && hash_len != 64) || !max_secret_len || max_secret_len > SSHK_SECRET_MAX || !n_recs || n_recs >= ((size_t)1 << 31)) return AESGCM_EARG;
    aesgcm_sshkdf *k = new aesgcm_sshkdf();
    k->t.n_recs = (u32)n_recs; k->t.hash_len = (u32)hash_len; k->t.max_secret_len = (u32)max_secret_len; k->t.rec_words = sshk_rec_words((u32)max_secret_len);
    int rc = devtab_create(&k->base, device, sshk_state_bytes(k->t), (void **)&k->t.rec, "aesgcm_sshkdf_create");
    if (rc) { delete k; return rc; }
    k->t.status = k->base.status;
    const hipError_t e = klaunch_sshk_attributes();                       // (the device is current: devtab_create)
    if (e != hipSuccess) { rc = hip_fail(e, "aesgcm_sshkdf_create: klaunch_sshk_attributes"); aesgcm_sshkdf_destroy(k); return rc; }
    *out = k;
    return AESGCM_OK;
}

int aesgcm_sshkdf_set(aesgcm_sshkdf *k, size_t first, size_t n, const uint8_t *secrets, const uint32_t *secret_off, const uint8_t *session_ids, void *stream) {
    if (!k) return AESGCM_EARG;
    if (!n) return AESGCM_OK;
    if (!secrets || !secret_off || !session_ids || !devtab_in_range(first, n, k->t.n_recs)) return AESGCM_EARG;
    for (size_t i = 0; i < n; i++)
        if (secret_off[i + 1] <= secret_off[i] || secret_off[i + 1] - secret_off[i] > k->t.max_secret_len) return AESGCM_EARG;      // before anything is stored
    SecretWords rec(n * k->t.rec_words, 0);                                                 // (wiped on every return path)
    SshkTable host = k->t;                                                                  // the same record layout, by the same function, over the host's copy
    host.rec = rec.data();
    for (size_t i = 0; i < n; i++) sshk_store(host, (u32)i, secrets + secret_off[i], secret_off[i + 1] - secret_off[i], session_ids + i * k->t.hash_len);
    return devtab_put(&k->base, k->t.rec + first * k->t.rec_words, rec.data(), rec.size() * sizeof(u32), (hipStream_t)stream, true);
}

int aesgcm_sshkdf_set_dev(aesgcm_sshkdf *k, size_t n, const uint32_t *d_idx, const void *d_secrets, const uint32_t *d_secret_off, const void *d_session_ids, void *stream) {
    if (!k) return AESGCM_EARG;
    if (!n) return AESGCM_OK;
    if (!d_idx || !d_secrets || !d_secret_off || !d_session_ids || n >= ((size_t)1 << 31)) return AESGCM_EARG;
    SshkSetParams p;
    p.t = k->t; p.idx = d_idx; p.secrets = (const unsigned char *)d_secrets; p.secret_off = d_secret_off; p.sids = (const unsigned char *)d_session_ids; p.n = (u32)n;
    HIPCHK(hipSetDevice(k->base.device));
    HIPCHK(klaunch_sshk_set((hipStream_t)stream, p));
    return AESGCM_OK;
}

int aesgcm_sshkdf_clear(aesgcm_sshkdf *k, size_t first, size_t n, void *stream) {
    if (!k) return AESGCM_EARG;
    if (!n) return AESGCM_OK;
    if (!devtab_in_range(first, n, k->t.n_recs)) return AESGCM_EARG;
    return devtab_clear(&k->base, k->t.rec + first * k->t.rec_words, n * k->t.rec_words * sizeof(u32), (hipStream_t)stream);
}

int aesgcm_sshkdf_install_dev(aesgcm_sshkdf *k, aesgcm_keytab *keytab, size_t n, const uint32_t *d_idx, const uint32_t *d_c2s_slots, const uint32_t *d_s2c_slots, void *stream) {
    if (!k || !keytab) return AESGCM_EARG;
    if (!n) return AESGCM_OK;
    if (!d_idx || (!d_c2s_slots && !d_s2c_slots) || n >= ((size_t)1 << 31)) return AESGCM_EARG;
    const KtView kv = kt_view(keytab);
    if (kv.device != k->base.device) return AESGCM_EARG;
    SshkInstallParams p;
    memset(&p, 0, sizeof p);
    p.t = k->t; p.idx = d_idx; p.slots[SSHK_C2S] = d_c2s_slots; p.slots[SSHK_S2C] = d_s2c_slots;
    p.tab = kv.tab; p.n = (u32)n; p.n_slots = kv.n_slots;
    DeviceState *ds;
    const int rc = device_state(kv.device, &ds);                          // (made on first use: the ordinary call before a capture)
    if (rc) return rc;
    HIPCHK(hipSetDevice(kv.device));
    HIPCHK(klaunch_sshk_install(kv.nr, (hipStream_t)stream, ds->tables, p));
    return AESGCM_OK;
}

int aesgcm_sshkdf_status(aesgcm_sshkdf *k, int *code, uint64_t *detail) {
    if (!k || !code) return AESGCM_EARG;
    return devtab_status(&k->base, code, detail);
}

int aesgcm_sshkdf_destroy(aesgcm_sshkdf *k) {
    if (!k) return AESGCM_OK;
    const int rc = devtab_destroy(&k->base, k->t.rec, sshk_state_bytes(k->t), "aesgcm_sshkdf_destroy");      // the records and the stage wiped: both held secrets
    delete k;
    return rc;
}
