// aesgcm_keytab.hip -- key tables (include/aesgcm.h "key tables"): the host side of aesgcm_keytab_*.  The kernels are in aesgcm_<family>_kernels.hip, one source per family.
// A table is a DevTable (aesgcm_internal.h: create, the staged set, clear, status, destroy, the range check; defined in aesgcm_host.hip) whose state is n_slots KtSlot
// records (aesgcm_keytab.h).  Host data reaches the slots through the staging buffer, zeroed behind every use (kt_stage_set, on devtab_staged): keys by k_kt_setup,
// the other fields (salt, XPN state, TLS IV) by strided copies.  A crypt call is one launch of a kernel that runs k_batch3's body,
// planned by batch_plan (aesgcm_host.hip) as the batch path's: the shape by batch_pick_lg, the same dispenser ring, order and deal.
//   family   entry point                          kernel       the format's cut (aesgcm_wirecut.h)
//   keytab   aesgcm_keytab_crypt_dev              k_kt_batch   -                       packets as five arrays
//   wire     aesgcm_keytab_frames_crypt_dev       k_kt_wire    cut_wire                frames in wire format
//   wirex    aesgcm_keytab_frames_crypt_x_dev     k_kt_wirex   cut_wire                ... with a number per frame that is not on the wire (MACsec XPN, ESP ESN)
//   tls      aesgcm_keytab_records_crypt_dev      k_kt_tls     cut_wire                TLS records with their 64-bit sequence numbers
//   quic     aesgcm_keytab_quic_crypt_dev         k_kt_quic    cut_quic                QUIC packets, and a second launch, k_kt_quic_hp (header protection, a lane per packet)
//   dtls     aesgcm_keytab_dtls_crypt_dev         k_kt_dtls    cut_dtls13, cut_wire    DTLS records; 1.3: and a second launch, k_kt_dtls_sn (record-number encryption, a lane per record)
//   srtp     aesgcm_keytab_srtp_crypt_dev         k_kt_srtp    (body text), cut_srtcp    SRTP and SRTCP packets (RFC 7714)
//   ssh      aesgcm_keytab_ssh_crypt_dev          k_kt_ssh     cut_ssh                 SSH binary packets (RFC 5647) with the number of packets sent before each
// The calls in wire format all go through kt_wire_crypt.
#include "aesgcm_keytab.h"

#include <stddef.h>
#include <string.h>

struct aesgcm_keytab {
    DevTable base;                     // base.stage: host keys wait there for k_kt_setup, zeroed behind it on the same stream; base.stage_done: behind that zeroing
    int nr = 0;
    size_t key_len = 0, n_slots = 0;
    KtSlot *tab = nullptr;
};

KtView kt_view(const aesgcm_keytab *t) { return KtView{t->tab, (u32)t->n_slots, t->nr, t->base.device}; }

static int kt_setup(aesgcm_keytab *t, const unsigned char *d_keys, const u32 *d_slots, size_t first, size_t n, hipStream_t st) {
    DeviceState *ds;
    int rc = device_state(t->base.device, &ds);
    if (rc) return rc;
    if ((rc = set_lds_attrs(t->base.device, ds))) return rc;
    KtSetupParams s;
    s.keys = d_keys; s.slots = d_slots; s.first = (u32)first; s.n = (u32)n; s.n_slots = (u32)t->n_slots; s.tab = t->tab; s.status = t->base.status;
    HIPCHK(klaunch_kt_setup(t->nr, st, ds->tables, s));
    return AESGCM_OK;
}

int aesgcm_keytab_create(aesgcm_keytab **out, int device, size_t key_len, size_t n_slots) {
    if (!out) return AESGCM_EARG;
    *out = nullptr;
    if ((key_len != 16 && key_len != 24 && key_len != 32) || !n_slots || n_slots >= ((size_t)1 << 31)) return AESGCM_EARG;
    aesgcm_keytab *t = new aesgcm_keytab();
    t->key_len = key_len; t->n_slots = n_slots; t->nr = (int)(key_len / 4 + 6);
    const int rc = devtab_create(&t->base, device, n_slots * sizeof(KtSlot), (void **)&t->tab, "aesgcm_keytab_create");
    if (rc) { delete t; return rc; }
    *out = t;
    return AESGCM_OK;
}

// What every host-to-slot setter does: one staged set (devtab_staged: the stage holds key material, so it is zeroed behind the call) whose body copies `parts` side
// by side into the stage and has `into_slots` (the expansion kernel, or a strided copy per part) take them from there into the slots.  The caller has checked its
// arguments.
struct KtPart {
    const uint8_t *src;                // host: n * width bytes; NULL = the field becomes zero (nothing staged)
    size_t width, field;               // bytes per slot; offset inside KtSlot
};
template <size_t N, class F>
static int kt_stage_set(aesgcm_keytab *t, size_t n, const KtPart (&parts)[N], hipStream_t st, F into_slots) {
    DevTable &b = t->base;
    size_t bytes = 0;
    for (const KtPart &p : parts) if (p.src) bytes += n * p.width;
    return devtab_staged(b, bytes, st, true, [&]() -> int {
        size_t at = 0;
        for (const KtPart &p : parts) if (p.src) { HIPCHK(hipMemcpyAsync(b.stage + at, p.src, n * p.width, hipMemcpyHostToDevice, st)); at += n * p.width; }
        return into_slots();
    });
}

// the fields that k_kt_setup leaves alone (salt, xpn): each part from the stage into its field of slots first_slot, ... by one 2-D copy (the slots are 384 bytes apart)
template <size_t N>
static int kt_set_fields(aesgcm_keytab *t, size_t first_slot, size_t n, const KtPart (&parts)[N], hipStream_t st) {
    return kt_stage_set(t, n, parts, st, [&]() -> int {
        size_t at = 0;
        for (const KtPart &p : parts) {
            unsigned char *const dst = (unsigned char *)(t->tab + first_slot) + p.field;
            if (p.src) { HIPCHK(hipMemcpy2DAsync(dst, sizeof(KtSlot), t->base.stage + at, p.width, p.width, n, hipMemcpyDeviceToDevice, st)); at += n * p.width; }
            else HIPCHK(hipMemset2DAsync(dst, sizeof(KtSlot), 0, p.width, n, st));
        }
        return AESGCM_OK;
    });
}

int aesgcm_keytab_set(aesgcm_keytab *t, size_t first_slot, size_t n, const uint8_t *keys, void *stream) {
    if (!t) return AESGCM_EARG;
    if (!n) return AESGCM_OK;
    if (!keys || !devtab_in_range(first_slot, n, t->n_slots)) return AESGCM_EARG;
    hipStream_t st = (hipStream_t)stream;
    const KtPart parts[] = {{keys, t->key_len, 0}};
    return kt_stage_set(t, n, parts, st, [&] { return kt_setup(t, t->base.stage, nullptr, first_slot, n, st); });
}

int aesgcm_keytab_set_dev(aesgcm_keytab *t, size_t n, const uint32_t *d_slots, const void *d_keys, void *stream) {
    if (!t) return AESGCM_EARG;
    if (!n) return AESGCM_OK;
    if (!d_slots || !d_keys || n >= ((size_t)1 << 31)) return AESGCM_EARG;
    HIPCHK(hipSetDevice(t->base.device));
    return kt_setup(t, (const unsigned char *)d_keys, d_slots, 0, n, (hipStream_t)stream);
}

int aesgcm_keytab_clear(aesgcm_keytab *t, size_t first_slot, size_t n, void *stream) {
    if (!t) return AESGCM_EARG;
    if (!n) return AESGCM_OK;
    if (!devtab_in_range(first_slot, n, t->n_slots)) return AESGCM_EARG;
    return devtab_clear(&t->base, t->tab + first_slot, n * sizeof(KtSlot), (hipStream_t)stream);
}

// Batches with a slot per packet: the argument checks and KtParams here, the dispenser, shape, order and deal by batch_plan, as batch_launch does for k_batch3
int aesgcm_keytab_crypt_dev(aesgcm_keytab *t, int decrypt, size_t n_pkts, const uint32_t *d_slots, const void *d_ivs,
                            const void *d_aad, size_t aad_len, const uint64_t *d_aad_off,
                            const void *d_in, size_t pkt_len, const uint64_t *d_data_off, void *d_out,
                            void *d_tags, const void *d_expect_tags, int *d_auth, void *stream) {
    if (!t || (decrypt != 0 && decrypt != 1)) return AESGCM_EARG;
    if (!n_pkts) return AESGCM_OK;
    const bool var = d_data_off != nullptr;
    if (!d_slots || !d_ivs || !d_tags || n_pkts >= ((size_t)1 << 31)) return AESGCM_EARG;
    if (var ? (!d_in || !d_out) : (pkt_len && (!d_in || !d_out))) return AESGCM_EARG;
    if (d_aad_off ? !d_aad : (!var && aad_len && !d_aad)) return AESGCM_EARG;
    if (!var && (pkt_len >= ((size_t)1 << 28) || aad_len >= ((size_t)1 << 28))) return AESGCM_EARG;
    KtParams kp;
    memset(&kp, 0, sizeof kp);
    BatchParams &p = kp.b;
    p.ivs = (const unsigned char *)d_ivs; p.in = (const unsigned char *)d_in; p.out = (unsigned char *)d_out; p.tags = (unsigned char *)d_tags;
    p.expect = (const unsigned char *)d_expect_tags; p.auth = d_auth;
    p.data_off = d_data_off; p.aad_off = d_aad_off;
    if (d_aad_off) p.aad = (const unsigned char *)d_aad;
    else if (!var) { p.aad = aad_len ? (const unsigned char *)d_aad : nullptr; p.aad_len = (u32)aad_len; }
    p.pkt_len = var ? 0u : (u32)pkt_len;
    p.aligned = (var || pkt_len % 16 == 0) && (((uintptr_t)d_in | (uintptr_t)d_out) & 15) == 0;     // offset arrays: and the packet's offset is a multiple of 16
    kp.slots = d_slots; kp.tab = t->tab; kp.n_slots = (u32)t->n_slots; kp.status = t->base.status;
    BatchPlan b;
    const int rc = batch_plan(t->base.device, decrypt, n_pkts, t->key_len, p, stream, b);
    if (rc) return rc;
    HIPCHK(klaunch_kt_batch(b.nr, decrypt, b.lg, b.wgs, b.st, b.tables, kp));
    return batch_done(b, p);
}

// ---------------------------------------------------------------- frames in wire format
int aesgcm_wire_fmt_check(const aesgcm_wire_fmt *f) {
    if (!f) return AESGCM_EARG;
    if (f->salt_len != 0 && f->salt_len != 4 && f->salt_len != 8) return AESGCM_EARG;
    if (f->tag_len != 8 && f->tag_len != 12 && f->tag_len != 16) return AESGCM_EARG;
    if (f->flags & ~AESGCM_WIRE_AUTH_ONLY) return AESGCM_EARG;
    if (f->hdr_len >= (1u << 16) || (!(f->flags & AESGCM_WIRE_AUTH_ONLY) && f->hdr_len < f->aad_len)) return AESGCM_EARG;      // (auth-only: aad_len is ignored)
    if (f->iv_off > f->hdr_len || 12u - f->salt_len > f->hdr_len - f->iv_off) return AESGCM_EARG;       // the nonce's frame bytes end at the payload at the latest
    return AESGCM_OK;
}

// the salts go the way the keys go: through the table's staging buffer on `stream`, from there into the slots (8 bytes each)
int aesgcm_keytab_set_salt(aesgcm_keytab *t, size_t first_slot, size_t n, const uint8_t *salts, void *stream) {
    if (!t) return AESGCM_EARG;
    if (!n) return AESGCM_OK;
    if (!salts || !devtab_in_range(first_slot, n, t->n_slots)) return AESGCM_EARG;
    const KtPart parts[] = {{salts, 8, offsetof(KtSlot, salt)}};
    return kt_set_fields(t, first_slot, n, parts, (hipStream_t)stream);
}

// MACsec XPN's slot state the same way: salts (12 bytes each) and SSCIs (4 each) side by side in the staging buffer, from there into KtSlot::xpn
int aesgcm_keytab_set_xpn(aesgcm_keytab *t, size_t first_slot, size_t n, const uint8_t *salts, const uint8_t *sscis, void *stream) {
    if (!t) return AESGCM_EARG;
    if (!n) return AESGCM_OK;
    if (!salts || !sscis || !devtab_in_range(first_slot, n, t->n_slots)) return AESGCM_EARG;
    const KtPart parts[] = {{salts, 12, offsetof(KtSlot, xpn)}, {sscis, 4, offsetof(KtSlot, xpn) + 12}};
    return kt_set_fields(t, first_slot, n, parts, (hipStream_t)stream);
}

int aesgcm_wire_xfmt_check(const aesgcm_wire_xfmt *xf) {
    if (!xf) return AESGCM_EARG;
    const int frc = aesgcm_wire_fmt_check(&xf->f);
    if (frc) return frc;
    if (xf->reserved || (xf->ext & ~(AESGCM_WIREX_XPN | AESGCM_WIREX_ESN)) || xf->ext == (AESGCM_WIREX_XPN | AESGCM_WIREX_ESN)) return AESGCM_EARG;
    if ((xf->ext & AESGCM_WIREX_XPN) && xf->f.salt_len != 8) return AESGCM_EARG;                // the PN's lower half is the nonce's only frame bytes
    if ((xf->ext & AESGCM_WIREX_ESN) && (xf->f.aad_len != 8 || (xf->f.flags & AESGCM_WIRE_AUTH_ONLY))) return AESGCM_EARG;      // SPI | sequence number, and a payload behind the header
    return AESGCM_OK;
}

// What every call of packets in wire format does behind its own format check (and the pointer checks that the ABI puts in front of the table's): packet p = bytes
// [d_off[p], d_off[p + 1]) of d_in and d_out under slot d_slots[p].  In this order: the common argument checks (table and direction; n == 0 is OK; then the pointers,
// `own_ok` standing for the caller's own); the kernel parameters; the plan, as aesgcm_keytab_crypt_dev's offset-array call (the lengths are on the device: shape by count,
// order by falling frame length class); the launches; batch_done.  `aead(b, xp)` sets what its format adds to xp (w.f, the per-packet numbers) and launches its kernel.
// `mask`, or NULL: the call's second launch on the same stream, a lane per packet (QUIC: header protection; DTLS 1.3: record-number encryption).  Encrypt: the AEAD first,
// then the mask from the fresh ciphertext.  Decrypt: the mask off first -- that kernel leaves the unprotected header in d_out and the decoded numbers in d_pn_out, which is
// where the AEAD reads both.  No scratch memory, no host synchronisation: capture-safe (include/aesgcm.h, CAPTURE; batch_plan never orders a captured call).
struct KtMaskCall {
    hipError_t (*launch)(int nr, int dec, hipStream_t st, const DevTables *tb, const KtQuicHpParams &p);
    const uint32_t *d_hp_slots, *d_pn_off;
    const uint64_t *d_pn;
    uint64_t *d_pn_out;
};
template <class Aead>
static int kt_wire_crypt(aesgcm_keytab *t, int decrypt, size_t n, bool own_ok, const uint32_t *d_slots, const void *d_in, const uint64_t *d_off, void *d_out, int *d_auth,
                         void *stream, const KtMaskCall *mask, Aead aead) {
    if (!t || (decrypt != 0 && decrypt != 1)) return AESGCM_EARG;
    if (!n) return AESGCM_OK;
    if (!own_ok || !d_slots || !d_in || !d_out || !d_off || (decrypt && !d_auth) || n >= ((size_t)1 << 31)) return AESGCM_EARG;
    if (mask && (!mask->d_hp_slots || !mask->d_pn || !mask->d_pn_off || (decrypt && !mask->d_pn_out))) return AESGCM_EARG;
    KtWireXParams xp;
    memset(&xp, 0, sizeof xp);
    BatchParams &p = xp.w.k.b;
    p.in = (const unsigned char *)d_in; p.out = (unsigned char *)d_out;
    p.aad = mask && decrypt ? p.out : p.in;                                      // the AAD: where the header lies unprotected
    p.auth = decrypt ? d_auth : nullptr;
    p.data_off = d_off;
    p.aligned = (((uintptr_t)d_in | (uintptr_t)d_out) & 15) == 0;                // ... and the payload's offset is a multiple of 16 (per packet, in the kernel)
    xp.w.k.slots = d_slots; xp.w.k.tab = t->tab; xp.w.k.n_slots = (u32)t->n_slots; xp.w.k.status = t->base.status;
    KtQuicHpParams m = {};
    if (mask) {
        xp.seq = decrypt ? mask->d_pn_out : mask->d_pn;
        xp.pn_off = mask->d_pn_off; xp.hp_slots = mask->d_hp_slots;
        m.in = p.in; m.out = p.out; m.pkt_off = d_off; m.slots = d_slots; m.hp_slots = mask->d_hp_slots; m.pn_off = mask->d_pn_off;
        m.pn = mask->d_pn; m.pn_out = decrypt ? mask->d_pn_out : nullptr; m.tab = t->tab; m.n_pkts = (u32)n; m.n_slots = (u32)t->n_slots;
    }
    BatchPlan b;
    const int rc = batch_plan(t->base.device, decrypt, n, t->key_len, p, stream, b);
    if (rc) return rc;
    if (mask && decrypt) HIPCHK(mask->launch(b.nr, 1, b.st, b.tables, m));
    HIPCHK(aead(b, xp));
    if (mask && !decrypt) HIPCHK(mask->launch(b.nr, 0, b.st, b.tables, m));
    return batch_done(b, p);
}

// frame p laid out by *fmt: one k_kt_wire launch
int aesgcm_keytab_frames_crypt_dev(aesgcm_keytab *t, int decrypt, const aesgcm_wire_fmt *fmt, size_t n_frames, const uint32_t *d_slots, const void *d_in,
                                   const uint64_t *d_frame_off, void *d_out, int *d_auth, void *stream) {
    const int frc = aesgcm_wire_fmt_check(fmt);
    if (frc) return frc;
    return kt_wire_crypt(t, decrypt, n_frames, true, d_slots, d_in, d_frame_off, d_out, d_auth, stream, nullptr, [&](const BatchPlan &b, KtWireXParams &xp) {
        xp.w.f = *fmt;
        return klaunch_kt_wire(b.nr, decrypt, b.lg, b.wgs, b.st, b.tables, xp.w);
    });
}

// ... with hi[p], the half of frame p's 64-bit number that is not on the wire (MACsec XPN: into the nonce; ESP ESN: into the AAD): one k_kt_wirex launch.  ext 0 is the
// call above.
int aesgcm_keytab_frames_crypt_x_dev(aesgcm_keytab *t, int decrypt, const aesgcm_wire_xfmt *xf, size_t n_frames, const uint32_t *d_slots, const uint32_t *d_hi,
                                     const void *d_in, const uint64_t *d_frame_off, void *d_out, int *d_auth, void *stream) {
    const int frc = aesgcm_wire_xfmt_check(xf);
    if (frc) return frc;
    if (xf->ext && !d_hi) return AESGCM_EARG;
    return kt_wire_crypt(t, decrypt, n_frames, true, d_slots, d_in, d_frame_off, d_out, d_auth, stream, nullptr, [&](const BatchPlan &b, KtWireXParams &xp) {
        xp.w.f = xf->f;
        if (!xf->ext) return klaunch_kt_wire(b.nr, decrypt, b.lg, b.wgs, b.st, b.tables, xp.w);
        xp.hi = d_hi;
        return klaunch_kt_wirex(xf->ext, b.nr, decrypt, b.lg, b.wgs, b.st, b.tables, xp);
    });
}

// ---------------------------------------------------------------- TLS records
int aesgcm_tls_fmt_check(const aesgcm_tls_fmt *f) {
    if (!f || (f->version != AESGCM_TLS_13 && f->version != AESGCM_TLS_12) || f->reserved) return AESGCM_EARG;
    return AESGCM_OK;
}

// a connection direction's 12-byte write IV into KtSlot::xpn, the way aesgcm_keytab_set_xpn's salts go; the word behind it (there: the SSCI) becomes zero
int aesgcm_keytab_set_tls_iv(aesgcm_keytab *t, size_t first_slot, size_t n, const uint8_t *ivs, void *stream) {
    if (!t) return AESGCM_EARG;
    if (!n) return AESGCM_OK;
    if (!ivs || !devtab_in_range(first_slot, n, t->n_slots)) return AESGCM_EARG;
    const KtPart parts[] = {{ivs, 12, offsetof(KtSlot, xpn)}, {nullptr, 4, offsetof(KtSlot, xpn) + 12}};
    return kt_set_fields(t, first_slot, n, parts, (hipStream_t)stream);
}

// One k_kt_tls launch: record p = bytes [d_rec_off[p], d_rec_off[p + 1]) of d_in and d_out.  The kernel runs k_kt_wire's loop; what it takes from a wire format
// (header length, where the explicit nonce lies, the tag's length) is the version's constant format here
int aesgcm_keytab_records_crypt_dev(aesgcm_keytab *t, int decrypt, const aesgcm_tls_fmt *fmt, size_t n_recs, const uint32_t *d_slots, const uint64_t *d_seq,
                                    const void *d_in, const uint64_t *d_rec_off, void *d_out, int *d_auth, void *stream) {
    const int frc = aesgcm_tls_fmt_check(fmt);
    if (frc) return frc;
    if (!d_seq) return AESGCM_EARG;
    static const aesgcm_wire_fmt f13 = {5, 5, 5, 0, 16, 0}, f12 = {13, 13, 5, 4, 16, 0};          // {aad_len, hdr_len, iv_off, salt_len, tag_len, flags}
    return kt_wire_crypt(t, decrypt, n_recs, true, d_slots, d_in, d_rec_off, d_out, d_auth, stream, nullptr, [&](const BatchPlan &b, KtWireXParams &xp) {
        xp.w.f = fmt->version == AESGCM_TLS_13 ? f13 : f12;
        xp.seq = d_seq;
        return klaunch_kt_tls(fmt->version, b.nr, decrypt, b.lg, b.wgs, b.st, b.tables, xp);
    });
}

// ---------------------------------------------------------------- QUIC packets
// Two launches: the AEAD (k_kt_quic) and header protection (k_kt_quic_hp), in kt_wire_crypt's order
int aesgcm_keytab_quic_crypt_dev(aesgcm_keytab *t, int decrypt, size_t n_pkts, const uint32_t *d_slots, const uint32_t *d_hp_slots, const uint64_t *d_pn, uint64_t *d_pn_out,
                                 const uint32_t *d_pn_off, const void *d_in, const uint64_t *d_pkt_off, void *d_out, int *d_auth, void *stream) {
    const KtMaskCall hp = {klaunch_kt_quic_hp, d_hp_slots, d_pn_off, d_pn, d_pn_out};
    return kt_wire_crypt(t, decrypt, n_pkts, true, d_slots, d_in, d_pkt_off, d_out, d_auth, stream, &hp, [&](const BatchPlan &b, KtWireXParams &xp) {
        xp.w.f.tag_len = 16;                                                          // the rest of a wire format is per packet here
        return klaunch_kt_quic(b.nr, decrypt, b.lg, b.wgs, b.st, b.tables, xp);
    });
}

// ---------------------------------------------------------------- DTLS records
int aesgcm_dtls_fmt_check(const aesgcm_dtls_fmt *f) {
    if (!f || (f->version != AESGCM_DTLS_13 && f->version != AESGCM_DTLS_12) || f->reserved) return AESGCM_EARG;
    return AESGCM_OK;
}

// 1.2: one k_kt_dtls launch; what the kernel takes from a wire format is the version's constant format.  1.3: the QUIC call's two launches, the second k_kt_dtls_sn
// (record-number encryption)
int aesgcm_keytab_dtls_crypt_dev(aesgcm_keytab *t, int decrypt, const aesgcm_dtls_fmt *fmt, size_t n_recs, const uint32_t *d_slots, const uint32_t *d_sn_slots,
                                 const uint64_t *d_seq, uint64_t *d_seq_out, const uint32_t *d_sn_off, const void *d_in, const uint64_t *d_rec_off, void *d_out, int *d_auth,
                                 void *stream) {
    const int frc = aesgcm_dtls_fmt_check(fmt);
    if (frc) return frc;
    const bool v13 = fmt->version == AESGCM_DTLS_13;
    const KtMaskCall sn = {klaunch_kt_dtls_sn, d_sn_slots, d_sn_off, d_seq, d_seq_out};
    static const aesgcm_wire_fmt f12 = {13, 21, 13, 4, 16, 0};                        // {aad_len, hdr_len, iv_off, salt_len, tag_len, flags}
    return kt_wire_crypt(t, decrypt, n_recs, true, d_slots, d_in, d_rec_off, d_out, d_auth, stream, v13 ? &sn : nullptr, [&](const BatchPlan &b, KtWireXParams &xp) {
        if (v13) xp.w.f.tag_len = 16;                                                 // the rest of a wire format is per record here
        else xp.w.f = f12;
        return klaunch_kt_dtls(fmt->version, b.nr, decrypt, b.lg, b.wgs, b.st, b.tables, xp);
    });
}

// ---------------------------------------------------------------- SRTP and SRTCP packets
int aesgcm_srtp_fmt_check(const aesgcm_srtp_fmt *f) {
    if (!f || (f->kind != AESGCM_SRTP_RTP && f->kind != AESGCM_SRTP_RTCP) || f->mki_len > 128u) return AESGCM_EARG;
    return AESGCM_OK;
}

// One k_kt_srtp launch: everything the kernel needs beside the rollover counters and the MKI's length is in the packet
int aesgcm_keytab_srtp_crypt_dev(aesgcm_keytab *t, int decrypt, const aesgcm_srtp_fmt *fmt, size_t n_pkts, const uint32_t *d_slots, const uint32_t *d_roc, const void *d_in,
                                 const uint64_t *d_pkt_off, void *d_out, int *d_auth, void *stream) {
    const int frc = aesgcm_srtp_fmt_check(fmt);
    if (frc) return frc;
    const bool rtp = fmt->kind == AESGCM_SRTP_RTP;
    return kt_wire_crypt(t, decrypt, n_pkts, !rtp || d_roc, d_slots, d_in, d_pkt_off, d_out, d_auth, stream, nullptr, [&](const BatchPlan &b, KtWireXParams &xp) {
        xp.w.f.tag_len = 16;                                                          // the rest of a wire format is per packet here
        xp.hi = rtp ? d_roc : nullptr;
        xp.mki_len = fmt->mki_len;
        return klaunch_kt_srtp(fmt->kind, b.nr, decrypt, b.lg, b.wgs, b.st, b.tables, xp);
    });
}

// ---------------------------------------------------------------- SSH binary packets
// One k_kt_ssh launch, planned as a TLS call: the packet's cut and its nonce are the kernel's (cut_ssh, nonce_iv_add_num); of a wire format it takes the tag's length and,
// for the bytes that pass through out of place, the four length bytes in front of the body.
// A library made of the host units alone (tests/fake_hip links them against a fake runtime whose launcher list is fixed) has no launcher for this family: the one
// below is the weak one, as aesgcm_prfplus.hip's are, and the call fails there with AESGCM_EHIP behind its argument checks and its plan; in the product the kernels'
// object defines the strong one
__attribute__((weak)) hipError_t klaunch_kt_ssh(int, int, int, unsigned, hipStream_t, const DevTables *, const KtWireXParams &) { return hipErrorNotSupported; }

int aesgcm_keytab_ssh_crypt_dev(aesgcm_keytab *t, int decrypt, size_t n_pkts, const uint32_t *d_slots, const uint64_t *d_seq, const void *d_in, const uint64_t *d_pkt_off,
                                void *d_out, int *d_auth, void *stream) {
    if (!d_seq) return AESGCM_EARG;
    static const aesgcm_wire_fmt f = {4, 4, 4, 0, 16, 0};                             // {aad_len, hdr_len, iv_off, salt_len, tag_len, flags}
    return kt_wire_crypt(t, decrypt, n_pkts, true, d_slots, d_in, d_pkt_off, d_out, d_auth, stream, nullptr, [&](const BatchPlan &b, KtWireXParams &xp) {
        xp.w.f = f;
        xp.seq = d_seq;
        return klaunch_kt_ssh(b.nr, decrypt, b.lg, b.wgs, b.st, b.tables, xp);
    });
}

int aesgcm_keytab_status(aesgcm_keytab *t, int *code, uint64_t *detail) {
    if (!t || !code) return AESGCM_EARG;
    return devtab_status(&t->base, code, detail);
}

int aesgcm_keytab_destroy(aesgcm_keytab *t) {
    if (!t) return AESGCM_OK;
    const int rc = devtab_destroy(&t->base, t->tab, t->n_slots * sizeof(KtSlot), "aesgcm_keytab_destroy");      // the slots and the stage wiped: both held key material
    delete t;
    return rc;
}
