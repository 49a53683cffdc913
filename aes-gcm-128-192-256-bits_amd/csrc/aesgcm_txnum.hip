// aesgcm_txnum.hip -- send counters (include/aesgcm.h "SEND COUNTERS"): the host side of aesgcm_txnum_*.  The kernels are in aesgcm_txnum_kernels.hip, the lane code and
// the layout of the state in aesgcm_txnum.h.  A table is a DevTable (aesgcm_internal.h: create, put, get, status, destroy, the range check; defined in
// aesgcm_host.hip) whose state is ONE allocation: n_ctrs counter records, then the scratch of an assign call -- the sort's TX_ENTRIES counts and its one or two
// arrays of max_pkts packet indices -- so that a call allocates nothing.  Host state reaches the records through the staging buffer (devtab_put), which is not zeroed behind
// a set and not wiped by destroy (it holds numbers, no keys); aesgcm_txnum_get copies records back and waits (devtab_get).  assign is 3 * passes + 2 launches on the caller's stream; it neither synchronises nor
// allocates nor reads anything back: capture-safe (include/aesgcm.h, CAPTURE).
#include "aesgcm_internal.h"
#include "aesgcm_txnum.h"

#include <string.h>

struct aesgcm_txnum {
    DevTable base;                     // base.stage: records wait there for their copy into the state; base.stage_done: behind the last such copy
    TxTable t = {};                    // t.status == base.status: the kernels' copy of the pointer
    void *state = nullptr;             // the allocation: t.rec | t.counts | t.idx[0] | t.idx[1]
};

int aesgcm_txnum_create(aesgcm_txnum **out, int device, size_t n_ctrs, size_t max_pkts) {
    if (!out) return AESGCM_EARG;
    *out = nullptr;
    if (!n_ctrs || n_ctrs >= ((size_t)1 << 31) || !max_pkts || max_pkts >= ((size_t)1 << 31)) return AESGCM_EARG;
    aesgcm_txnum *c = new aesgcm_txnum();
    c->t.n_ctrs = (u32)n_ctrs; c->t.max_pkts = (u32)max_pkts; c->t.passes = tx_passes((u32)n_ctrs);
    const size_t rec_bytes = n_ctrs * TX_REC_WORDS * sizeof(u64), cnt_bytes = (size_t)TX_ENTRIES * sizeof(u32), idx_bytes = (max_pkts * sizeof(u32) + 15u) & ~(size_t)15u;
    const int rc = devtab_create(&c->base, device, rec_bytes + cnt_bytes + (c->t.passes > 1u ? 2u : 1u) * idx_bytes, &c->state, "aesgcm_txnum_create");
    if (rc) { delete c; return rc; }
    unsigned char *at = (unsigned char *)c->state;
    c->t.rec = (u64 *)at; at += rec_bytes;                 // (rec_bytes is a multiple of 32: the counts stay 16-byte aligned for k_tx_scan)
    c->t.counts = (u32 *)at; at += cnt_bytes;
    c->t.idx[0] = (u32 *)at; at += idx_bytes;
    c->t.idx[1] = c->t.passes > 1u ? (u32 *)at : nullptr;
    c->t.status = c->base.status;
    *out = c;
    return AESGCM_OK;
}

int aesgcm_txnum_set(aesgcm_txnum *c, size_t first, size_t n, const uint64_t *next, const uint64_t *limit, void *stream) {
    if (!c) return AESGCM_EARG;
    if (!n) return AESGCM_OK;
    if (!next || !limit || !devtab_in_range(first, n, c->t.n_ctrs)) return AESGCM_EARG;
    for (size_t k = 0; k < n; k++) if (next[k] > limit[k]) return AESGCM_EARG;
    std::vector<u64> rec(n * TX_REC_WORDS, 0);
    for (size_t k = 0; k < n; k++) { rec[k * TX_REC_WORDS] = next[k]; rec[k * TX_REC_WORDS + 1] = limit[k]; }
    return devtab_put(&c->base, c->t.rec + first * TX_REC_WORDS, rec.data(), rec.size() * sizeof(u64), (hipStream_t)stream, false);
}

int aesgcm_txnum_get(aesgcm_txnum *c, size_t first, size_t n, uint64_t *next, uint64_t *limit, void *stream) {
    if (!c) return AESGCM_EARG;
    if (!n) return AESGCM_OK;
    if (!next || !devtab_in_range(first, n, c->t.n_ctrs)) return AESGCM_EARG;
    std::vector<u64> rec(n * TX_REC_WORDS);
    const int rc = devtab_get(&c->base, rec.data(), c->t.rec + first * TX_REC_WORDS, rec.size() * sizeof(u64), (hipStream_t)stream);
    if (rc) return rc;
    for (size_t k = 0; k < n; k++) {
        next[k] = rec[k * TX_REC_WORDS];
        if (limit) limit[k] = rec[k * TX_REC_WORDS + 1];
    }
    return AESGCM_OK;
}

int aesgcm_txnum_fmt_check(const aesgcm_txnum_fmt *f) {
    if (!f || f->num_off >= (1u << 16) || f->dup_off >= (1u << 16)) return AESGCM_EARG;
    if (f->flags & ~(AESGCM_TXNUM_FROM_END | AESGCM_TXNUM_KEEP_TOP | AESGCM_TXNUM_WHOLE)) return AESGCM_EARG;
    const u32 L = f->num_len;
    if (L == 0) return (f->dup_off || (f->flags & (AESGCM_TXNUM_KEEP_TOP | AESGCM_TXNUM_WHOLE))) ? AESGCM_EARG : AESGCM_OK;      // nothing is written: nothing to keep, to fit or to repeat
    if (L != 2 && L != 4 && L != 6 && L != 8) return AESGCM_EARG;
    if (f->dup_off && (f->dup_off > f->num_off ? f->dup_off - f->num_off : f->num_off - f->dup_off) < L) return AESGCM_EARG;      // the duplicate overlaps the field
    return AESGCM_OK;
}

int aesgcm_txnum_assign_dev(aesgcm_txnum *c, const aesgcm_txnum_fmt *fmt, size_t n_pkts, const uint32_t *d_ctr, void *d_pkts, const uint64_t *d_pkt_off,
                            uint64_t *d_num_out, uint32_t *d_hi_out, uint32_t *d_slots, void *stream) {
    const int frc = aesgcm_txnum_fmt_check(fmt);
    if (frc) return frc;
    if (!c) return AESGCM_EARG;
    if (!n_pkts) return AESGCM_OK;
    if (!d_ctr || !d_num_out || (fmt->num_len && (!d_pkts || !d_pkt_off)) || n_pkts >= ((size_t)1 << 31) || n_pkts > c->t.max_pkts) return AESGCM_EARG;      // (the table is looked at last)
    TxAssignParams q;
    memset(&q, 0, sizeof q);
    q.t = c->t; q.f = *fmt; q.ctr = d_ctr; q.pkts = (unsigned char *)d_pkts; q.pkt_off = d_pkt_off; q.num_out = d_num_out; q.hi_out = d_hi_out; q.slots = d_slots;
    q.n_pkts = (u32)n_pkts;
    HIPCHK(hipSetDevice(c->base.device));
    HIPCHK(klaunch_txnum_assign((hipStream_t)stream, q));
    return AESGCM_OK;
}

int aesgcm_txnum_status(aesgcm_txnum *c, int *code, uint64_t *detail) {
    if (!c || !code) return AESGCM_EARG;
    return devtab_status(&c->base, code, detail);
}

int aesgcm_txnum_destroy(aesgcm_txnum *c) {
    if (!c) return AESGCM_OK;
    const int rc = devtab_destroy(&c->base, c->state, 0, "aesgcm_txnum_destroy");        // (nothing wiped: numbers, no keys)
    delete c;
    return rc;
}
