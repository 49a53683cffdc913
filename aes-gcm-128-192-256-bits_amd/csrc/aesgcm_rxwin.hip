// aesgcm_rxwin.hip -- receive windows (include/aesgcm.h "RECEIVE WINDOWS"): the host side of aesgcm_rxwin_*.  The kernels are in aesgcm_rxwin_kernels.hip, the lane code and
// the layout of the state in aesgcm_rxwin.h.  A table is a DevTable (aesgcm_internal.h: create, put, get, status, destroy, the range check; defined in
// aesgcm_host.hip) whose state is n_wins window records.  Host state reaches the records through the staging buffer (devtab_put), which is not zeroed behind a set and
// not wiped by destroy (it holds numbers, no keys); aesgcm_rxwin_get copies records back and waits (devtab_get).  The normalised form of set / get and the records' ring are converted
// into one another here, on the host (rx_norm_to_ring, rx_ring_to_norm).  recover is one launch, commit three; neither synchronises or allocates: capture-safe (include/aesgcm.h, CAPTURE).
#include "aesgcm_internal.h"
#include "aesgcm_rxwin.h"

#include <string.h>

struct aesgcm_rxwin {
    DevTable base;                     // base.stage: records wait there for their copy into the state; base.stage_done: behind the last such copy
    RxTable t = {};                    // t.status == base.status: the kernels' copy of the pointer
};

int aesgcm_rxwin_create(aesgcm_rxwin **out, int device, size_t n_wins, size_t window) {
    if (!out) return AESGCM_EARG;
    *out = nullptr;
    if (window < 64 || window > 4096 || (window & (window - 1)) || !n_wins || n_wins >= ((size_t)1 << 31)) return AESGCM_EARG;
    aesgcm_rxwin *w = new aesgcm_rxwin();
    w->t.n_wins = (u32)n_wins; w->t.window = (u32)window; w->t.stride = rx_stride_words((u32)window);
    const int rc = devtab_create(&w->base, device, n_wins * w->t.stride * sizeof(u64), (void **)&w->t.state, "aesgcm_rxwin_create");
    if (rc) { delete w; return rc; }
    w->t.status = w->base.status;
    *out = w;
    return AESGCM_OK;
}

int aesgcm_rxwin_set(aesgcm_rxwin *w, size_t first, size_t n, const uint64_t *next, const uint64_t *seen, void *stream) {
    if (!w) return AESGCM_EARG;
    if (!n) return AESGCM_OK;
    if (!next || !devtab_in_range(first, n, w->t.n_wins)) return AESGCM_EARG;
    const u32 W = w->t.window, stride = w->t.stride, sw = W / 64u;
    for (size_t k = 0; k < n; k++) if (!rx_norm_valid(next[k], seen ? seen + k * sw : nullptr, W)) return AESGCM_EARG;      // a bit for a number below 0
    std::vector<u64> rec(n * stride, 0);
    for (size_t k = 0; k < n; k++) {
        u64 *r = rec.data() + k * stride;
        r[0] = r[1] = next[k];
        rx_norm_to_ring(next[k], seen ? seen + k * sw : nullptr, W, r + RX_HDR_WORDS);
    }
    return devtab_put(&w->base, w->t.state + first * stride, rec.data(), rec.size() * sizeof(u64), (hipStream_t)stream, false);
}

int aesgcm_rxwin_get(aesgcm_rxwin *w, size_t first, size_t n, uint64_t *next, uint64_t *seen, void *stream) {
    if (!w) return AESGCM_EARG;
    if (!n) return AESGCM_OK;
    if (!next || !devtab_in_range(first, n, w->t.n_wins)) return AESGCM_EARG;
    const u32 W = w->t.window, stride = w->t.stride, sw = W / 64u;
    std::vector<u64> rec(n * stride);
    const int rc = devtab_get(&w->base, rec.data(), w->t.state + first * stride, rec.size() * sizeof(u64), (hipStream_t)stream);
    if (rc) return rc;
    for (size_t k = 0; k < n; k++) {
        const u64 *r = rec.data() + k * stride;
        next[k] = r[0];
        if (seen) rx_ring_to_norm(r[0], r + RX_HDR_WORDS, W, seen + k * sw);
    }
    return AESGCM_OK;
}

int aesgcm_rxwin_fmt_check(const aesgcm_rxwin_fmt *f) {
    if (!f || f->num_off >= (1u << 16)) return AESGCM_EARG;
    const u32 L = f->num_len;
    switch (f->rule) {
    case AESGCM_RXWIN_WIRE:
        if ((L != 2 && L != 4 && L != 6 && L != 8) || (f->flags & ~(AESGCM_RXWIN_FROM_END | AESGCM_RXWIN_CLEAR_TOP))) return AESGCM_EARG;
        return AESGCM_OK;
    case AESGCM_RXWIN_LOWEST:
        return ((L != 2 && L != 4) || f->flags) ? AESGCM_EARG : AESGCM_OK;
    case AESGCM_RXWIN_SRTP:
        return (L != 2 || f->flags) ? AESGCM_EARG : AESGCM_OK;
    case AESGCM_RXWIN_EXPECT:
        return (L != 0 || f->flags) ? AESGCM_EARG : AESGCM_OK;
    default:
        return AESGCM_EARG;
    }
}

int aesgcm_rxwin_recover_dev(aesgcm_rxwin *w, const aesgcm_rxwin_fmt *fmt, size_t n_pkts, const uint32_t *d_win, const void *d_in, const uint64_t *d_pkt_off,
                             uint64_t *d_num_out, uint32_t *d_hi_out, void *stream) {
    const int frc = aesgcm_rxwin_fmt_check(fmt);
    if (frc) return frc;
    if (!w) return AESGCM_EARG;
    if (!n_pkts) return AESGCM_OK;
    const bool bytes = fmt->rule != AESGCM_RXWIN_EXPECT;
    if (!d_win || !d_num_out || (bytes && (!d_in || !d_pkt_off)) || n_pkts >= ((size_t)1 << 31)) return AESGCM_EARG;
    RxRecoverParams q;
    memset(&q, 0, sizeof q);
    q.t = w->t; q.f = *fmt; q.win = d_win; q.in = (const unsigned char *)d_in; q.pkt_off = d_pkt_off; q.num_out = d_num_out; q.hi_out = d_hi_out; q.n_pkts = (u32)n_pkts;
    HIPCHK(hipSetDevice(w->base.device));
    HIPCHK(klaunch_rxwin_recover((hipStream_t)stream, q));
    return AESGCM_OK;
}

int aesgcm_rxwin_commit_dev(aesgcm_rxwin *w, size_t n_pkts, const uint32_t *d_win, const uint64_t *d_num, const int *d_auth, int *d_accept, int *d_why, void *stream) {
    if (!w) return AESGCM_EARG;
    if (!n_pkts) return AESGCM_OK;
    if (!d_win || !d_num || !d_auth || !d_accept || n_pkts >= ((size_t)1 << 31)) return AESGCM_EARG;
    RxCommitParams c;
    memset(&c, 0, sizeof c);
    c.t = w->t; c.win = d_win; c.num = d_num; c.auth = d_auth; c.accept = d_accept; c.why = d_why; c.n_pkts = (u32)n_pkts;
    HIPCHK(hipSetDevice(w->base.device));
    HIPCHK(klaunch_rxwin_commit((hipStream_t)stream, c));
    return AESGCM_OK;
}

int aesgcm_rxwin_status(aesgcm_rxwin *w, int *code, uint64_t *detail) {
    if (!w || !code) return AESGCM_EARG;
    return devtab_status(&w->base, code, detail);
}

int aesgcm_rxwin_destroy(aesgcm_rxwin *w) {
    if (!w) return AESGCM_OK;
    const int rc = devtab_destroy(&w->base, w->t.state, 0, "aesgcm_rxwin_destroy");      // (nothing wiped: numbers, no keys)
    delete w;
    return rc;
}
