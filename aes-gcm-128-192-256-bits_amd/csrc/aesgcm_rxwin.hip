// aesgcm_rxwin.hip -- receive windows (include/aesgcm.h "RECEIVE WINDOWS"): the host side of aesgcm_rxwin_*.  The kernels are in aesgcm_rxwin_kernels.hip, the lane code and
// the layout of the state in aesgcm_rxwin.h.  A table is one device allocation of n_wins window records and a status word.  Host state reaches the records through the
// table's staging buffer, as a key table's keys do; aesgcm_rxwin_get copies records back and waits.  The normalised form of set / get and the records' ring are converted
// into one another here, on the host (rx_norm_to_ring, rx_ring_to_norm).  recover is one launch, commit three; neither synchronises or allocates: capture-safe (include/aesgcm.h, CAPTURE).
#include "aesgcm_internal.h"
#include "aesgcm_rxwin.h"

#include <string.h>

struct aesgcm_rxwin {
    int device = 0;
    RxTable t = {};
    unsigned char *stage = nullptr;    // device: records wait here for their copy into the state
    size_t stage_cap = 0;
    hipEvent_t stage_done = nullptr;   // behind the last copy out of `stage`, on whichever stream it ran
    std::mutex mu;
};

int aesgcm_rxwin_create(aesgcm_rxwin **out, int device, size_t n_wins, size_t window) {
    if (!out) return AESGCM_EARG;
    *out = nullptr;
    if (window < 64 || window > 4096 || (window & (window - 1)) || !n_wins || n_wins >= ((size_t)1 << 31)) return AESGCM_EARG;
    DeviceState *ds;
    int rc = device_state(device, &ds);            // (AESGCM_EHIP without a device)
    if (rc) return rc;
    HIPCHK(hipSetDevice(device));
    aesgcm_rxwin *w = new aesgcm_rxwin();
    w->device = device;
    w->t.n_wins = (u32)n_wins; w->t.window = (u32)window; w->t.stride = rx_stride_words((u32)window);
    const size_t bytes = n_wins * w->t.stride * sizeof(u64);
    hipError_t e = hipMalloc((void **)&w->t.state, bytes);
    if (e == hipSuccess) e = hipMalloc((void **)&w->t.status, sizeof(u32));
    if (e == hipSuccess) e = hipMemset(w->t.state, 0, bytes);
    if (e == hipSuccess) e = hipMemset(w->t.status, 0xFF, sizeof(u32));
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) {
        if (w->t.state) (void)hipFree(w->t.state);
        if (w->t.status) (void)hipFree(w->t.status);
        delete w;
        return e == hipErrorOutOfMemory ? AESGCM_ENOMEM : hip_fail(e, "aesgcm_rxwin_create");
    }
    *out = w;
    return AESGCM_OK;
}

int aesgcm_rxwin_set(aesgcm_rxwin *w, size_t first, size_t n, const uint64_t *next, const uint64_t *seen, void *stream) {
    if (!w) return AESGCM_EARG;
    if (!n) return AESGCM_OK;
    if (!next || first >= w->t.n_wins || n > w->t.n_wins - first) return AESGCM_EARG;
    const u32 W = w->t.window, stride = w->t.stride, sw = W / 64u;
    for (size_t k = 0; k < n; k++) if (!rx_norm_valid(next[k], seen ? seen + k * sw : nullptr, W)) return AESGCM_EARG;      // a bit for a number below 0
    hipStream_t st = (hipStream_t)stream;
    std::vector<u64> rec(n * stride, 0);
    for (size_t k = 0; k < n; k++) {
        u64 *r = rec.data() + k * stride;
        r[0] = r[1] = next[k];
        rx_norm_to_ring(next[k], seen ? seen + k * sw : nullptr, W, r + RX_HDR_WORDS);
    }
    const size_t bytes = rec.size() * sizeof(u64);
    std::lock_guard<std::mutex> lk(w->mu);
    HIPCHK(hipSetDevice(w->device));
    if (bytes > w->stage_cap) {
        if (w->stage) { HIPCHK(hipFree(w->stage)); w->stage = nullptr; w->stage_cap = 0; }   // hipFree waits for the copies that may still read it
        const hipError_t e = hipMalloc((void **)&w->stage, bytes);
        if (e == hipErrorOutOfMemory) return AESGCM_ENOMEM;
        if (e != hipSuccess) return hip_fail(e, "hipMalloc");
        w->stage_cap = bytes;
    }
    if (!w->stage_done) HIPCHK(hipEventCreateWithFlags(&w->stage_done, hipEventDisableTiming));
    else HIPCHK(hipStreamWaitEvent(st, w->stage_done, 0));
    HIPCHK(hipMemcpyAsync(w->stage, rec.data(), bytes, hipMemcpyHostToDevice, st));      // (pageable memory: copied out of `rec` when the call returns)
    HIPCHK(hipMemcpyAsync(w->t.state + first * stride, w->stage, bytes, hipMemcpyDeviceToDevice, st));
    HIPCHK(hipEventRecord(w->stage_done, st));
    return AESGCM_OK;
}

int aesgcm_rxwin_get(aesgcm_rxwin *w, size_t first, size_t n, uint64_t *next, uint64_t *seen, void *stream) {
    if (!w) return AESGCM_EARG;
    if (!n) return AESGCM_OK;
    if (!next || first >= w->t.n_wins || n > w->t.n_wins - first) return AESGCM_EARG;
    const u32 W = w->t.window, stride = w->t.stride, sw = W / 64u;
    hipStream_t st = (hipStream_t)stream;
    std::vector<u64> rec(n * stride);
    HIPCHK(hipSetDevice(w->device));
    HIPCHK(hipMemcpyAsync(rec.data(), w->t.state + first * stride, rec.size() * sizeof(u64), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
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
    HIPCHK(hipSetDevice(w->device));
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
    HIPCHK(hipSetDevice(w->device));
    HIPCHK(klaunch_rxwin_commit((hipStream_t)stream, c));
    return AESGCM_OK;
}

int aesgcm_rxwin_status(aesgcm_rxwin *w, int *code, uint64_t *detail) {
    if (!w || !code) return AESGCM_EARG;
    HIPCHK(hipSetDevice(w->device));
    u32 v = ~0u;
    HIPCHK(hipMemcpy(&v, w->t.status, sizeof v, hipMemcpyDeviceToHost));
    *code = v == ~0u ? AESGCM_OK : AESGCM_EARG;
    if (detail) *detail = v == ~0u ? 0 : v;
    if (v != ~0u) HIPCHK(hipMemset(w->t.status, 0xFF, sizeof(u32)));
    return AESGCM_OK;
}

int aesgcm_rxwin_destroy(aesgcm_rxwin *w) {
    if (!w) return AESGCM_OK;
    int rc = AESGCM_OK;
    hipError_t e = hipSetDevice(w->device);
    if (e == hipSuccess) e = hipDeviceSynchronize();                       // calls in flight may still use the records
    if (e != hipSuccess) rc = hip_fail(e, "aesgcm_rxwin_destroy");
    (void)hipFree(w->t.state);
    (void)hipFree(w->t.status);
    if (w->stage) (void)hipFree(w->stage);
    if (w->stage_done) (void)hipEventDestroy(w->stage_done);
    delete w;
    return rc;
}
