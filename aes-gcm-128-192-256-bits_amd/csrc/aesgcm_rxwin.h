// aesgcm_rxwin.h -- receive windows (aesgcm_rxwin_*, include/aesgcm.h "RECEIVE WINDOWS"): anti-replay and the recovery of a packet's full number, a lane per packet.
// Shared by the kernels (aesgcm_rxwin_kernels.hip), the host side (aesgcm_rxwin.hip) and the CPU harness tests/rxwin_emul, which runs the lane functions below phase by
// phase with the lanes in shuffled orders: everything a lane does is here, HD; the kernels only hand out lane numbers.
//
// STATE.  n_wins records of rx_stride_words(window) 64-bit words, 64 bytes apart or a multiple (two windows never share a 64-byte atomic request):
//   word 0        next      the highest accepted number + 1, 0 = nothing accepted yet
//   word 1        next_new  the commit's running maximum; equals `next` between calls
//   words 2 ..    ring      window / 64 words: number n has bit n mod window, (n mod window) / 64 its word.  Between calls a set bit stands for a seen number of
//                           [next - window, next); the positions of numbers below 0 (next < window) are zero
// A COMMIT is three launches behind one another on the caller's stream (S = the call's packets with auth != 0, a window in range and a number):
//   1  rx_commit_max_lane    next_new = max(next_new, num + 1) over S, a 64-bit atomic max behind a filter (a lane whose number is not above what it reads there skips it)
//   2  rx_commit_clear_lane  M = next_new is final.  Every lane that holds it (num + 1 == M) clears the ring positions of [next, M), all of them when M - next >= window:
//                            the same words and masks from each such lane, so any number of them may run in any order
//   3  rx_commit_mark_lane   old if M - num > window; otherwise a 64-bit atomic OR of the number's bit, and the word that comes back says replay (bit set: seen before the
//                            call, or another lane of this call was first) or accept.  The maximum's holders store next = M
// Between the phases lies a kernel boundary; inside a phase lanes meet only in agent-scope atomics, and every write to a window's words inside a kernel is one (the ring's
// clearing and `next` included): no plain store shares a line with an atomic that another compute die executes at the memory side.
// A RECOVER (rx_recover_lane) is one launch and writes no state.
#pragma once
#include "aesgcm_base.h"
#include "../../include/aesgcm.h"

#define RX_HDR_WORDS 2u
#define RX_WG 256u
HD u32 rx_stride_words(u32 window) { return (RX_HDR_WORDS + window / 64u + 7u) & ~7u; }

struct RxTable {
    u64 *state;                            // n_wins records
    u32 *status;                           // lowest refused packet (atomic min), ~0 = none
    u32 n_wins, window, stride;            // stride = rx_stride_words(window)
};

struct RxRecoverParams {
    RxTable t;
    aesgcm_rxwin_fmt f;                    // checked by aesgcm_rxwin_fmt_check
    const u32 *win;                        // n_pkts window numbers
    const unsigned char *in;               // the packets; unused by AESGCM_RXWIN_EXPECT
    const u64 *pkt_off;                    // n_pkts + 1 offsets; unused by AESGCM_RXWIN_EXPECT
    u64 *num_out;
    u32 *hi_out;                           // or NULL
    u32 n_pkts;
};

struct RxCommitParams {
    RxTable t;
    const u32 *win;
    const u64 *num;
    const int *auth;
    int *accept;                           // may be auth: a lane reads its auth before it writes its accept, and only phase 3 writes
    int *why;                              // or NULL
    u32 n_pkts;
};

#define RX_WHY_NOAUTH 0
#define RX_WHY_ACCEPT 1
#define RX_WHY_OLD 2
#define RX_WHY_REPLAY 3
#define RX_WHY_REFUSED 4

// ---------------------------------------------------------------- the atomics: agent scope on the device; the host harness runs one lane after another
HD u64 rx_fetch_max(u64 *p, u64 v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return atomicMax((unsigned long long *)p, (unsigned long long)v);
#else
    const u64 o = *p; if (v > o) *p = v; return o;
#endif
}
HD u64 rx_fetch_or(u64 *p, u64 v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return atomicOr((unsigned long long *)p, (unsigned long long)v);
#else
    const u64 o = *p; *p = o | v; return o;
#endif
}
HD u64 rx_fetch_and(u64 *p, u64 v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return atomicAnd((unsigned long long *)p, (unsigned long long)v);
#else
    const u64 o = *p; *p = o & v; return o;
#endif
}
HD u64 rx_peek(const u64 *p) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
    return *p;
#endif
}
HD void rx_poke(u64 *p, u64 v) {
#if defined(__HIP_DEVICE_COMPILE__)
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
    *p = v;
#endif
}
HD void rx_refuse(u32 *status, u32 i) {
#if defined(__HIP_DEVICE_COMPILE__)
    atomicMin(status, i);
#else
    if (i < *status) *status = i;
#endif
}

// ---------------------------------------------------------------- number recovery
// AESGCM_RXWIN_LOWEST (RFC 4303 Appendix A2.1, 802.1AEbw 10.6.2): the smallest n >= B = max(T - W, 0) whose low `bits` bits are t.  -> false: no such number below 2^64 - 1
HD bool rx_lowest(u64 T, u32 W, u64 t, u32 bits, u64 &n) {
    const u64 B = T >= W ? T - W : 0u, mod = (u64)1 << bits;
    n = (B & ~(mod - 1u)) | t;
    if (n < B) {
        if (n > ~(u64)0 - mod) return false;
        n += mod;
    }
    return n != AESGCM_RXWIN_NONE;
}
// AESGCM_RXWIN_SRTP (RFC 3711 3.3.1, Appendix A) on s_l = (T - 1) & 0xFFFF, ROC = (T - 1) >> 16: the rollover counter v to take for SEQ.  Nothing goes below ROC 0;
// a result above 2^32 - 1 is the caller's to refuse
HD u64 rx_srtp_roc(u64 T, u32 seq) {
    if (T == 0u) return 0u;
    const u32 s_l = (u32)((T - 1u) & 0xFFFFu);
    const u64 roc = (T - 1u) >> 16;
    if (s_l < 32768u) return seq > s_l + 32768u ? (roc ? roc - 1u : 0u) : roc;
    return s_l - 32768u > seq ? roc + 1u : roc;
}

// Packet i of a recover call.  The tests in this order, nothing of the packet read past the one that refuses it: the window in range; (EXPECT: next is a number;) the
// offsets do not fall; the number field inside the packet; the result below 2^64 - 1 and its rollover counter at most 2^32 - 1
HD void rx_recover_lane(const RxRecoverParams &q, u32 i) {
    const aesgcm_rxwin_fmt &f = q.f;
    const u32 w = q.win[i];
    u64 num = AESGCM_RXWIN_NONE;
    u32 hi = 0xFFFFFFFFu;
    bool ok = w < q.t.n_wins;
    if (ok && f.rule == AESGCM_RXWIN_EXPECT) {
        num = rx_peek(q.t.state + (size_t)w * q.t.stride);
        ok = num != AESGCM_RXWIN_NONE;
        hi = (u32)(num >> 32);
    } else if (ok) {
        const u64 b = q.pkt_off[i], e = q.pkt_off[i + 1];
        const u64 len = e - b;
        ok = e >= b && ((f.flags & AESGCM_RXWIN_FROM_END) ? f.num_off <= len && f.num_len <= f.num_off : (u64)f.num_off + f.num_len <= len);
        if (ok) {
            const unsigned char *const s = q.in + b + ((f.flags & AESGCM_RXWIN_FROM_END) ? len - f.num_off : (u64)f.num_off);
            u64 t = 0;
            for (u32 k = 0; k < f.num_len; k++) t = (t << 8) | s[k];
            if (f.rule == AESGCM_RXWIN_WIRE) {
                if (f.flags & AESGCM_RXWIN_CLEAR_TOP) t &= ~((u64)1 << (8u * f.num_len - 1u));
                num = t;
                ok = num != AESGCM_RXWIN_NONE;
                hi = (u32)(num >> 32);
            } else {
                const u64 T = rx_peek(q.t.state + (size_t)w * q.t.stride);
                if (f.rule == AESGCM_RXWIN_LOWEST) {
                    ok = rx_lowest(T, q.t.window, t, 8u * f.num_len, num);
                    hi = (u32)(num >> (8u * f.num_len));
                } else {
                    const u64 v = rx_srtp_roc(T, (u32)t);
                    ok = v <= 0xFFFFFFFFu;
                    num = (v << 16) | t;
                    hi = (u32)v;
                }
            }
        }
    }
    if (!ok) { num = AESGCM_RXWIN_NONE; hi = 0xFFFFFFFFu; rx_refuse(q.t.status, i); }
    q.num_out[i] = num;
    if (q.hi_out) q.hi_out[i] = hi;
}

// ---------------------------------------------------------------- commit
// packet i's window record and number if it is in S.  -> 0: not authenticated; 4: refused; 1: in S
HD int rx_commit_take(const RxCommitParams &c, u32 i, u64 *&rec, u64 &num) {
    if (c.auth[i] == 0) return RX_WHY_NOAUTH;
    const u32 w = c.win[i];
    if (w >= c.t.n_wins) return RX_WHY_REFUSED;
    num = c.num[i];
    if (num == AESGCM_RXWIN_NONE) return RX_WHY_REFUSED;
    rec = c.t.state + (size_t)w * c.t.stride;
    return RX_WHY_ACCEPT;
}

HD void rx_commit_max_lane(const RxCommitParams &c, u32 i) {
    u64 *rec, num;
    const int k = rx_commit_take(c, i, rec, num);
    if (k == RX_WHY_REFUSED) rx_refuse(c.t.status, i);
    if (k != RX_WHY_ACCEPT) return;
    if (num + 1u > rx_peek(rec + 1)) rx_fetch_max(rec + 1, num + 1u);        // the filter: most lanes of a call find a larger number there already
}

HD void rx_commit_clear_lane(const RxCommitParams &c, u32 i) {
    u64 *rec, num;
    if (rx_commit_take(c, i, rec, num) != RX_WHY_ACCEPT) return;
    const u64 M = rx_peek(rec + 1), T = rx_peek(rec);
    if (num + 1u != M || M == T) return;
    const u32 W = c.t.window;
    u64 *const ring = rec + RX_HDR_WORDS;
    if (M - T >= W) {
        for (u32 k = 0; k < W / 64u; k++) rx_fetch_and(ring + k, 0u);
        return;
    }
    u32 at = (u32)T & (W - 1u), left = (u32)(M - T);                          // left < W positions from `at`, cyclic; a step ends at a word's end at the latest
    while (left) {
        const u32 bit = at & 63u, take = 64u - bit < left ? 64u - bit : left;
        const u64 mask = (take == 64u ? ~(u64)0 : (((u64)1 << take) - 1u)) << bit;
        rx_fetch_and(ring + (at >> 6), ~mask);
        at = (at + take) & (W - 1u);
        left -= take;
    }
}

HD void rx_commit_mark_lane(const RxCommitParams &c, u32 i) {
    u64 *rec, num;
    int why = rx_commit_take(c, i, rec, num);
    if (why == RX_WHY_ACCEPT) {
        const u64 M = rx_peek(rec + 1);
        const u32 W = c.t.window;
        if (M - num > W) why = RX_WHY_OLD;
        else {
            const u32 at = (u32)num & (W - 1u);
            const u64 bit = (u64)1 << (at & 63u);
            if (rx_fetch_or(rec + RX_HDR_WORDS + (at >> 6), bit) & bit) why = RX_WHY_REPLAY;
            if (num + 1u == M) rx_poke(rec, M);
        }
    }
    c.accept[i] = why == RX_WHY_ACCEPT;
    if (c.why) c.why[i] = why;
}

// ---------------------------------------------------------------- the normalised form of aesgcm_rxwin_set / _get (host): bit i of seen[] = number next - 1 - i was seen
HD void rx_norm_to_ring(u64 next, const u64 *seen, u32 W, u64 *ring) {
    for (u32 k = 0; k < W / 64u; k++) ring[k] = 0;
    for (u32 i = 0; i < W && i < next; i++)
        if (seen && ((seen[i >> 6] >> (i & 63u)) & 1u)) { const u32 at = (u32)(next - 1u - i) & (W - 1u); ring[at >> 6] |= (u64)1 << (at & 63u); }
}
HD void rx_ring_to_norm(u64 next, const u64 *ring, u32 W, u64 *seen) {
    for (u32 k = 0; k < W / 64u; k++) seen[k] = 0;
    for (u32 i = 0; i < W && i < next; i++) {
        const u32 at = (u32)(next - 1u - i) & (W - 1u);
        if ((ring[at >> 6] >> (at & 63u)) & 1u) seen[i >> 6] |= (u64)1 << (i & 63u);
    }
}
// bits of a normalised form that stand for numbers below 0
HD bool rx_norm_valid(u64 next, const u64 *seen, u32 W) {
    if (!seen) return true;
    for (u32 i = 0; i < W; i++) if (i >= next && ((seen[i >> 6] >> (i & 63u)) & 1u)) return false;
    return true;
}

// launchers (aesgcm_rxwin_kernels.hip)
hipError_t klaunch_rxwin_recover(hipStream_t st, const RxRecoverParams &p);
hipError_t klaunch_rxwin_commit(hipStream_t st, const RxCommitParams &p);        // the three phases
