// aesgcm_txnum.h -- send counters (aesgcm_txnum_*, include/aesgcm.h "SEND COUNTERS"): packet numbers handed out on the device, in packet order, a lane per packet.
// Shared by the kernels (aesgcm_txnum_kernels.hip), the host side (aesgcm_txnum.hip) and the CPU harness tests/txnum_emul, which runs the lane functions below with
// the lanes in shuffled orders over a rank array from a host stable sort: everything a lane DECIDES is here, HD; the kernels hand out lane numbers and sort.
//
// STATE.  n_ctrs records of TX_REC_WORDS 64-bit words:
//   word 0   next    the number the next packet gets
//   word 1   limit   exclusive upper bound: only numbers below it are ever handed out (next <= limit always)
//   word 2   base    scratch of one assign call: `next` as the call found it
//   word 3   head    scratch of one assign call: the position in the sorted order of the counter's first packet
// An ASSIGN is a stable sort of the packet indices by counter number (out-of-range counters as key n_ctrs, last), then two launches a lane per sorted position i:
//   tx_heads_lane    where the key differs from position i - 1's: head = i, base = next.  One writer per counter, plain stores
//   tx_assign_lane   num = base + (i - head); the refusal tests in order; the outputs and the field bytes of its packet; the LAST lane of a counter's run stores
//                    next = min(base + count, limit).  No lane reads `next` here: that is what `base` is for
// Between the two lies a kernel boundary.  No atomics but the status word's minimum: the cost does not depend on how many packets share a counter.
#pragma once
#include "aesgcm_base.h"
#include "../../include/aesgcm.h"

#define TX_REC_WORDS 4u
#define TX_WG 256u
#define TX_SLICES 256u                      /* workgroups of a sort pass: each owns a slice of consecutive positions */
#define TX_DIGITS 256u                      /* 8-bit digits */
#define TX_ENTRIES (TX_SLICES * TX_DIGITS)  /* counts[digit * TX_SLICES + slice] */

struct TxTable {
    u64 *rec;                              // n_ctrs records
    u32 *status;                           // lowest refused packet (atomic min), ~0 = none
    u32 *counts;                           // TX_ENTRIES: a pass's per-slice digit counts, then their exclusive prefix sums
    u32 *idx[2];                           // max_pkts packet indices each: the passes' outputs in turn (idx[1] only with more than one pass)
    u32 n_ctrs, max_pkts, passes;          // passes = ceil(bitlen(n_ctrs) / 8): the keys are 0 .. n_ctrs
};

struct TxAssignParams {
    TxTable t;
    aesgcm_txnum_fmt f;                    // checked by aesgcm_txnum_fmt_check
    const u32 *ctr;                        // n_pkts counter numbers
    unsigned char *pkts;                   // the packets, written in place; unused with num_len == 0
    const u64 *pkt_off;                    // n_pkts + 1 offsets; unused with num_len == 0
    u64 *num_out;
    u32 *hi_out;                           // or NULL
    u32 *slots;                            // or NULL: 0xFFFFFFFF for a refused packet
    const u32 *sorted;                     // the packet indices, stable by key (the last pass's output)
    u32 n_pkts;
};

HD u32 tx_passes(u32 n_ctrs) { u32 bits = 0; while (bits < 32u && (n_ctrs >> bits)) bits++; return (bits + 7u) / 8u; }
// the sort key of a packet: its counter, or n_ctrs for every counter out of range
HD u32 tx_key(u32 ctr, u32 n_ctrs) { return ctr < n_ctrs ? ctr : n_ctrs; }

HD void tx_refuse(u32 *status, u32 i) {
#if defined(__HIP_DEVICE_COMPILE__)
    atomicMin(status, i);
#else
    if (i < *status) *status = i;
#endif
}

// ---------------------------------------------------------------- what a lane decides
// the k-th packet (k = 0, 1, ..) of a run that found its counter at `base`: its number, if one below `limit` is left
HD bool tx_number(u64 base, u64 limit, u32 k, u64 &num) {
    if ((u64)k >= limit - base) return false;
    num = base + k;
    return true;
}
// `next` behind a run of `count` packets
HD u64 tx_next_after(u64 base, u64 limit, u32 count) { return (u64)count >= limit - base ? limit : base + count; }
// the bits the field carries
HD u32 tx_field_bits(const aesgcm_txnum_fmt &f) { return 8u * f.num_len - ((f.flags & AESGCM_TXNUM_KEEP_TOP) ? 1u : 0u); }
// AESGCM_TXNUM_WHOLE: the number must fit the field
HD bool tx_fits(const aesgcm_txnum_fmt &f, u64 num) {
    const u32 bits = tx_field_bits(f);
    return !(f.flags & AESGCM_TXNUM_WHOLE) || bits >= 64u || (num >> bits) == 0u;
}
// where a run of num_len bytes at offset `off` starts in a packet of `len` bytes.  -> false: not inside the packet
HD bool tx_field_at(const aesgcm_txnum_fmt &f, u64 len, u32 off, u64 &at) {
    if (f.flags & AESGCM_TXNUM_FROM_END) {
        if (off > len || f.num_len > off) return false;
        at = len - off;
        return true;
    }
    if ((u64)off + f.num_len > len) return false;
    at = off;
    return true;
}
// the low bytes of num, big-endian; AESGCM_TXNUM_KEEP_TOP leaves the first byte's top bit as it is
HD void tx_put(const aesgcm_txnum_fmt &f, unsigned char *dst, u64 num) {
    for (u32 k = 0; k < f.num_len; k++) {
        u32 b = (u32)(num >> (8u * (f.num_len - 1u - k))) & 0xFFu;
        if (k == 0 && (f.flags & AESGCM_TXNUM_KEEP_TOP)) b = (dst[0] & 0x80u) | (b & 0x7Fu);
        dst[k] = (unsigned char)b;
    }
}
// Tests 3 to 5 of a packet that has its number, then the field bytes: nothing of the packet is written unless every test passes
HD bool tx_place(const aesgcm_txnum_fmt &f, u64 num, unsigned char *pkts, const u64 *pkt_off, u32 p) {
    if (f.num_len == 0u) return true;
    if (!tx_fits(f, num)) return false;
    const u64 b = pkt_off[p], e = pkt_off[p + 1];
    if (e < b) return false;
    u64 at = 0, dup = 0;
    if (!tx_field_at(f, e - b, f.num_off, at)) return false;
    if (f.dup_off && !tx_field_at(f, e - b, f.dup_off, dup)) return false;
    tx_put(f, pkts + b + at, num);
    if (f.dup_off) tx_put(f, pkts + b + dup, num);
    return true;
}

// ---------------------------------------------------------------- the two launches behind the sort
// the key at position i of the sorted order (an index that is no packet of the call reads nothing: the sort leaves none)
HD u32 tx_key_at(const TxAssignParams &q, u32 i) {
    const u32 p = q.sorted[i];
    return p < q.n_pkts ? tx_key(q.ctr[p], q.t.n_ctrs) : q.t.n_ctrs;
}
HD void tx_heads_lane(const TxAssignParams &q, u32 i) {
    const u32 c = tx_key_at(q, i);
    if (c >= q.t.n_ctrs || (i && tx_key_at(q, i - 1u) == c)) return;
    u64 *const rec = q.t.rec + (size_t)c * TX_REC_WORDS;
    rec[2] = rec[0];
    rec[3] = i;
}

// Position i of the sorted order.  The tests in this order: the counter in range; a number below `limit` left; (WHOLE) the number fits the field; the offsets do not
// fall; the field and its duplicate inside the packet
HD void tx_assign_lane(const TxAssignParams &q, u32 i) {
    const u32 p = q.sorted[i];
    if (p >= q.n_pkts) return;
    const u32 c = tx_key(q.ctr[p], q.t.n_ctrs);
    u64 num = AESGCM_RXWIN_NONE;
    bool ok = c < q.t.n_ctrs;
    if (ok) {
        u64 *const rec = q.t.rec + (size_t)c * TX_REC_WORDS;
        const u64 limit = rec[1], base = rec[2];
        const u32 k = i - (u32)rec[3];
        const bool last = i + 1u == q.n_pkts || tx_key_at(q, i + 1u) != c;
        if (last) rec[0] = tx_next_after(base, limit, k + 1u);
        ok = tx_number(base, limit, k, num) && tx_place(q.f, num, q.pkts, q.pkt_off, p);
    }
    if (!ok) {
        num = AESGCM_RXWIN_NONE;
        if (q.slots) q.slots[p] = 0xFFFFFFFFu;
        tx_refuse(q.t.status, p);
    }
    q.num_out[p] = num;
    if (q.hi_out) q.hi_out[p] = (u32)(num >> 32);
}

// launcher (aesgcm_txnum_kernels.hip): the sort's passes (three launches each), k_tx_heads, k_tx_assign; p.sorted is set by the launcher
hipError_t klaunch_txnum_assign(hipStream_t st, const TxAssignParams &p);
