// CPU harness for the send counters' lane code (csrc/aesgcm_txnum.h is __host__ __device__): it runs the SAME functions k_tx_heads and k_tx_assign run, over a rank
// array from a host stable sort (std::stable_sort by tx_key: what the radix passes of aesgcm_txnum_kernels.hip produce), with the lanes of both launches in an order
// shuffled by a seed -- a result that depended on which lane comes first would show.  Beside it runs a SEQUENTIAL REFERENCE written here from the header's text alone
// (include/aesgcm.h "SEND COUNTERS"): the packets one after another in array order, a counter incremented per packet.  Every call prints what the lane code made of
// it and, per packet and per counter, whether the reference made the same; "MISMATCH" lines and a non-zero exit say it did not.  tests/test_txnum_cpu.py writes the
// scripts and also holds the printed values to its own expectations.  Test infrastructure only.
//   T n_ctrs                         a new table, every counter next = 0, limit = 0
//   S ctr next limit                 sets a counter
//   D hex | D -                      the packet bytes of the assign calls that follow (each call works on a fresh copy with guard bytes behind)
//   A off len dup flags n seed       an assign call of n packets; then a line "O o_0 .. o_n" (the offsets) and a line "C c_0 .. c_(n-1)" (the counters)
//                                      -> n lines "a num hi slot", a line "d hex" (the bytes afterwards), a line "x status"
//   G                                -> per counter "g ctr next limit"
//   B                                -> lines "b n passes": tx_passes(n) for n = 1, 255, 256, 65535, 65536, 65537, 2^31 - 1
#include "../../aes-gcm-128-192-256-bits_amd/csrc/aesgcm_txnum.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <string>
#include <vector>

static u64 g_rng;
static u64 splitmix() { u64 z = (g_rng += 0x9E3779B97F4A7C15ull); z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
static std::vector<u32> order(u32 n) {
    std::vector<u32> o(n);
    for (u32 i = 0; i < n; i++) o[i] = i;
    for (u32 i = n; i > 1; i--) std::swap(o[i - 1], o[splitmix() % i]);
    return o;
}

// ---------------------------------------------------------------- the sequential reference: nothing of aesgcm_txnum.h but the format struct and the constants
struct RefOut { u64 num; u32 hi, slot; };
static bool ref_inside(const aesgcm_txnum_fmt &f, u64 len, u64 off, u64 &at) {
    if (f.flags & AESGCM_TXNUM_FROM_END) { if (off > len || f.num_len > off) return false; at = len - off; return true; }
    if (off + f.num_len > len) return false;
    at = off;
    return true;
}
static void ref_write(const aesgcm_txnum_fmt &f, unsigned char *dst, u64 num) {
    const unsigned char top = dst[0] & 0x80;
    for (u32 k = 0; k < f.num_len; k++) dst[f.num_len - 1 - k] = (unsigned char)(num >> (8 * k));
    if (f.flags & AESGCM_TXNUM_KEEP_TOP) dst[0] = (unsigned char)((dst[0] & 0x7F) | top);
}
static u32 ref_call(const aesgcm_txnum_fmt &f, std::vector<u64> &next, const std::vector<u64> &limit, const std::vector<u32> &ctr, const std::vector<u64> &off,
                    std::vector<unsigned char> &data, std::vector<RefOut> &out) {
    u32 status = ~0u;
    for (u32 p = 0; p < ctr.size(); p++) {
        bool ok = ctr[p] < next.size();
        u64 num = 0;
        if (ok) {
            u64 &nx = next[ctr[p]];
            ok = nx < limit[ctr[p]];                                          // (2) a number below the limit is left
            if (ok) num = nx++;                                               // counted from here on: tests 3 to 5 burn the number
        }
        if (ok && f.num_len) {
            const u32 bits = 8 * f.num_len - ((f.flags & AESGCM_TXNUM_KEEP_TOP) ? 1 : 0);
            if ((f.flags & AESGCM_TXNUM_WHOLE) && bits < 64 && num >= ((u64)1 << bits)) ok = false;      // (3)
            u64 at = 0, dup = 0;
            if (ok && off[p + 1] < off[p]) ok = false;                                                    // (4)
            if (ok && !ref_inside(f, off[p + 1] - off[p], f.num_off, at)) ok = false;                     // (5)
            if (ok && f.dup_off && !ref_inside(f, off[p + 1] - off[p], f.dup_off, dup)) ok = false;
            if (ok) { ref_write(f, data.data() + off[p] + at, num); if (f.dup_off) ref_write(f, data.data() + off[p] + dup, num); }
        }
        out[p].num = ok ? num : AESGCM_RXWIN_NONE;
        out[p].hi = ok ? (u32)(num >> 32) : 0xFFFFFFFFu;
        out[p].slot = ok ? 7u : 0xFFFFFFFFu;
        if (!ok && p < status) status = p;
    }
    return status;
}

int main() {
    TxTable t = {};
    std::vector<u64> rec;
    std::vector<unsigned char> data(16, 0);
    u32 status = ~0u;
    int mismatches = 0;
    static char line[1 << 20], a[1 << 19];
    auto need = [&](bool ok) { if (!ok) { printf("bad script line: %s\n", line); exit(2); } };
    while (fgets(line, sizeof line, stdin)) {
        unsigned long long x0, x1, x2, x3, x4, x5;
        if (line[0] == 'T') {
            need(sscanf(line + 1, "%llu", &x0) == 1 && x0);
            t.n_ctrs = (u32)x0; t.max_pkts = 1u << 20; t.passes = tx_passes(t.n_ctrs);
            rec.assign((size_t)t.n_ctrs * TX_REC_WORDS, 0);
            t.rec = rec.data(); t.status = &status;
        } else if (line[0] == 'S') {
            need(sscanf(line + 1, "%llu %llu %llu", &x0, &x1, &x2) == 3 && x0 < t.n_ctrs && x1 <= x2);
            rec[x0 * TX_REC_WORDS] = x1; rec[x0 * TX_REC_WORDS + 1] = x2;
        } else if (line[0] == 'D') {
            need(sscanf(line + 1, "%524287s", a) == 1);
            data.assign(16, 0xA5);
            if (a[0] != '-') { const size_t n = strlen(a) / 2; data.assign(n + 16, 0xA5); for (size_t k = 0; k < n; k++) { unsigned b; sscanf(a + 2 * k, "%2x", &b); data[k] = (unsigned char)b; } }
        } else if (line[0] == 'A') {
            need(sscanf(line + 1, "%llu %llu %llu %llu %llu %llu", &x0, &x1, &x2, &x3, &x4, &x5) == 6);
            const u32 n = (u32)x4;
            g_rng = x5;
            std::vector<u64> off(n + 1), num(n, 7);
            std::vector<u32> ctr(n), hi(n, 7), slot(n, 7), sorted(n);
            for (int row = 0; row < 2; row++) {
                need(fgets(line, sizeof line, stdin) && line[0] == "OC"[row]);
                char *p = line + 1;
                for (u32 k = 0; k < (row ? n : n + 1); k++) { const u64 v = strtoull(p, &p, 10); if (row) ctr[k] = (u32)v; else off[k] = v; }
            }
            TxAssignParams q = {};
            q.f.num_off = (u32)x0; q.f.num_len = (u32)x1; q.f.dup_off = (u32)x2; q.f.flags = (u32)x3;
            // the reference first, on copies
            std::vector<u64> rnext(t.n_ctrs), rlimit(t.n_ctrs);
            for (u32 c = 0; c < t.n_ctrs; c++) { rnext[c] = rec[c * TX_REC_WORDS]; rlimit[c] = rec[c * TX_REC_WORDS + 1]; }
            std::vector<unsigned char> rdata = data, work = data;
            std::vector<RefOut> want(n);
            const u32 rstatus = ref_call(q.f, rnext, rlimit, ctr, off, rdata, want);
            // the lane code: the rank array from a host stable sort, both launches with their lanes shuffled
            for (u32 i = 0; i < n; i++) sorted[i] = i;
            std::stable_sort(sorted.begin(), sorted.end(), [&](u32 l, u32 r) { return tx_key(ctr[l], t.n_ctrs) < tx_key(ctr[r], t.n_ctrs); });
            q.t = t; q.ctr = ctr.data(); q.pkts = work.data(); q.pkt_off = off.data(); q.num_out = num.data(); q.hi_out = hi.data(); q.slots = slot.data();
            q.sorted = sorted.data(); q.n_pkts = n;
            for (u32 i : order(n)) tx_heads_lane(q, i);
            for (u32 i : order(n)) tx_assign_lane(q, i);
            for (u32 i = 0; i < n; i++) {
                printf("a %llu %u %u\n", (unsigned long long)num[i], hi[i], slot[i]);
                if (num[i] != want[i].num || hi[i] != want[i].hi || slot[i] != want[i].slot) { printf("MISMATCH packet %u: reference %llu %u %u\n", i, (unsigned long long)want[i].num, want[i].hi, want[i].slot); mismatches++; }
            }
            std::string s;
            char b[4];
            for (unsigned char c : work) { snprintf(b, sizeof b, "%02x", c); s += b; }
            printf("d %s\n", s.c_str());
            if (work != rdata) { printf("MISMATCH bytes\n"); mismatches++; }
            for (u32 c = 0; c < t.n_ctrs; c++)
                if (rec[c * TX_REC_WORDS] != rnext[c] || rec[c * TX_REC_WORDS + 1] != rlimit[c]) { printf("MISMATCH counter %u: reference next %llu\n", c, (unsigned long long)rnext[c]); mismatches++; }
            printf("x %u\n", status);
            if (status != rstatus) { printf("MISMATCH status: reference %u\n", rstatus); mismatches++; }
            status = ~0u;
        } else if (line[0] == 'G') {
            for (u32 c = 0; c < t.n_ctrs; c++) printf("g %u %llu %llu\n", c, (unsigned long long)rec[c * TX_REC_WORDS], (unsigned long long)rec[c * TX_REC_WORDS + 1]);
        } else if (line[0] == 'B') {
            for (u32 n : {1u, 255u, 256u, 65535u, 65536u, 65537u, 0x7FFFFFFFu}) printf("b %u %u\n", n, tx_passes(n));
        } else need(line[0] == '#' || line[0] == '\n');
    }
    return mismatches ? 1 : 0;
}
