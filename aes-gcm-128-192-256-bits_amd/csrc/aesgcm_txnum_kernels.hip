// aesgcm_txnum_kernels.hip -- send counters (gfx950): the kernels of aesgcm_txnum_assign_dev and their launcher; the host side is aesgcm_txnum.hip, the lane code
// and the state's layout aesgcm_txnum.h.
//
// "The packets of a counter in ascending array index" is a STABLE ranking by key: an LSD radix sort of the packet indices by counter number, 8 bits a pass, then a
// lane per sorted position.  No workgroup ever waits for another: every dependency between workgroups is a kernel boundary.
//   k_tx_hist      a pass, launch 1: TX_SLICES workgroups own a slice of consecutive positions each and count its digits -> counts[digit * TX_SLICES + slice]
//   k_tx_scan      a pass, launch 2: one workgroup's exclusive prefix sums over counts[] in that (digit-major, slice-minor) order, in place
//   k_tx_scatter   a pass, launch 3: each workgroup walks its slice tile by tile IN ORDER; an entry's place = the slice's cursor of its digit + its rank among the
//                  tile's earlier entries of that digit.  The rank comes from wave ballots (the lanes of a wave that hold the same digit, by eight ballots) and a
//                  count table per wave in LDS with one writer per word: no atomic places anything, so the order inside a digit is the array's
//   k_tx_heads     a lane per sorted position: the first of each counter's run stores head and base (aesgcm_txnum.h tx_heads_lane)
//   k_tx_assign    a lane per sorted position: the number, the refusal tests, the outputs and field bytes of its packet, `next` (tx_assign_lane)
// The only atomic of the unit is the status word's minimum (refused packets).  The cost does not depend on how many packets share a counter.
// A translation unit of its own: its ISA census (`make asm_txnum`) is read apart from the others', whose instruction streams stay what they were.
#include "aesgcm_txnum.h"

struct TxSortParams {
    const u32 *ctr;                        // the call's counter numbers
    const u32 *src;                        // the previous pass's order, or NULL: the identity (pass 0)
    u32 *dst;                              // this pass's order (k_tx_scatter)
    u32 *counts;                           // TX_ENTRIES
    u32 n, n_ctrs, shift;                  // shift = 8 * pass
};

__device__ __forceinline__ void tx_slice(u32 n, u32 &lo, u32 &hi) {
    const u32 per = (n + TX_SLICES - 1u) / TX_SLICES;
    lo = blockIdx.x * per < n ? blockIdx.x * per : n;
    hi = lo + per < n ? lo + per : n;
}
// position i of a pass's input: the packet index there and the digit of its key
__device__ __forceinline__ u32 tx_digit(const TxSortParams &s, u32 i, u32 &pkt) {
    pkt = s.src ? s.src[i] : i;
    return (tx_key(s.ctr[pkt], s.n_ctrs) >> s.shift) & (TX_DIGITS - 1u);
}
// The lanes of this wave that are active and hold the same digit as the caller (eight ballots), as a mask; meaningless for an inactive caller
__device__ __forceinline__ unsigned long long tx_peers(bool active, u32 d) {
    unsigned long long peers = __ballot(active);
#pragma unroll
    for (u32 b = 0; b < 8u; ++b) {
        const bool bit = (d >> b) & 1u;
        const unsigned long long bal = __ballot(active && bit);
        peers &= bit ? bal : ~bal;
    }
    return peers;
}

__global__ __launch_bounds__(TX_WG) void k_tx_hist(const TxSortParams s) {
    __shared__ u32 h[TX_WG / 64u][TX_DIGITS];              // a table per wave: its words have one writer at a time, the lowest lane of a digit's peers
    const u32 lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
#pragma unroll
    for (u32 k = 0; k < TX_WG / 64u; ++k) h[k][threadIdx.x] = 0;
    __syncthreads();
    u32 lo, hi;
    tx_slice(s.n, lo, hi);
    for (u32 t0 = lo; t0 < hi; t0 += TX_WG) {
        const u32 i = t0 + threadIdx.x;
        const bool active = i < hi;
        u32 pkt, d = 0;
        if (active) d = tx_digit(s, i, pkt);
        const unsigned long long peers = tx_peers(active, d);
        if (active && (peers & ((1ull << lane) - 1ull)) == 0ull) h[w][d] += (u32)__popcll(peers);
        __syncthreads();                                   // (the next tile's writer of a word may be another lane of the wave)
    }
    u32 sum = 0;
#pragma unroll
    for (u32 k = 0; k < TX_WG / 64u; ++k) sum += h[k][threadIdx.x];
    s.counts[threadIdx.x * TX_SLICES + blockIdx.x] = sum;
}

// Exclusive prefix sums over the TX_ENTRIES counts, in place; one workgroup of sixteen waves.  Every wave owns 4096 consecutive entries and holds all of them in
// registers, four consecutive entries per lane and step: one trip to memory for the whole array, a wave scan by lane shuffles per step, a carry.
__global__ __launch_bounds__(1024) void k_tx_scan(u32 *__restrict__ counts) {
    __shared__ u32 wave_sum[16];
    constexpr u32 PER_WAVE = TX_ENTRIES / 16u, STEPS = PER_WAVE / 256u;
    static_assert(TX_ENTRIES % (16u * 256u) == 0 && STEPS == 16u, "k_tx_scan: sixteen waves of sixteen steps of 64 lanes x 4 entries");
    const u32 lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    uint4 *seg = reinterpret_cast<uint4 *>(counts + w * PER_WAVE);
    uint4 v[STEPS];
#pragma unroll
    for (u32 k = 0; k < STEPS; ++k) v[k] = seg[k * 64u + lane];
    u32 sum = 0;
#pragma unroll
    for (u32 k = 0; k < STEPS; ++k) sum += v[k].x + v[k].y + v[k].z + v[k].w;
#pragma unroll
    for (u32 off = 32u; off; off >>= 1) sum += __shfl_xor(sum, off);
    if (lane == 0) wave_sum[w] = sum;
    __syncthreads();
    u32 carry = 0;
    for (u32 i = 0; i < w; ++i) carry += wave_sum[i];
#pragma unroll
    for (u32 k = 0; k < STEPS; ++k) {
        const u32 mine = v[k].x + v[k].y + v[k].z + v[k].w;
        u32 incl = mine;
#pragma unroll
        for (u32 off = 1; off < 64u; off <<= 1) { const u32 t = __shfl_up(incl, off); if (lane >= off) incl += t; }
        const u32 e0 = carry + incl - mine;
        seg[k * 64u + lane] = make_uint4(e0, e0 + v[k].x, e0 + v[k].x + v[k].y, e0 + v[k].x + v[k].y + v[k].z);
        carry += __shfl(incl, 63);
    }
}

__global__ __launch_bounds__(TX_WG) void k_tx_scatter(const TxSortParams s) {
    __shared__ u32 cur[TX_DIGITS];                         // where the slice's next entry of each digit goes
    __shared__ u32 wcnt[TX_WG / 64u][TX_DIGITS];           // per wave: the tile's entries of each digit
    const u32 lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    cur[threadIdx.x] = s.counts[threadIdx.x * TX_SLICES + blockIdx.x];
#pragma unroll
    for (u32 k = 0; k < TX_WG / 64u; ++k) wcnt[k][threadIdx.x] = 0;
    u32 lo, hi;
    tx_slice(s.n, lo, hi);
    __syncthreads();
    for (u32 t0 = lo; t0 < hi; t0 += TX_WG) {
        const u32 i = t0 + threadIdx.x;
        const bool active = i < hi;
        u32 pkt = 0, d = 0;
        if (active) d = tx_digit(s, i, pkt);
        const unsigned long long peers = tx_peers(active, d);
        const u32 rank = (u32)__popcll(peers & ((1ull << lane) - 1ull));          // the wave's earlier lanes with this digit
        if (active && rank == 0u) wcnt[w][d] = (u32)__popcll(peers);
        __syncthreads();
        if (active) {
            u32 at = cur[d] + rank;
            for (u32 k = 0; k < w; ++k) at += wcnt[k][d];                         // the tile's earlier waves
            if (at < s.n) s.dst[at] = pkt;                                        // (always: the sums place n entries at 0 .. n - 1)
        }
        __syncthreads();
        {
            u32 add = 0;
#pragma unroll
            for (u32 k = 0; k < TX_WG / 64u; ++k) { add += wcnt[k][threadIdx.x]; wcnt[k][threadIdx.x] = 0; }
            cur[threadIdx.x] += add;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(TX_WG) void k_tx_heads(const TxAssignParams q) {
    const u32 i = blockIdx.x * TX_WG + threadIdx.x;
    if (i < q.n_pkts) tx_heads_lane(q, i);
}

__global__ __launch_bounds__(TX_WG) void k_tx_assign(const TxAssignParams q) {
    const u32 i = blockIdx.x * TX_WG + threadIdx.x;
    if (i < q.n_pkts) tx_assign_lane(q, i);
}

// ------------------------------------------------------------------------------------------------ launcher
hipError_t klaunch_txnum_assign(hipStream_t st, const TxAssignParams &p) {
    TxSortParams s;
    s.ctr = p.ctr; s.src = nullptr; s.counts = p.t.counts; s.n = p.n_pkts; s.n_ctrs = p.t.n_ctrs;
    for (u32 pass = 0; pass < p.t.passes; ++pass) {
        s.dst = p.t.idx[pass & 1u]; s.shift = 8u * pass;
        hipLaunchKernelGGL(k_tx_hist, dim3(TX_SLICES), dim3(TX_WG), 0, st, s);
        hipLaunchKernelGGL(k_tx_scan, dim3(1), dim3(1024), 0, st, s.counts);
        hipLaunchKernelGGL(k_tx_scatter, dim3(TX_SLICES), dim3(TX_WG), 0, st, s);
        s.src = s.dst;
    }
    TxAssignParams q = p;
    q.sorted = s.src;
    const dim3 wgs((p.n_pkts + TX_WG - 1u) / TX_WG);
    hipLaunchKernelGGL(k_tx_heads, wgs, dim3(TX_WG), 0, st, q);
    hipLaunchKernelGGL(k_tx_assign, wgs, dim3(TX_WG), 0, st, q);
    return hipGetLastError();
}
