// aesgcm_lanes.h -- cross-lane helpers and the lane-group pieces of the body k_batch3 shares with k_kt_batch (aesgcm_batch3_body.inc).
// Device code only: included by the two kernel translation units, not by aesgcm_dev.h (the host harness of tests/host_emul never sees it).
#pragma once
#include "aesgcm_dev.h"

// value of lane (lane ^ MASK).  For MASK < 32 this is ds_swizzle in bit mode (and 0x1F, or 0, xor MASK: no address register);
// __shfl_xor lowers to ds_bpermute with a per-lane index, and the compiler hoists those index registers out of the packet
// loops -- in k_pktg at 128 registers they were 7 of the ~20 dwords it then spilled to scratch (round-3 ISA).
template <int MASK>
__device__ __forceinline__ u32 lane_xor(u32 x) {
    if constexpr (MASK < 32) return (u32)__builtin_amdgcn_ds_swizzle((int)x, (MASK << 10) | 0x1F);
    else return (u32)__shfl_xor((int)x, MASK);
}
// the lane's index in its wave from nothing but the execution mask (no input register, opaque to common-subexpression elimination)
__device__ __forceinline__ u32 lane_id_fresh() {
    u32 x;
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(x));
    return x;
}
__device__ __forceinline__ u32 lane_xor_pow2(u32 x, int j) {           // lane ^ (1 << j); j is a constant after unrolling
    switch (j) {
    case 0: return lane_xor<1>(x);
    case 1: return lane_xor<2>(x);
    case 2: return lane_xor<4>(x);
    case 3: return lane_xor<8>(x);
    case 4: return lane_xor<16>(x);
    default: return lane_xor<32>(x);
    }
}

// the two-table Shoup form of a constant c at LDS offset `tab` (Th at tab, Tl = Th * x^4 at tab + 256), built by the 2^LG lanes that share it
template <int LG>
__device__ __forceinline__ void shoup2_build(unsigned char *smem, u32 tab, G128 c, u32 l) {
#pragma unroll
    for (u32 v = l; v < 16; v += (1u << LG)) {               // 16 entries per table, built by the group's own lanes
        const G128 e = shoup_entry(c, v), el = gf_mulx4(e);
        *reinterpret_cast<uint4 *>(smem + tab + 16 * v) = make_uint4(e.w[0], e.w[1], e.w[2], e.w[3]);
        *reinterpret_cast<uint4 *>(smem + tab + 256 + 16 * v) = make_uint4(el.w[0], el.w[1], el.w[2], el.w[3]);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ---- k_batch3 / k_kt_batch lane groups (aesgcm_kernels.hip says why the lanes are laid out so)
#ifndef BATCH3_PERM
#define BATCH3_PERM 1
#endif
#ifndef BATCH3_DR
#define BATCH3_DR 1                        /* shoup2_mul_dr: the table multiply with its reduction delayed */
#endif
template <int LG>
__device__ __forceinline__ void batch3_pos(u32 lane, u32 &grp, u32 &l) {
    if (BATCH3_PERM && LG == 4) { grp = ((lane >> 4) & 2u) | (((lane >> 2) ^ (lane >> 3) ^ (lane >> 4)) & 1u); l = ((lane >> 1) & 12u) | (lane & 3u); }
    else if (BATCH3_PERM && LG == 3) { grp = ((lane >> 3) & 6u) | (((lane >> 2) ^ (lane >> 3)) & 1u); l = ((lane >> 1) & 4u) | (lane & 3u); }
    else { grp = lane >> LG; l = lane & ((1u << LG) - 1u); }
}
template <int LG>
__device__ __forceinline__ constexpr u32 batch3_first_lane(u32 g) {          // lane of position 0 of packet group g
    return (BATCH3_PERM && LG == 4) ? (g >> 1) * 32u + (g & 1u) * 4u : (BATCH3_PERM && LG == 3) ? (g >> 2) * 32u + ((g >> 1) & 1u) * 16u + (g & 1u) * 4u : g << LG;
}
template <int LG>
__device__ __forceinline__ u32 batch3_groups_max(u32 v) {                     // the largest value of a group-uniform quantity over the wave's packets
    u32 m = 0;
#pragma unroll
    for (u32 g = 0; g < (64u >> LG); g++) { const u32 x = (u32)__builtin_amdgcn_readlane((int)v, (int)batch3_first_lane<LG>(g)); m = x > m ? x : m; }
    return m;
}
template <int LG>
__device__ __forceinline__ u32 batch3_partner(u32 x, int j) {                 // the value of the lane whose position differs in bit j
    if (LG == 6) return lane_xor_pow2(x, j);                                   // a wave per packet: positions are the lanes
#if BATCH3_PERM
    switch (j) {
    case 0: return lane_xor<1>(x);
    case 1: return lane_xor<2>(x);
    case 2: return lane_xor<12>(x);
    default: return lane_xor<20>(x);
    }
#else
    return lane_xor_pow2(x, j);
#endif
}
#if BATCH3_DR
#define BATCH3_MUL shoup2_mul_dr
#else
#define BATCH3_MUL shoup2_mul
#endif
// 8 lanes per packet: a service group still holds TWO packets, and their table reads collide (23.8 % of the LDS-array cycles, profiles/r04/batch_ab.txt).
// BATCH3_PAIR=1 splits every multiply over the two lanes lane and lane ^ 20 of the two packets (the reference's split multiplier, src/gcm_ghash.vhd:317-333,
// over lanes instead of over two multiplier halves): in a first pass ALL sixteen lanes of the service group read the table of the packet with lane bit 4
// clear -- its own lanes for words 0, 1 of their accumulators, the partner lanes for words 2, 3 of the same accumulators -- in a second pass the other
// packet's.  Same 32 reads per lane, never two tables in one service group; the partials (6 words each way) cross by ds_swizzle.
#ifndef BATCH3_PAIR
#define BATCH3_PAIR 1
#endif
__device__ __forceinline__ G128 batch3_mul_pair(G128 y, const unsigned char *smem, u32 tab_mine, u32 tab_partner, bool first) {
    const u32 p2 = lane_xor<20>(y.w[2]), p3 = lane_xor<20>(y.w[3]);            // the partner's accumulator, words 2, 3
    u32 V1[6], V2[6];
    shoup2_half_dr(first ? y.w[0] : p2, first ? y.w[1] : p3, smem, first ? tab_mine : tab_partner, V1);     // pass 1: the table of the `first` packet
    shoup2_half_dr(first ? p2 : y.w[0], first ? p3 : y.w[1], smem, first ? tab_partner : tab_mine, V2);     // pass 2: the other packet's
    u32 Vo[6], Vh[6];
#pragma unroll
    for (int j = 0; j < 6; j++) {
        Vo[j] = first ? V1[j] : V2[j];                                         // the pass in which this lane worked on its own accumulator
        Vh[j] = lane_xor<20>(first ? V2[j] : V1[j]);                           // what the partner computed for this lane's accumulator
    }
    return shoup2_pair_join(Vo, Vh);
}
