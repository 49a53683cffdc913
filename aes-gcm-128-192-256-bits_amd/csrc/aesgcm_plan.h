// aesgcm_plan.h -- the PURE part of the packet paths' launch planning: arithmetic on counts and lengths, with the measurements each rule stands on.  Which shape a
// call takes (lanes per packet), k_pktl's ILP form, packets per dispenser fetch, the loops without padding tests (`plain`), the grid.  No HIP call, no context and
// no HIP header.  The planners that act on these -- packets_plan, the routed loop of packets_rows, batch_plan: aesgcm_host.hip -- add what needs a context or
// the runtime: the dispensers, the streams, the forced shapes of the debug build.
// NOT self-contained: the kernels' geometry (AESGCM_PKT_WG, AESGCM_PKTL_WG, AESGCM_PKTL_WG_ILP, PKTG_WG, PKTG_MAX_DEAL) comes from the includer, which defines it
// first -- aesgcm_internal.h, from the kernel headers' workgroup sizes; nothing else includes this file.
#pragma once
#include <stddef.h>
#include <stdint.h>

// Packets under ONE key: how many lanes work on one packet, as log2 (0 = one LANE per packet, k_pktl; 2, 3, 4 = a lane GROUP of 4, 8, 16, k_pktg; 6 = a whole
// wave, k_pktg<.., 6>).  Measured (profiles/archive/r03/packets_sweep_aes256.txt, GiB/s wave / g16 / g8 / g4 / lane): the best shape is the one that just fills the
// resident lanes (256 CUs x 16 waves x 64) -- 65536 x 1 KiB 203 / 232 / 340 / 384 / 194, 16384 x 4 KiB 235 / 367 / 290 / 177 / 53, 4096 x 16 KiB
// 362 / 172 / 95 / 49 / 13 (the one regime where a whole wave per packet is right: at most 4096 packets of at least 4 KiB) -- but never more lanes than an
// eighth of the packet's blocks once the machine is full (closing cost per byte: 16384 x 1 KiB 62 / 128 / 176 / 138 / 50, 16384 x 256 B 16 / 35 / 58 / 72 / 41),
// a quarter when it is not (4096 x 1 KiB 34 / 69 / 57 / 38 / 13).  Lanes win from 131072 packets (2^20 x 1 KiB 303 / 592 / 657 / 742 / 767; 262144 x 4 KiB
// 496 / 656 / 704 / 722 / 724), short packets from 32768 (65536 x 256 B 51 / 61 / 95 / 129 / 148).
inline int packets_pick_lg(uint32_t n_cu, size_t n_pkts, size_t pkt_len) {
    const size_t lanes_total = (size_t)n_cu * (AESGCM_PKT_WG / 64) * 64, lanes_l = (size_t)n_cu * AESGCM_PKTL_WG;
    const size_t blocks = (pkt_len + 15) / 16;
    // One lane per packet once the packets fill k_pktl's resident lanes (256 x 768); frames of up to 1 KiB from three quarters of that, short ones much earlier.
    // Round 4 (profiles/r04/packets_sweep_aes256.txt, after k_pktl's rebuild): 131072 x 4 KiB 553 by lanes against 722 by groups of 4 (196608: 795 / 713),
    // 131072 x 16 KiB 573 / 789, 131072 x 1 KiB 488 / 509 (196608: 677 / 577), 49152 x 256 B 142 / 124, 16384 x 64 B 28 / 23.
    // (Offset arrays -- the host does not know the lengths -- are routed on the device since round 6: route_pick_lg, aesgcm_pkt.h, with the measurements behind it.)
    // k_pktl's ILP form (512-lane workgroups) moves the 1 KiB mark down: 131072 x 1 KiB 592 by lanes against 500 by groups of 4, 98304: 454 / 456.
    const size_t lanes_ilp = (size_t)n_cu * AESGCM_PKTL_WG_ILP;
    if (n_pkts >= lanes_l || (pkt_len <= 1024 && 8 * n_pkts >= 7 * lanes_ilp) || (pkt_len <= 256 && n_pkts >= 32768) || (pkt_len <= 64 && n_pkts >= 16384)) return 0;
    // Lane groups: the group that just fills the resident lanes.  Packets of 4 KiB and more round the fill UP to a power of two (half again as many lanes as
    // are resident is cheaper than rows twice as long: 49152 x 4 KiB 474 with 4 lanes, 576 with 8; x 16 KiB 542 / 722), shorter ones down (49152 x 1 KiB 325 / 291).
    size_t fill = lanes_total / n_pkts;
    if (pkt_len >= 4096 && (fill & (fill - 1))) { size_t f = 1; while (f < fill) f <<= 1; fill = f; }
    const size_t cap = n_pkts >= 16384 ? blocks / 8 : blocks / 4;
    const size_t g = fill < cap ? fill : cap;
    return g >= 64 ? 6 : g >= 16 ? 4 : g >= 8 ? 3 : 2;
}

// the ILP form (512-lane workgroups, eight independent keystream chains per line) while the packets fit one round of it; its workgroups are spread over
// all CUs, a wave of 64 packets each first
// Measured, AES-256, GiB/s 768-lane form / ILP form (profiles/r04/packets_sweep_ilp_aes256.txt): 1 KiB packets 16384 66 / 78, 65536 255 / 306, 131072 481 / 592;
// 256 B 32768 99 / 95, 98304 245 / 266, 131072 295 / 330; 64 B (no whole line to work on) 16384 27 / 19.
// Packets shorter than two lines gain from it only once they fill the chip (fewer, fatter waves): 196608 x 256 B 380 / 414, 262144 442 / 460 (2^20: 682 / 642);
// 64 B 196608 127 / 146, 393216 183 / 201, 2^20 254 / 266.
inline bool pktl_pick_ilp(uint32_t n_cu, size_t n_pkts, size_t pkt_len) {
    return n_pkts <= (size_t)n_cu * AESGCM_PKTL_WG_ILP ? (pkt_len >= 512 || (pkt_len >= 256 && n_pkts >= 49152))
                                                       : (n_pkts >= (size_t)n_cu * AESGCM_PKTL_WG && (pkt_len <= 64 || (pkt_len <= 256 && n_pkts <= 300000)));
}

// deal: about 4 dispenser fetches per resident wave, a multiple of P, at most 64 packets (one E_K(J0) pass per fetch)
inline uint32_t pktg_pick_deal(uint32_t n_cu, int lg, size_t n_pkts) {
    const uint32_t P = 64u >> lg, waves_per_wg = (uint32_t)PKTG_WG(lg) / 64;                                    // P: packets per wave-iteration
    uint32_t deal = (uint32_t)(n_pkts / ((size_t)n_cu * waves_per_wg * 4));
    deal = deal / P * P;
    return deal < P ? P : deal > PKTG_MAX_DEAL ? PKTG_MAX_DEAL : deal;
}
// PktParams::plain -- k_pktg<.., 6 | 2>: fixed-size aligned records of whole group-iterations, no AAD
inline bool pktg_is_plain(int lg, bool aad, bool aligned, size_t pkt_len) { return (lg == 6 || lg == 2) && !aad && aligned && pkt_len && pkt_len % ((size_t)16 << lg) == 0; }

// The grid of a k_pktl (lg 0; ilp: its 512-lane form) or k_pktg launch over n packets on n_cu CUs: nb dispenser blocks -- a wave's 64 packets for k_pktl, `deal`
// packets for k_pktg -- on wgs workgroups of waves_per_wg waves, at most one workgroup per CU (registers and LDS).  The ILP form spreads its workgroups over all
// CUs, a wave of 64 packets each first.  Every wave ends on one failing fetch: the launch moves its dispenser on by nb + wgs * waves_per_wg.
struct PktGrid { uint32_t nb, wgs, waves_per_wg; };
inline PktGrid pkt_grid(uint32_t n_cu, size_t n, int lg, bool ilp, uint32_t deal) {
    PktGrid g;
    g.waves_per_wg = (uint32_t)(lg ? PKTG_WG(lg) : ilp ? AESGCM_PKTL_WG_ILP : AESGCM_PKTL_WG) / 64;
    g.nb = lg ? (uint32_t)((n + deal - 1) / deal) : (uint32_t)((n + 63) / 64);
    g.wgs = !lg && ilp ? g.nb : (g.nb + g.waves_per_wg - 1) / g.waves_per_wg;
    if (g.wgs > n_cu) g.wgs = n_cu;
    return g;
}

// Packets with their OWN key (k_batch3): lanes per packet as log2 (3, 4, 6 = 8 / 16 lanes, a whole wave; the two-pass kernel k_batch of rounds 2 - 3 that
// the numbers below call by name is gone since round 4: k_batch3<.., 6> took its place, 4096 x 1 MiB 443 -> 637 GiB/s).  16 lanes once
// there are packets enough to fill the machine that way (one 1024-lane workgroup per CU = 64 packets per CU) or the packets are short, else one wave per packet.
// Measured, AES-128, GiB/s k_batch / k_batch3 (profiles/archive/r03/batch_sweep_aes128.txt): 4096 x 1 KiB 30 / 56, 4096 x 256 B 7.5 / 17, 1024 x 1 KiB 14 / 16.5; 1024 x 4 KiB
// 45 / 33, 4096 x 4 KiB 108 / 120, 4096 x 16 KiB 286 / 168; from 16384 packets k_batch3 wins at every size (4 KiB 179 / 350).  8 lanes (eight packets per wave
// share what a wave-iteration pays once) when there are packets enough to fill the chip that way and they are not long: 2^20 packets of 64 B 42 -> 74 GiB/s,
// 256 B 163 -> 265, 1 KiB 424 -> 560, 1500 B 484 -> 598, 4 KiB 658 -> 706, 16 KiB 770 -> 736; 16384 packets: 1 KiB 125 -> 155, 4 KiB 352 -> 273
// (profiles/archive/r03c/batch_sweep_lanes8_aes128.txt).  Batches with per-packet lengths (offset arrays on the device: the host does not know the lengths) go by count
// alone and assume frames of MACsec size, where 8 lanes gain most; a batch of frames beyond 8 KiB loses ~5 % by it.
inline int batch_pick_lg(int n_cu, size_t n_pkts, size_t pkt_len, bool var) {
    int lg = (n_pkts >= (size_t)64 * n_cu || (!var && pkt_len <= 2048)) ? 4 : 6;
    if (lg == 4 && (var ? n_pkts >= (size_t)64 * n_cu
                        : ((n_pkts >= (size_t)256 * n_cu && pkt_len <= 8192) || (n_pkts >= (size_t)64 * n_cu && pkt_len <= 2048)))) lg = 3;
    return lg;
}
// deal: a sixteenth of a wave's share, a multiple of P, at most 8 P
inline uint32_t batch_pick_deal(uint32_t wgs, uint32_t waves_per_wg, int lg, size_t n_pkts) {
    const uint32_t P = 64u >> lg;
    const uint32_t deal = (uint32_t)(n_pkts / ((size_t)wgs * waves_per_wg * 16));
    return deal < P ? P : deal > 8 * P ? 8 * P : (deal + P - 1) / P * P;
}
// BatchParams::plain -- fixed-size aligned records of a whole number of wave-iterations, no AAD
inline bool batch_is_plain(int lg, bool var_or_aad, bool aligned, uint32_t pkt_len) { return !var_or_aad && aligned && pkt_len && pkt_len % (16u << lg) == 0; }
