// aesgcm_rxwin_kernels.hip -- receive windows (gfx950): the kernels of aesgcm_rxwin_recover_dev and aesgcm_rxwin_commit_dev and their launchers; the host side is
// aesgcm_rxwin.hip, the lane code and the state's layout aesgcm_rxwin.h.
//
//   k_rxwin_recover   a lane per packet: the packet's full number from its truncated one and its window's `next` (or `next` itself); writes no state
//   k_rxwin_max       commit, phase 1: the per-window maximum of the authenticated numbers (64-bit atomic max behind a filter)
//   k_rxwin_clear     commit, phase 2: the lanes that hold a window's maximum clear the ring positions the window moves over
//   k_rxwin_mark      commit, phase 3: 64-bit atomic OR of each number's bit; the returned word decides accept or replay; `next` stored
// Four kernels of 256-lane workgroups, no LDS, no scratch, no table of the AES kernels.  The three commit kernels are launched behind one another on one stream: what one
// phase leaves is complete before the next reads it.
// A translation unit of its own: its ISA census (`make asm_rxwin`) is read apart from the others', whose instruction streams stay what they were.
#include "aesgcm_rxwin.h"

__global__ __launch_bounds__(RX_WG) void k_rxwin_recover(const RxRecoverParams q) {
    const u32 i = blockIdx.x * RX_WG + threadIdx.x;
    if (i < q.n_pkts) rx_recover_lane(q, i);
}

// The lanes take the packets from the call's LAST one backwards: traffic carries rising numbers, so the first waves to run meet each window's largest numbers, and the
// lanes behind them find a value in next_new that their number does not exceed and skip the atomic.  Taken forwards, every lane of such a call beats what it reads (2^20
// frames on 64 windows: 16 384 atomics in a row on each of 64 addresses).  Any order gives the same maximum.
__global__ __launch_bounds__(RX_WG) void k_rxwin_max(const RxCommitParams c) {
    const u32 i = blockIdx.x * RX_WG + threadIdx.x;
    if (i < c.n_pkts) rx_commit_max_lane(c, c.n_pkts - 1u - i);
}

__global__ __launch_bounds__(RX_WG) void k_rxwin_clear(const RxCommitParams c) {
    const u32 i = blockIdx.x * RX_WG + threadIdx.x;
    if (i < c.n_pkts) rx_commit_clear_lane(c, i);
}

__global__ __launch_bounds__(RX_WG) void k_rxwin_mark(const RxCommitParams c) {
    const u32 i = blockIdx.x * RX_WG + threadIdx.x;
    if (i < c.n_pkts) rx_commit_mark_lane(c, i);
}

// ------------------------------------------------------------------------------------------------ launchers
hipError_t klaunch_rxwin_recover(hipStream_t st, const RxRecoverParams &p) {
    hipLaunchKernelGGL(k_rxwin_recover, dim3((p.n_pkts + RX_WG - 1u) / RX_WG), dim3(RX_WG), 0, st, p);
    return hipGetLastError();
}

hipError_t klaunch_rxwin_commit(hipStream_t st, const RxCommitParams &p) {
    const dim3 wgs((p.n_pkts + RX_WG - 1u) / RX_WG);
    hipLaunchKernelGGL(k_rxwin_max, wgs, dim3(RX_WG), 0, st, p);
    hipLaunchKernelGGL(k_rxwin_clear, wgs, dim3(RX_WG), 0, st, p);
    hipLaunchKernelGGL(k_rxwin_mark, wgs, dim3(RX_WG), 0, st, p);
    return hipGetLastError();
}
