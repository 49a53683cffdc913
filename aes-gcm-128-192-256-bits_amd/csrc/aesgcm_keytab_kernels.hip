// aesgcm_keytab_kernels.hip -- the kernels of key tables (gfx950) and their launchers; the host side is aesgcm_keytab.hip.
//
//   k_kt_setup<NR>          a thread per slot: aes_kexp, H = E_K(0), H^(2^j) for j = 0 .. 6, then the slot's `set` marker.
//   k_kt_batch<NR,DEC,LG>   k_batch3's body (aesgcm_batch3_body.inc, SLOTS = true) with the key material read from the packet's slot: no aes_kexp, no E_K(0),
//                           no squaring chain in front of the block loop.  E_K(J0) stays per packet (it depends on the IV).
//                           A packet it cannot take -- slot out of range or unset, data / AAD range falling or of 2^28 bytes or more -- reads nothing but its
//                           slot number and offsets: output untouched, tag zero, auth 0, its index into the table's status word (atomicMin).
#include "aesgcm_keytab.h"
#include "aesgcm_lanes.h"
#include "aesgcm_wirecut.h"
#include "aesgcm_dispatch.h"

template <int NR>
__global__ __launch_bounds__(256) void k_kt_setup(const DevTables *__restrict__ tb, const KtSetupParams s) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const u32 tid = threadIdx.x;
    main_fill_lds(smem, nullptr, tb, tid, false, 256u);          // T0 | T2 (the S-box of the key schedule is byte 1 of T0)
    __syncthreads();
    const u32 i = blockIdx.x * 256u + tid;
    if (i >= s.n) return;
    const u32 slot = s.slots ? s.slots[i] : s.first + i;
    if (slot >= s.n_slots) { atomicMin(s.status, i); return; }
    const u32 lb = (tid & 31u) << 2;
    u32 rk[4 * (NR + 1)];
    batch_key_expand<NR>(s.keys + (size_t)i * (4 * (NR - 6)), rk, smem, lb);
    u32 s0 = rk[0], s1 = rk[1], s2 = rk[2], s3 = rk[3];
    aes_rounds_lds<NR>(s0, s1, s2, s3, rk, smem, lb);            // H = E_K(0^128)
    G128 h = mo_to_be(make_uint4(s0, s1, s2, s3));
    KtSlot *d = s.tab + slot;
#pragma unroll
    for (int q = 0; q < NR + 1; q++) *reinterpret_cast<uint4 *>(d->rk + 4 * q) = make_uint4(rk[4 * q], rk[4 * q + 1], rk[4 * q + 2], rk[4 * q + 3]);
#pragma unroll
    for (int j = 0; j < KT_HPOW; j++) {
        d->hpow[j] = make_uint4(h.w[0], h.w[1], h.w[2], h.w[3]);
        h = gf_sqr(h);
    }
    d->nr = NR;
    __threadfence();
    d->set = KT_SET;
}

template <int NR, int DEC, int LG>                       // DEC: 0 encrypt, 1 decrypt
__global__ __launch_bounds__(BATCH3_LANES(NR), (BATCH3_LANES(NR) + 255) / 256) void k_kt_batch(const DevTables *__restrict__ tb, const KtParams kp) {
    constexpr bool SLOTS = true;                         // key material from the slots of kt
    const KtParams *const kt = &kp;
    const BatchParams &p = kp.b;
    constexpr bool WIRE = false;                         // packets as five arrays, not frames in wire format (aesgcm_wire_kernels.hip)
    constexpr const aesgcm_wire_fmt *wf = nullptr;
    constexpr u32 WIREX = 0;                            // ... and no number per packet beside them (aesgcm_wirex_kernels.hip)
    constexpr const KtWireXParams *wx = nullptr;
#include "aesgcm_batch3_body.inc"
}

// ------------------------------------------------------------------------------------------------ launchers
#define KT_SETUP_LDS (AESGCM_LDS_AES_OFF + AESGCM_LDS_AES)
hipError_t klaunch_kt_attributes() {
    const hipError_t e = batch3_each([](auto NR, auto D, auto LG) { return hipFuncSetAttribute(reinterpret_cast<const void *>(&k_kt_batch<NR(), D(), LG()>), hipFuncAttributeMaxDynamicSharedMemorySize, BATCH3_LDS_BYTES_LG(LG())); });
    return e != hipSuccess ? e : nr_each([](auto NR) { return hipFuncSetAttribute(reinterpret_cast<const void *>(&k_kt_setup<NR()>), hipFuncAttributeMaxDynamicSharedMemorySize, KT_SETUP_LDS); });
}

hipError_t klaunch_kt_setup(int nr, hipStream_t st, const DevTables *tb, const KtSetupParams &s) {
    const unsigned wgs = (s.n + 255u) / 256u;
    nr_dispatch(nr, [&](auto NR) { hipLaunchKernelGGL(k_kt_setup<NR()>, dim3(wgs), dim3(256), KT_SETUP_LDS, st, tb, s); });
    return hipGetLastError();
}

hipError_t klaunch_kt_batch(int nr, int dec, int lg, unsigned wgs, hipStream_t st, const DevTables *tb, const KtParams &p) {
    batch3_dispatch(nr, dec, lg, [&](auto NR, auto D, auto LG) { hipLaunchKernelGGL((k_kt_batch<NR(), D(), LG()>), dim3(wgs), dim3(BATCH3_LANES(NR())), BATCH3_LDS_BYTES_LG(LG()), st, tb, p); });
    return hipGetLastError();
}
