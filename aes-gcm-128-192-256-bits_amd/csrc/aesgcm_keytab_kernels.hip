// aesgcm_keytab_kernels.hip -- the kernels of key tables (gfx950) and their launchers; the host side is aesgcm_keytab.hip.
//
//   k_kt_setup<NR>          a thread per slot: aes_kexp, H = E_K(0), H^(2^j) for j = 0 .. 6, then the slot's `set` marker.
//   k_kt_batch<NR,DEC,LG>   k_batch3's body (aesgcm_batch3_body.inc, SLOTS = true) with the key material read from the packet's slot: no aes_kexp, no E_K(0),
//                           no squaring chain in front of the block loop.  E_K(J0) stays per packet (it depends on the IV).
//                           A packet it cannot take -- slot out of range or unset, data / AAD range falling or of 2^28 bytes or more -- reads nothing but its
//                           slot number and offsets: output untouched, tag zero, auth 0, its index into the table's status word (atomicMin).
#include "aesgcm_keytab.h"
#include "aesgcm_lanes.h"

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
#define ATTRCHK(call) do { const hipError_t _e = (call); if (_e != hipSuccess) return _e; } while (0)
hipError_t klaunch_kt_attributes() {
#define SETATTRKT(NR, D) ATTRCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_kt_batch<NR, D, 6>), hipFuncAttributeMaxDynamicSharedMemorySize, BATCH3_LDS_BYTES_LG(6))); \
                         ATTRCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_kt_batch<NR, D, 4>), hipFuncAttributeMaxDynamicSharedMemorySize, BATCH3_LDS_BYTES_LG(4))); \
                         ATTRCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_kt_batch<NR, D, 3>), hipFuncAttributeMaxDynamicSharedMemorySize, BATCH3_LDS_BYTES_LG(3)))
    SETATTRKT(10, 0); SETATTRKT(12, 0); SETATTRKT(14, 0); SETATTRKT(10, 1); SETATTRKT(12, 1); SETATTRKT(14, 1);
#undef SETATTRKT
    ATTRCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_kt_setup<10>), hipFuncAttributeMaxDynamicSharedMemorySize, KT_SETUP_LDS));
    ATTRCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_kt_setup<12>), hipFuncAttributeMaxDynamicSharedMemorySize, KT_SETUP_LDS));
    ATTRCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_kt_setup<14>), hipFuncAttributeMaxDynamicSharedMemorySize, KT_SETUP_LDS));
    return hipSuccess;
}
#undef ATTRCHK

hipError_t klaunch_kt_setup(int nr, hipStream_t st, const DevTables *tb, const KtSetupParams &s) {
    const unsigned wgs = (s.n + 255u) / 256u;
    if (nr == 10) hipLaunchKernelGGL(k_kt_setup<10>, dim3(wgs), dim3(256), KT_SETUP_LDS, st, tb, s);
    else if (nr == 12) hipLaunchKernelGGL(k_kt_setup<12>, dim3(wgs), dim3(256), KT_SETUP_LDS, st, tb, s);
    else hipLaunchKernelGGL(k_kt_setup<14>, dim3(wgs), dim3(256), KT_SETUP_LDS, st, tb, s);
    return hipGetLastError();
}

hipError_t klaunch_kt_batch(int nr, int dec, int lg, unsigned wgs, hipStream_t st, const DevTables *tb, const KtParams &p) {
#define LKT(NR, D, LG) hipLaunchKernelGGL((k_kt_batch<NR, D, LG>), dim3(wgs), dim3(BATCH3_LANES(NR)), BATCH3_LDS_BYTES_LG(LG), st, tb, p)
#define LKTN(D, LG) do { if (nr == 10) LKT(10, D, LG); else if (nr == 12) LKT(12, D, LG); else LKT(14, D, LG); } while (0)
    if (lg == 3) { if (dec) LKTN(1, 3); else LKTN(0, 3); }
    else if (lg == 4) { if (dec) LKTN(1, 4); else LKTN(0, 4); }
    else { if (dec) LKTN(1, 6); else LKTN(0, 6); }
#undef LKTN
#undef LKT
    return hipGetLastError();
}
