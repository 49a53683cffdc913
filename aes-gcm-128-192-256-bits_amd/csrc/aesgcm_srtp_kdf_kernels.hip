// aesgcm_srtp_kdf_kernels.hip -- SRTP / SRTCP session keys derived on the device (gfx950): the kernels of aesgcm_srtp_kdf_install_dev and _set_dev and their launchers;
// the host side is aesgcm_srtp_kdf.hip, the lane code (the x block, the AES-CM PRF's blocks, what an entry decides, the records) and the state's layout
// aesgcm_srtp_kdf.h, the slot build it shares with the HKDF family aesgcm_kdf_slot.h.
//
//   k_srtp_kdf_install<NR>   grid = entries x 2 roles, 256 lanes; blockIdx.y is the ROLE, uniform per workgroup (no wave diverges): 0 key, 1 salt.  Both run AES, so
//                            both stage T0 | T2.  Both lanes of an entry come to the same verdict (skdf_install_entry); role 0 reports a refused entry.  A lane
//                            loads the master key into registers, runs its schedule there and encrypts one counter block (the key of AES-192 / AES-256: two).  A key
//                            lane hands the output words to kdf_slot_build: session schedule, H, its powers, nr, fence, marker.  A salt lane stores the slot's
//                            TLS-IV field as aesgcm_keytab_set_tls_iv leaves it.  Neither the master schedule nor the PRF's output is stored anywhere else.
//   k_srtp_kdf_set           a lane per entry: a master key and salt from device memory into their record
// The only atomic of the unit is the status word's minimum (kdf_refuse).  A translation unit of its own: its ISA census (`make asm_srtp_kdf`) is read apart from the
// others', and the HKDF family's census keeps the kernels it had.
#include "aesgcm_srtp_kdf.h"

template <int NR>
__global__ __launch_bounds__(KDF_WG) void k_srtp_kdf_install(const DevTables *__restrict__ tb, const SkdfInstallParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const u32 tid = threadIdx.x, role = blockIdx.y;
    main_fill_lds(smem, nullptr, tb, tid, false, KDF_WG);           // T0 | T2, as k_kt_setup
    __syncthreads();
    const u32 i = blockIdx.x * KDF_WG + tid;
    if (i >= p.n) return;
    u32 rec, slot;
    u64 r;
    if (!skdf_install_entry(p, i, rec, slot, r)) {
        if (role == SKDF_ROLE_KEY) kdf_refuse(p.t.status, i);
        return;
    }
    const u32 lb = (tid & 31u) << 2;
    u32 rk[4 * (NR + 1)], out[8];
    skdf_derive<NR>(p.t, role, p.label[role], rec, r, rk, smem, lb, out);
    KtSlot *d = p.tab + slot;
    if (role == SKDF_ROLE_SALT) {                                    // the session salt's first 12 bytes as three memory-order words, then 0 (KtSlot::xpn)
        *reinterpret_cast<uint4 *>(d->xpn) = make_uint4(out[0], out[1], out[2], 0u);
        return;
    }
#pragma unroll
    for (int w = 0; w < NR - 6; w++) rk[w] = out[w];                 // the master schedule ends here: the session key takes its registers
    kdf_slot_build<NR>(d, rk, smem, lb);
}

__global__ __launch_bounds__(KDF_WG) void k_srtp_kdf_set(const SkdfSetParams p) {
    const u32 i = blockIdx.x * KDF_WG + threadIdx.x;
    if (i < p.n) skdf_set_lane(p, i);
}

// ------------------------------------------------------------------------------------------------ launchers
#define SKDF_INSTALL_LDS (AESGCM_LDS_AES_OFF + AESGCM_LDS_AES)
hipError_t klaunch_srtp_kdf_attributes() {
    return nr_each([](auto NR) {
        return hipFuncSetAttribute(reinterpret_cast<const void *>(&k_srtp_kdf_install<NR()>), hipFuncAttributeMaxDynamicSharedMemorySize, SKDF_INSTALL_LDS);
    });
}

hipError_t klaunch_srtp_kdf_install(int nr, hipStream_t st, const DevTables *tb, const SkdfInstallParams &p) {
    const dim3 grid((p.n + KDF_WG - 1u) / KDF_WG, 2u);
    nr_dispatch(nr, [&](auto NR) { hipLaunchKernelGGL((k_srtp_kdf_install<NR()>), grid, dim3(KDF_WG), SKDF_INSTALL_LDS, st, tb, p); });
    return hipGetLastError();
}

hipError_t klaunch_srtp_kdf_set(hipStream_t st, const SkdfSetParams &p) {
    hipLaunchKernelGGL(k_srtp_kdf_set, dim3((p.n + KDF_WG - 1u) / KDF_WG), dim3(KDF_WG), 0, st, p);
    return hipGetLastError();
}
