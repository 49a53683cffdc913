// aesgcm_mka_kernels.hip -- MACsec's MKA on the device (gfx950): the kernels of aesgcm_mka_install_dev, _unwrap_dev and _set_dev and their launchers; the host side is
// aesgcm_mka.hip, the lane code (AES-CMAC and the KDF over it, the RFC 3394 steps, the inverse cipher, what an entry decides, the records) and the state's layout
// aesgcm_mka.h, the slot build it shares with the four other derivation families aesgcm_kdf_slot.h.
//
//   k_mka_install<NRC,NRS>   grid = entries, 256 lanes, A LANE PER ENTRY.  The lane loads the CAK into registers, runs its schedule there, forms K1 / K2, runs the
//                            CBC-MAC over ctr | "IEEE8021 SAK" | 0 | context | be16(bits) once or twice and hands the output words to kdf_slot_build: the SAK's
//                            schedule, H, its powers, nr, fence, marker.  Where the call asked for wrapped output (uniform for the launch) the SAME LANE derives the KEK
//                            in between, runs its schedule over the CAK's registers, does the 6 n wrap steps and stores the key_len + 8 public bytes: the wrap needs
//                            the SAK, and a second role on blockIdx.y would run the SAK's CBC-MACs -- up to 130 blocks each -- a second time to have it.
//   k_mka_unwrap<NRC,NRS>    grid = entries, 256 lanes, a lane per entry.  The workgroup stages T0 | T2 and builds the 256-byte inverse S-box behind them
//                            (mka_fill_inv).  The lane derives the KEK, runs its schedule, unwraps with the inverse cipher over the forward round keys, checks
//                            the recovered initial value and hands the candidate to kdf_slot_build -- or refuses, and the candidate dies in its registers.
//   k_mka_set                a lane per entry: a CAK and its Keyid from device memory into their record
// The block loop of the CBC-MAC (mka_prf) is the one place where lanes of a wave run different trip counts: contexts differ in length.  Neither the CAK's schedule, the
// KEK, its schedule, a CMAC subkey nor an unwrapped candidate is stored anywhere.  The only atomic of the unit is the status word's minimum (kdf_refuse).  A translation
// unit of its own: its ISA census (`make asm_mka`) is read apart from the others', and the other families' censuses keep the kernels they had.
#include "aesgcm_mka.h"

template <int NRC, int NRS>
__global__ __launch_bounds__(KDF_WG) void k_mka_install(const DevTables *__restrict__ tb, const MkaInstallParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const u32 tid = threadIdx.x;
    main_fill_lds(smem, nullptr, tb, tid, false, KDF_WG);           // T0 | T2, as k_kt_setup
    __syncthreads();
    const u32 i = blockIdx.x * KDF_WG + tid;
    if (i >= p.n) return;
    const u32 lb = (tid & 31u) << 2;
    u32 rk[4 * ((NRC > NRS ? NRC : NRS) + 1)], slot;
    if (!mka_install_lane<NRC, NRS>(p, i, smem, lb, rk, slot)) return;
    kdf_slot_build<NRS>(p.tab + slot, rk, smem, lb);
}

template <int NRC, int NRS>
__global__ __launch_bounds__(KDF_WG) void k_mka_unwrap(const DevTables *__restrict__ tb, const MkaUnwrapParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const u32 tid = threadIdx.x;
    main_fill_lds(smem, nullptr, tb, tid, false, KDF_WG);
    __syncthreads();
    mka_fill_inv(smem, tid);                                         // (KDF_WG is 256 lanes: one per S-box value)
    __syncthreads();
    const u32 i = blockIdx.x * KDF_WG + tid;
    if (i >= p.n) return;
    const u32 lb = (tid & 31u) << 2;
    u32 rk[4 * ((NRC > NRS ? NRC : NRS) + 1)], slot;
    if (!mka_unwrap_lane<NRC, NRS>(p, i, smem, lb, rk, slot)) return;
    kdf_slot_build<NRS>(p.tab + slot, rk, smem, lb);
}

__global__ __launch_bounds__(KDF_WG) void k_mka_set(const MkaSetParams p) {
    const u32 i = blockIdx.x * KDF_WG + threadIdx.x;
    if (i < p.n) mka_set_lane(p, i);
}

// ------------------------------------------------------------------------------------------------ launchers
static_assert(KDF_WG == 256u, "mka_fill_inv: a lane per S-box value");
// the four instances of each: the CAK's rounds 10 -> 10, anything else -> 14; the key table's rounds the same (the host lets no AES-192 in)
using mka_set_t = kset<klist<10, 14>, klist<10, 14>>;

hipError_t klaunch_mka_attributes() {
    return set_each(mka_set_t{}, [](auto NRC, auto NRS) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&k_mka_install<NRC(), NRS()>), hipFuncAttributeMaxDynamicSharedMemorySize, MKA_LDS_INV_OFF);
        if (e != hipSuccess) return e;
        return hipFuncSetAttribute(reinterpret_cast<const void *>(&k_mka_unwrap<NRC(), NRS()>), hipFuncAttributeMaxDynamicSharedMemorySize, MKA_LDS_BYTES);
    });
}

hipError_t klaunch_mka_install(int nr, hipStream_t st, const DevTables *tb, const MkaInstallParams &p) {
    const dim3 grid((p.n + KDF_WG - 1u) / KDF_WG);
    set_pick(mka_set_t{}, [&](auto NRC, auto NRS) { hipLaunchKernelGGL((k_mka_install<NRC(), NRS()>), grid, dim3(KDF_WG), MKA_LDS_INV_OFF, st, tb, p); }, (int)p.t.cak_len / 4 + 6, nr);
    return hipGetLastError();
}

hipError_t klaunch_mka_unwrap(int nr, hipStream_t st, const DevTables *tb, const MkaUnwrapParams &p) {
    const dim3 grid((p.n + KDF_WG - 1u) / KDF_WG);
    set_pick(mka_set_t{}, [&](auto NRC, auto NRS) { hipLaunchKernelGGL((k_mka_unwrap<NRC(), NRS()>), grid, dim3(KDF_WG), MKA_LDS_BYTES, st, tb, p); }, (int)p.t.cak_len / 4 + 6, nr);
    return hipGetLastError();
}

hipError_t klaunch_mka_set(hipStream_t st, const MkaSetParams &p) {
    hipLaunchKernelGGL(k_mka_set, dim3((p.n + KDF_WG - 1u) / KDF_WG), dim3(KDF_WG), 0, st, p);
    return hipGetLastError();
}
