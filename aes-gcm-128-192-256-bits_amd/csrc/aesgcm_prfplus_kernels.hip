// aesgcm_prfplus_kernels.hip -- IKEv2's prf+ on the device (gfx950): the kernels of aesgcm_prfplus_install_dev and _set_dev and their launchers; the host side is
// aesgcm_prfplus.hip, the lane code (the HMAC whose block count is a run-time value, prf+ and what a lane takes of it, what an entry decides, the records) and the
// state's layout aesgcm_prfplus.h, the slot build it shares with the three other derivation families aesgcm_kdf_slot.h.
//
//   k_prfp_install<NR,HL>    grid = entries x 2 directions, 256 lanes; blockIdx.y is the DIRECTION, uniform per workgroup (no wave diverges on it): 0 initiator to
//                            responder, 1 responder to initiator.  A direction the call does not install (its slot array is NULL) leaves at once.  Both lanes of an
//                            entry come to the same verdict (prfp_entry); ONE direction reports a refused entry: i2r, or r2i where the call has no i2r array.  A lane
//                            runs prf+ up to the last T(n) its NK + 1 words need -- the key and the salt together, no lane of its own for the salt -- stores the
//                            slot's salt field as aesgcm_keytab_set_salt leaves it for salt | 00 00 00 00, stages T0 | T2 and hands the key words to kdf_slot_build:
//                            schedule, H, its powers, nr, fence, marker.  The marker stays the slot's last store, so the salt goes in front of the build.
//                            The block loop of the HMAC (prfp_hmac) is the one place where lanes of a wave run different trip counts: seeds differ in length.
//   k_prfp_set               a lane per entry: an SK_d from device memory into its record
// The only atomic of the unit is the status word's minimum (kdf_refuse).  A translation unit of its own: its ISA census (`make asm_prfplus`) is read apart from the
// others', and the other families' censuses keep the kernels they had.
#include "aesgcm_prfplus.h"
#include "aesgcm_kdf_slot.h"

template <int NR, int HL>
__global__ __launch_bounds__(KDF_WG) void k_prfp_install(const DevTables *__restrict__ tb, const PrfpInstallParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const u32 tid = threadIdx.x, dir = blockIdx.y;
    if (!p.slots[dir]) return;                                       // (uniform: the call installs nothing for this direction)
    main_fill_lds(smem, nullptr, tb, tid, false, KDF_WG);           // T0 | T2, as k_kt_setup
    __syncthreads();
    const u32 i = blockIdx.x * KDF_WG + tid;
    if (i >= p.n) return;
    u32 rec, slot[2], len;
    const unsigned char *s;
    if (!prfp_entry(p, i, rec, slot, s, len)) {
        if (dir == PRFP_I2R || !p.slots[PRFP_I2R]) kdf_refuse(p.t.status, i);
        return;
    }
    if (slot[dir] == PRFP_NONE) return;                              // the entry installs the other direction only
    constexpr int NK = NR - 6;
    u32 out[NK + 1];
    prfp_install_derive<HL, NK>(p, rec, dir, s, len, out);
    KtSlot *d = p.tab + slot[dir];
    *reinterpret_cast<uint2 *>(d->salt) = make_uint2(bswap32(out[NK]), 0u);      // the four bytes as a memory-order word, the field's other four zero
    u32 rk[4 * (NR + 1)];
#pragma unroll
    for (int w = 0; w < NK; w++) rk[w] = bswap32(out[w]);
    kdf_slot_build<NR>(d, rk, smem, (tid & 31u) << 2);
}

__global__ __launch_bounds__(KDF_WG) void k_prfp_set(const PrfpSetParams p) {
    const u32 i = blockIdx.x * KDF_WG + threadIdx.x;
    if (i < p.n) prfp_set_lane(p, i);
}

// ------------------------------------------------------------------------------------------------ launchers
#define PRFP_INSTALL_LDS (AESGCM_LDS_AES_OFF + AESGCM_LDS_AES)
// the nine instances: nr 10 -> 10, 12 -> 12, anything else -> 14; hash_len 32 -> 32, 48 -> 48, anything else -> 64 (create lets nothing else in)
using prfp_set_t = kset<nr_list, klist<32, 48, 64>>;

hipError_t klaunch_prfp_attributes() {
    return set_each(prfp_set_t{}, [](auto NR, auto HL) {
        return hipFuncSetAttribute(reinterpret_cast<const void *>(&k_prfp_install<NR(), HL()>), hipFuncAttributeMaxDynamicSharedMemorySize, PRFP_INSTALL_LDS);
    });
}

hipError_t klaunch_prfp_install(int nr, hipStream_t st, const DevTables *tb, const PrfpInstallParams &p) {
    const dim3 grid((p.n + KDF_WG - 1u) / KDF_WG, 2u);
    set_pick(prfp_set_t{}, [&](auto NR, auto HL) { hipLaunchKernelGGL((k_prfp_install<NR(), HL()>), grid, dim3(KDF_WG), PRFP_INSTALL_LDS, st, tb, p); }, nr, (int)p.t.hash_len);
    return hipGetLastError();
}

hipError_t klaunch_prfp_set(hipStream_t st, const PrfpSetParams &p) {
    hipLaunchKernelGGL(k_prfp_set, dim3((p.n + KDF_WG - 1u) / KDF_WG), dim3(KDF_WG), 0, st, p);
    return hipGetLastError();
}
