// aesgcm_prf12_kernels.hip -- the TLS 1.2 PRF on the device (gfx950): the kernels of aesgcm_prf12_install_dev, _export_srtp_dev and _set_dev and their launchers; the
// host side is aesgcm_prf12.hip, the lane code (the seed, the three HMACs of fixed shape, P_hash and what a lane takes of it, what an entry decides, the records) and
// the state's layout aesgcm_prf12.h, the slot build it shares with the two other derivation families aesgcm_kdf_slot.h.
//
//   k_prf12_install<NR,HL>   grid = entries x 4 roles, 256 lanes; blockIdx.y is the ROLE, uniform per workgroup (no wave diverges): 0 the client's key, 1 the server's
//                            key, 2 the client's IV, 3 the server's IV.  A role whose direction the call does not install (its slot array is NULL) leaves at once.
//                            Every lane of an entry comes to the same verdict (prf12_entry); ONE role reports a refused entry: 0, or 1 where the call has no client slots.  A lane runs P_hash up to the last
//                            T(j) its words need.  A key lane stages T0 | T2 and hands its words to kdf_slot_build: schedule, H, its powers, nr, fence, marker.
//                            An IV lane needs no LDS and stores the slot's TLS-IV field as aesgcm_keytab_set_tls_iv leaves it for IV | 8 zero bytes.
//   k_prf12_export<HL>       grid = entries x 2 directions; a lane derives its direction's key and salt from the exporter's output and stores the SRTP master
//                            record whole (prf12_store_master: what aesgcm_srtp_kdf_set_dev makes of them), marker last; the first direction the call has reports a refusal
//   k_prf12_set              a lane per entry: a master secret and the two randoms from device memory into their record
// The only atomic of the unit is the status word's minimum (kdf_refuse).  A translation unit of its own: its ISA census (`make asm_prf12`) is read apart from the
// others', and the other families' censuses keep the kernels they had.
#include "aesgcm_prf12.h"

template <int NR, int HL>
__global__ __launch_bounds__(KDF_WG) void k_prf12_install(const DevTables *__restrict__ tb, const Prf12InstallParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const u32 tid = threadIdx.x, role = blockIdx.y, dir = role & 1u;
    if (!p.slots[dir]) return;                                       // (uniform: the call installs nothing for this direction)
    if (role < PRF12_ROLE_IV) {
        main_fill_lds(smem, nullptr, tb, tid, false, KDF_WG);       // T0 | T2, as k_kt_setup
        __syncthreads();
    }
    const u32 i = blockIdx.x * KDF_WG + tid;
    if (i >= p.n) return;
    u32 rec, slot[2];
    if (!prf12_entry(p.t, p.idx, p.slots, p.n_slots, i, rec, slot)) {
        if (role == 0u || (role == 1u && !p.slots[PRF12_CLIENT])) kdf_refuse(p.t.status, i);
        return;
    }
    if (slot[dir] == PRF12_NONE) return;                             // the entry installs the other direction only
    constexpr int NK = NR - 6;
    u32 out[NK];
    prf12_install_derive<HL, NK>(p, rec, role, out);
    KtSlot *d = p.tab + slot[dir];
    if (role >= PRF12_ROLE_IV) {                                     // the four bytes as a memory-order word, then the explicit nonce's place and the last word zero (KtSlot::xpn)
        *reinterpret_cast<uint4 *>(d->xpn) = make_uint4(bswap32(out[0]), 0u, 0u, 0u);
        return;
    }
    u32 rk[4 * (NR + 1)];
#pragma unroll
    for (int w = 0; w < NK; w++) rk[w] = bswap32(out[w]);
    kdf_slot_build<NR>(d, rk, smem, (tid & 31u) << 2);
}

template <int HL>
__global__ __launch_bounds__(KDF_WG) void k_prf12_export(const Prf12ExportParams p) {
    const u32 dir = blockIdx.y;
    if (!p.recs[dir]) return;                                        // (uniform)
    const u32 i = blockIdx.x * KDF_WG + threadIdx.x;
    if (i >= p.n) return;
    u32 rec, to[2];
    if (!prf12_entry(p.t, p.idx, p.recs, p.m.n_masters, i, rec, to)) {
        if (dir == PRF12_CLIENT || !p.recs[PRF12_CLIENT]) kdf_refuse(p.t.status, i);
        return;
    }
    if (to[dir] == PRF12_NONE) return;
    u32 key[8], salt[3];
    prf12_export_derive<HL>(p, rec, dir, key, salt);
    prf12_store_master(p.m, to[dir], key, salt);
}

__global__ __launch_bounds__(KDF_WG) void k_prf12_set(const Prf12SetParams p) {
    const u32 i = blockIdx.x * KDF_WG + threadIdx.x;
    if (i < p.n) prf12_set_lane(p, i);
}

// ------------------------------------------------------------------------------------------------ launchers
#define PRF12_INSTALL_LDS (AESGCM_LDS_AES_OFF + AESGCM_LDS_AES)
hipError_t klaunch_prf12_attributes() {
    return nr_each([](auto NR) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&k_prf12_install<NR(), 32>), hipFuncAttributeMaxDynamicSharedMemorySize, PRF12_INSTALL_LDS);
        return e != hipSuccess ? e : hipFuncSetAttribute(reinterpret_cast<const void *>(&k_prf12_install<NR(), 48>), hipFuncAttributeMaxDynamicSharedMemorySize, PRF12_INSTALL_LDS);
    });
}

hipError_t klaunch_prf12_install(int nr, hipStream_t st, const DevTables *tb, const Prf12InstallParams &p) {
    const dim3 grid((p.n + KDF_WG - 1u) / KDF_WG, 4u);
    nr_dispatch(nr, [&](auto NR) {
        if (p.t.hash_len == 48u) hipLaunchKernelGGL((k_prf12_install<NR(), 48>), grid, dim3(KDF_WG), PRF12_INSTALL_LDS, st, tb, p);
        else hipLaunchKernelGGL((k_prf12_install<NR(), 32>), grid, dim3(KDF_WG), PRF12_INSTALL_LDS, st, tb, p);
    });
    return hipGetLastError();
}

hipError_t klaunch_prf12_export(hipStream_t st, const Prf12ExportParams &p) {
    const dim3 grid((p.n + KDF_WG - 1u) / KDF_WG, 2u);
    if (p.t.hash_len == 48u) hipLaunchKernelGGL(k_prf12_export<48>, grid, dim3(KDF_WG), 0, st, p);
    else hipLaunchKernelGGL(k_prf12_export<32>, grid, dim3(KDF_WG), 0, st, p);
    return hipGetLastError();
}

hipError_t klaunch_prf12_set(hipStream_t st, const Prf12SetParams &p) {
    hipLaunchKernelGGL(k_prf12_set, dim3((p.n + KDF_WG - 1u) / KDF_WG), dim3(KDF_WG), 0, st, p);
    return hipGetLastError();
}
