// aesgcm_kdf_kernels.hip -- on-device key derivation (gfx950): the kernels of aesgcm_kdf_install_dev, _update_dev and _set_dev and their launchers; the host side is
// aesgcm_kdf.hip, the lane code (SHA-256 / SHA-512 compression, HKDF-Expand-Label as four compressions, what an entry decides) and the state's layout aesgcm_kdf.h.
//
//   k_kdf_install<NR,HL>   grid = entries x roles, 256 lanes; blockIdx.y is the ROLE, uniform per workgroup (no wave diverges): 0 key, 1 iv, 2 aux.  Every lane of an
//                          entry comes to the same verdict (kdf_install_entry); role 0 reports a refused entry.  A key or aux lane expands its label and goes on to
//                          the key schedule ITSELF: kdf_slot_build (aesgcm_kdf_slot.h, k_kt_setup's steps) takes the key's words from the lane's registers.  An iv lane
//                          stores the slot's TLS-IV field as aesgcm_keytab_set_tls_iv leaves it.  No derived value is stored anywhere else.
//   k_kdf_update<HL>       a lane per entry: rec[to] = Expand-Label(rec[from], label 3, hash_len)
//   k_kdf_set              a lane per entry: a secret from device memory into its record
// The only atomic of the unit is the status word's minimum.  A translation unit of its own: its ISA census (`make asm_kdf`) is read apart from the others'.
#include "aesgcm_kdf_slot.h"
#include "aesgcm_kdf.h"

template <int NR, int HL>
__global__ __launch_bounds__(KDF_WG) void k_kdf_install(const DevTables *__restrict__ tb, const KdfInstallParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const u32 tid = threadIdx.x, role = blockIdx.y;
    if (role != KDF_ROLE_IV) {
        main_fill_lds(smem, nullptr, tb, tid, false, KDF_WG);       // T0 | T2, as k_kt_setup
        __syncthreads();
    }
    const u32 i = blockIdx.x * KDF_WG + tid;
    if (i >= p.n) return;
    u32 rec, slot, aux;
    if (!kdf_install_entry(p, i, rec, slot, aux)) {
        if (role == KDF_ROLE_KEY) kdf_refuse(p.t.status, i);
        return;
    }
    if (role == KDF_ROLE_AUX) {
        if (aux == KDF_NO_SLOT) return;                              // the entry keeps its hp / sn slot (a key update)
        slot = aux;
    }
    u32 sec[HL / 4], out[HL / 4];
    kdf_load<HL>(p.t, rec, sec);
    kdf_expand<HL>(sec, p.msg[role], out);
    KtSlot *d = p.tab + slot;
    if (role == KDF_ROLE_IV) {                                       // three memory-order words, then 0 (KtSlot::xpn)
        *reinterpret_cast<uint4 *>(d->xpn) = make_uint4(bswap32(out[0]), bswap32(out[1]), bswap32(out[2]), 0u);
        return;
    }
    u32 rk[4 * (NR + 1)];
#pragma unroll
    for (int w = 0; w < NR - 6; w++) rk[w] = bswap32(out[w]);
    kdf_slot_build<NR>(d, rk, smem, (tid & 31u) << 2);
}

template <int HL>
__global__ __launch_bounds__(KDF_WG) void k_kdf_update(const KdfUpdateParams p) {
    const u32 i = blockIdx.x * KDF_WG + threadIdx.x;
    if (i < p.n) kdf_update_lane<HL>(p, i);
}

__global__ __launch_bounds__(KDF_WG) void k_kdf_set(const KdfSetParams p) {
    const u32 i = blockIdx.x * KDF_WG + threadIdx.x;
    if (i < p.n) kdf_set_lane(p, i);
}

// ------------------------------------------------------------------------------------------------ launchers
#define KDF_INSTALL_LDS (AESGCM_LDS_AES_OFF + AESGCM_LDS_AES)
hipError_t klaunch_kdf_attributes() {
    return nr_each([](auto NR) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&k_kdf_install<NR(), 32>), hipFuncAttributeMaxDynamicSharedMemorySize, KDF_INSTALL_LDS);
        return e != hipSuccess ? e : hipFuncSetAttribute(reinterpret_cast<const void *>(&k_kdf_install<NR(), 48>), hipFuncAttributeMaxDynamicSharedMemorySize, KDF_INSTALL_LDS);
    });
}

hipError_t klaunch_kdf_install(int nr, hipStream_t st, const DevTables *tb, const KdfInstallParams &p) {
    const dim3 grid((p.n + KDF_WG - 1u) / KDF_WG, p.aux_slots ? 3u : 2u);
    nr_dispatch(nr, [&](auto NR) {
        if (p.t.hash_len == 48u) hipLaunchKernelGGL((k_kdf_install<NR(), 48>), grid, dim3(KDF_WG), KDF_INSTALL_LDS, st, tb, p);
        else hipLaunchKernelGGL((k_kdf_install<NR(), 32>), grid, dim3(KDF_WG), KDF_INSTALL_LDS, st, tb, p);
    });
    return hipGetLastError();
}

hipError_t klaunch_kdf_update(hipStream_t st, const KdfUpdateParams &p) {
    const dim3 grid((p.n + KDF_WG - 1u) / KDF_WG);
    if (p.t.hash_len == 48u) hipLaunchKernelGGL(k_kdf_update<48>, grid, dim3(KDF_WG), 0, st, p);
    else hipLaunchKernelGGL(k_kdf_update<32>, grid, dim3(KDF_WG), 0, st, p);
    return hipGetLastError();
}

hipError_t klaunch_kdf_set(hipStream_t st, const KdfSetParams &p) {
    hipLaunchKernelGGL(k_kdf_set, dim3((p.n + KDF_WG - 1u) / KDF_WG), dim3(KDF_WG), 0, st, p);
    return hipGetLastError();
}
