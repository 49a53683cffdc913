// aesgcm_sshkdf_kernels.hip -- SSH's key derivation on the device (gfx950; RFC 4253 7.2): the kernels of aesgcm_sshkdf_install_dev and _set_dev and their launchers;
// the host side is aesgcm_sshkdf.hip, the lane code (the plain hash whose block count is a run-time value, what an entry decides, the records) and the state's layout
// aesgcm_sshkdf.h, the slot build it shares with the other derivation families aesgcm_kdf_slot.h.
//
//   k_sshk_install<NR,HL>    grid = entries x 4 letters, 256 lanes; blockIdx.y is the LETTER behind 'A', uniform per workgroup (no wave diverges on it): 0 'A' the IV
//                            client to server, 1 'B' the IV server to client, 2 'C' the key client to server, 3 'D' the key server to client.  A direction the call
//                            does not install (its slot array is NULL) leaves at once.  Every lane of an entry comes to the same verdict (sshk_entry); ONE letter
//                            reports a refused entry: 'A', or 'B' where the call has no client-to-server array.  An IV lane stores the slot's IV field as
//                            aesgcm_keytab_set_tls_iv leaves it.  A key lane hands the digest's first words to kdf_slot_build: schedule, H, its powers, nr, fence,
//                            marker -- the key goes from the lane's registers into the schedule and lies nowhere else.
//                            The block loop of the hash (sshk_hash) is the one place where lanes of a wave run different trip counts: secrets differ in length.
//   k_sshk_set               a lane per entry: a secret and a session identifier from device memory into their record
// The only atomic of the unit is the status word's minimum (kdf_refuse).  A translation unit of its own: its ISA census (`make asm_sshkdf`) is read apart from the
// others', and the other families' censuses keep the kernels they had.
#include "aesgcm_sshkdf.h"
#include "aesgcm_kdf_slot.h"

template <int NR, int HL>
__global__ __launch_bounds__(KDF_WG) void k_sshk_install(const DevTables *__restrict__ tb, const SshkInstallParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const u32 tid = threadIdx.x, dir = blockIdx.y & 1u, role = blockIdx.y >> 1;
    if (!p.slots[dir]) return;                                       // (uniform: the call installs nothing for this direction)
    if (role == SSHK_ROLE_KEY) {
        main_fill_lds(smem, nullptr, tb, tid, false, KDF_WG);       // T0 | T2, as k_kt_setup
        __syncthreads();
    }
    const u32 i = blockIdx.x * KDF_WG + tid;
    if (i >= p.n) return;
    u32 rec, slot[2];
    if (!sshk_entry(p, i, rec, slot)) {
        if (role == SSHK_ROLE_IV && (dir == SSHK_C2S || !p.slots[SSHK_C2S])) kdf_refuse(p.t.status, i);
        return;
    }
    if (slot[dir] == SSHK_NONE) return;                              // the entry installs the other direction only
    u32 out[HL / 4];
    sshk_derive<HL>(p.t, rec, role, dir, out);
    KtSlot *d = p.tab + slot[dir];
    if (role == SSHK_ROLE_IV) {                                      // three memory-order words, then 0 (KtSlot::xpn)
        *reinterpret_cast<uint4 *>(d->xpn) = make_uint4(bswap32(out[0]), bswap32(out[1]), bswap32(out[2]), 0u);
        return;
    }
    u32 rk[4 * (NR + 1)];
#pragma unroll
    for (int w = 0; w < NR - 6; w++) rk[w] = bswap32(out[w]);
    kdf_slot_build<NR>(d, rk, smem, (tid & 31u) << 2);
}

__global__ __launch_bounds__(KDF_WG) void k_sshk_set(const SshkSetParams p) {
    const u32 i = blockIdx.x * KDF_WG + threadIdx.x;
    if (i < p.n) sshk_set_lane(p, i);
}

// ------------------------------------------------------------------------------------------------ launchers
#define SSHK_INSTALL_LDS (AESGCM_LDS_AES_OFF + AESGCM_LDS_AES)
// the nine instances: nr 10 -> 10, 12 -> 12, anything else -> 14; hash_len 32 -> 32, 48 -> 48, anything else -> 64 (create lets nothing else in)
using sshk_set_t = kset<nr_list, klist<32, 48, 64>>;

hipError_t klaunch_sshk_attributes() {
    return set_each(sshk_set_t{}, [](auto NR, auto HL) {
        return hipFuncSetAttribute(reinterpret_cast<const void *>(&k_sshk_install<NR(), HL()>), hipFuncAttributeMaxDynamicSharedMemorySize, SSHK_INSTALL_LDS);
    });
}

hipError_t klaunch_sshk_install(int nr, hipStream_t st, const DevTables *tb, const SshkInstallParams &p) {
    const dim3 grid((p.n + KDF_WG - 1u) / KDF_WG, 4u);
    set_pick(sshk_set_t{}, [&](auto NR, auto HL) { hipLaunchKernelGGL((k_sshk_install<NR(), HL()>), grid, dim3(KDF_WG), SSHK_INSTALL_LDS, st, tb, p); }, nr, (int)p.t.hash_len);
    return hipGetLastError();
}

hipError_t klaunch_sshk_set(hipStream_t st, const SshkSetParams &p) {
    hipLaunchKernelGGL(k_sshk_set, dim3((p.n + KDF_WG - 1u) / KDF_WG), dim3(KDF_WG), 0, st, p);
    return hipGetLastError();
}
