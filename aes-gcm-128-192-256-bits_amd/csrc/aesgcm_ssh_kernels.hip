// aesgcm_ssh_kernels.hip -- key tables on SSH binary packets in wire format (gfx950; RFC 5647 AEAD_AES_128_GCM / AEAD_AES_256_GCM, aes128-gcm@openssh.com /
// aes256-gcm@openssh.com): aesgcm_keytab_ssh_crypt_dev's kernel and its launcher; the host side is aesgcm_keytab.hip.
//
//   k_kt_ssh<NR,DEC,LG>     k_kt_tls's TLS 1.3 path (aesgcm_batch3_body.inc, SLOTS = WIRE = true, WIREX = KT_WIREX_SSH) with another cut and another nonce (aesgcm_wirecut.h:
//                           cut_ssh, nonce_iv_add_num).  Packet = packet_length[4] | body | tag[16]; AAD = the four length bytes, which the kernel reads once more than
//                           a TLS header: they must say the body's length, or the packet is refused.  Nonce = the slot's IV (KtSlot::xpn, aesgcm_keytab_set_tls_iv) with
//                           its last eight bytes, a big-endian integer, INCREMENTED by seq[p] -- an addition with its carries, where TLS 1.3 XORs.  No nonce byte is read
//                           from the packet; a refused packet's seq is not read.
// 18 instances, the fixed-size loop (BatchParams::plain) not compiled in.  A translation unit of its own: its ISA census (`make asm_ssh`) is read apart from the
// others', whose instruction streams stay what they were.
#include "aesgcm_keytab.h"
#include "aesgcm_lanes.h"
#include "aesgcm_wirecut.h"
#include "aesgcm_dispatch.h"

template <int NR, int DEC, int LG>                       // DEC: 0 encrypt, 1 decrypt
__global__ __launch_bounds__(BATCH3_LANES(NR), (BATCH3_LANES(NR) + 255) / 256) void k_kt_ssh(const DevTables *__restrict__ tb, const KtWireXParams xp) {
    constexpr bool SLOTS = true, WIRE = true;
    constexpr u32 WIREX = KT_WIREX_SSH;
    const KtWireXParams *const wx = &xp;
    const KtParams *const kt = &xp.w.k;
    const BatchParams &p = xp.w.k.b;
    const aesgcm_wire_fmt *const wf = &xp.w.f;
#include "aesgcm_batch3_body.inc"
}

// ------------------------------------------------------------------------------------------------ launchers
hipError_t klaunch_ssh_attributes() {
    return batch3_each([](auto NR, auto D, auto LG) { return hipFuncSetAttribute(reinterpret_cast<const void *>(&k_kt_ssh<NR(), D(), LG()>), hipFuncAttributeMaxDynamicSharedMemorySize, BATCH3_LDS_BYTES_LG(LG())); });
}

hipError_t klaunch_kt_ssh(int nr, int dec, int lg, unsigned wgs, hipStream_t st, const DevTables *tb, const KtWireXParams &p) {
    batch3_dispatch(nr, dec, lg, [&](auto NR, auto D, auto LG) { hipLaunchKernelGGL((k_kt_ssh<NR(), D(), LG()>), dim3(wgs), dim3(BATCH3_LANES(NR())), BATCH3_LDS_BYTES_LG(LG()), st, tb, p); });
    return hipGetLastError();
}
