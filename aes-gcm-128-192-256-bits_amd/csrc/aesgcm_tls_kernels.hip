// aesgcm_tls_kernels.hip -- key tables on TLS records in wire format (gfx950): aesgcm_keytab_records_crypt_dev's kernel and its launcher; the host side is aesgcm_keytab.hip.
//
//   k_kt_tls<NR,DEC,LG,VER>   k_kt_wire's loop (aesgcm_batch3_body.inc, SLOTS = WIRE = true, WIREX = KT_WIREX_TLS13 / KT_WIREX_TLS12) with one 8-byte load per record: seq[p],
//                           its 64-bit sequence number, which no TLS record carries.  The slot's 12-byte IV lies in KtSlot::xpn (aesgcm_keytab_set_tls_iv).  VER says where the
//                           number goes:
//                             AESGCM_TLS_13  record = hdr[5] | payload | tag[16]; nonce = the slot's IV XOR (00 00 00 00 | be64(seq)), no nonce byte is read from the record;
//                                            AAD = the five header bytes: k_kt_wire's ordinary path with the format {5, 5, 5, 0, 16, 0}
//                             AESGCM_TLS_12  record = hdr[5] | explicit nonce[8] | payload | tag[16]; nonce = the slot IV's first four bytes, then the explicit eight (the body's
//                                            4-byte-salt path, format {13, 13, 5, 4, 16, 0}); AAD = be64(seq) | hdr[0..3) | be16(payload length), one block built in registers
//                                            where ESN builds its own (104 bits in the length block), the length taken from the offsets
//                           A record it cannot take -- k_kt_wire's refusals, and one of more than 5 + 65535 bytes -- is refused as k_kt_wire refuses a frame, and its seq is not read.
// The version is a template argument, as k_kt_wirex's mode is and for its reason (a launch-uniform flag cost the AES-256 decrypt instances scratch): 36 instances, and the
// loop for fixed-size records (BatchParams::plain) is not compiled in.  Every instance: no scratch, at most 128 registers.
// A translation unit of its own: its ISA census (`make asm_tls`) is read apart from the others', whose instruction streams stay what they were.
#include "aesgcm_keytab.h"
#include "aesgcm_lanes.h"
#include "aesgcm_wirecut.h"
#include "aesgcm_dispatch.h"

template <int NR, int DEC, int LG, u32 VER>              // DEC: 0 encrypt, 1 decrypt; VER: AESGCM_TLS_13 or AESGCM_TLS_12
__global__ __launch_bounds__(BATCH3_LANES(NR), (BATCH3_LANES(NR) + 255) / 256) void k_kt_tls(const DevTables *__restrict__ tb, const KtWireXParams xp) {
    static_assert(VER == AESGCM_TLS_13 || VER == AESGCM_TLS_12, "TLS 1.3 or TLS 1.2");
    constexpr bool SLOTS = true, WIRE = true;
    constexpr u32 WIREX = VER == AESGCM_TLS_13 ? KT_WIREX_TLS13 : KT_WIREX_TLS12;
    const KtWireXParams *const wx = &xp;
    const KtParams *const kt = &xp.w.k;
    const BatchParams &p = xp.w.k.b;
    const aesgcm_wire_fmt *const wf = &xp.w.f;
#include "aesgcm_batch3_body.inc"
}

// ------------------------------------------------------------------------------------------------ launchers
hipError_t klaunch_tls_attributes() {
    return batch3v_each<AESGCM_TLS_13, AESGCM_TLS_12>([](auto NR, auto D, auto LG, auto V) {
        return hipFuncSetAttribute(reinterpret_cast<const void *>(&k_kt_tls<NR(), D(), LG(), V()>), hipFuncAttributeMaxDynamicSharedMemorySize, BATCH3_LDS_BYTES_LG(LG()));
    });
}

hipError_t klaunch_kt_tls(unsigned version, int nr, int dec, int lg, unsigned wgs, hipStream_t st, const DevTables *tb, const KtWireXParams &p) {
    if (version != AESGCM_TLS_13 && version != AESGCM_TLS_12) return hipErrorInvalidValue;
    batch3v_dispatch<AESGCM_TLS_13, AESGCM_TLS_12>(nr, dec, lg, (int)version, [&](auto NR, auto D, auto LG, auto V) {
        hipLaunchKernelGGL((k_kt_tls<NR(), D(), LG(), V()>), dim3(wgs), dim3(BATCH3_LANES(NR())), BATCH3_LDS_BYTES_LG(LG()), st, tb, p);
    });
    return hipGetLastError();
}
