// aesgcm_wirex_kernels.hip -- key tables on frames in wire format whose 64-bit packet / sequence number is only half on the wire (gfx950): aesgcm_keytab_frames_crypt_x_dev's
// kernel and its launcher; the host side is aesgcm_keytab.hip.
//
//   k_kt_wirex<NR,DEC,LG,EXT>   k_kt_wire's loop (aesgcm_batch3_body.inc, SLOTS = WIRE = true, WIREX = EXT) with one more 4-byte load per frame: hi[p], the upper half of
//                           the frame's number, which the caller assigned (transmit) or recovered from its window (receive).  EXT says where it goes:
//                             AESGCM_WIREX_XPN  the nonce = the slot's 12-byte XPN salt XOR (the slot's SSCI | be32(hi) | the SecTAG's four PN bytes); the rest as k_kt_wire
//                             AESGCM_WIREX_ESN  the AAD = SPI | be32(hi) | sequence number, one block built in registers (96 bits in the length block); nonce, pass-through
//                                               header and payload as k_kt_wire
//                           A frame it cannot take is refused as k_kt_wire refuses it, and its hi is not read.
// The mode is a template argument: 36 instances.  As a kernel parameter (one scalar branch per frame) it cost the AES-256 decrypt instances of 16 and 64 lanes per frame,
// which sit at 128 registers in k_kt_wire already, eight bytes of scratch -- a launch-uniform flag that no longer fitted the scalar registers.  For the same reason the
// body's loop for fixed-size records without AAD (BatchParams::plain), which a call of frames never takes, is not compiled into these kernels (that form was not tried
// again as a kernel parameter afterwards).  Every instance: no scratch, 92 - 126 registers.
// A translation unit of its own: its ISA census (`make asm_wirex`) is read apart from k_kt_wire's (`make asm_wire`), whose instruction streams stay what they were.
#include "aesgcm_keytab.h"
#include "aesgcm_lanes.h"
#include "aesgcm_wirecut.h"
#include "aesgcm_dispatch.h"

template <int NR, int DEC, int LG, u32 EXT>              // DEC: 0 encrypt, 1 decrypt; EXT: AESGCM_WIREX_XPN or AESGCM_WIREX_ESN
__global__ __launch_bounds__(BATCH3_LANES(NR), (BATCH3_LANES(NR) + 255) / 256) void k_kt_wirex(const DevTables *__restrict__ tb, const KtWireXParams xp) {
    static_assert(EXT == AESGCM_WIREX_XPN || EXT == AESGCM_WIREX_ESN, "without an extension the kernel is k_kt_wire");
    constexpr bool SLOTS = true, WIRE = true;
    constexpr u32 WIREX = EXT;
    const KtWireXParams *const wx = &xp;
    const KtParams *const kt = &xp.w.k;
    const BatchParams &p = xp.w.k.b;
    const aesgcm_wire_fmt *const wf = &xp.w.f;
#include "aesgcm_batch3_body.inc"
}

// ------------------------------------------------------------------------------------------------ launchers
hipError_t klaunch_wirex_attributes() {
    return batch3v_each<AESGCM_WIREX_XPN, AESGCM_WIREX_ESN>([](auto NR, auto D, auto LG, auto V) {
        return hipFuncSetAttribute(reinterpret_cast<const void *>(&k_kt_wirex<NR(), D(), LG(), V()>), hipFuncAttributeMaxDynamicSharedMemorySize, BATCH3_LDS_BYTES_LG(LG()));
    });
}

hipError_t klaunch_kt_wirex(unsigned ext, int nr, int dec, int lg, unsigned wgs, hipStream_t st, const DevTables *tb, const KtWireXParams &p) {
    if (ext != AESGCM_WIREX_XPN && ext != AESGCM_WIREX_ESN) return hipErrorInvalidValue;
    batch3v_dispatch<AESGCM_WIREX_XPN, AESGCM_WIREX_ESN>(nr, dec, lg, (int)ext, [&](auto NR, auto D, auto LG, auto V) {
        hipLaunchKernelGGL((k_kt_wirex<NR(), D(), LG(), V()>), dim3(wgs), dim3(BATCH3_LANES(NR())), BATCH3_LDS_BYTES_LG(LG()), st, tb, p);
    });
    return hipGetLastError();
}
