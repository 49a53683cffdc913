// aesgcm_srtp_kernels.hip -- key tables on SRTP and SRTCP packets in wire format (gfx950; RFC 7714 AEAD_AES_128_GCM / AEAD_AES_256_GCM over RFC 3711's packets):
// aesgcm_keytab_srtp_crypt_dev's kernel and its launchers; the host side is aesgcm_keytab.hip.
//
//   k_kt_srtp<NR,DEC,LG,KIND>  the AEAD (aesgcm_batch3_body.inc, SLOTS = WIRE = true, WIREX = KT_WIREX_SRTP / KT_WIREX_SRTCP).  KIND says which packet:
//                                AESGCM_SRTP_RTP   packet = rtp_hdr | payload | tag[16] | mki.  The header's length is parsed on the device: 12 bytes, 4 per CSRC (the first
//                                                  byte's low four bits), and with its X bit (0x10) an extension of 4 bytes and 4 times the 16-bit length in its bytes 2, 3.
//                                                  AAD = the header.  Nonce = the slot's 12-byte salt (KtSlot::xpn) XOR (00 00 | SSRC | be32(hi[p]) | SEQ), hi[p] the rollover
//                                                  counter, which is not on the wire.
//                                AESGCM_SRTP_RTCP  packet = rtcp_hdr[8] | payload | tag[16] | W[4] | mki, W = E | 31-bit index, read from the wire.  Nonce = the salt XOR
//                                                  (00 00 | SSRC | 00 00 | 0, index).  E set: AAD = the header | W, one block built in registers.  E clear: nothing is
//                                                  encrypted and the AAD is everything in front of the tag, then W -- two pieces, whose seam falls on any byte of the last AAD
//                                                  block or two (load_block_split, aesgcm_stream.h).  E is per packet.
//                              In both the tag is not the packet's last bytes: the lane that writes or compares it also copies what follows it when out of place.
// One launch, no number but the rollover counter from outside the packet.  36 instances; the loop for fixed-size records (BatchParams::plain) is not compiled in; every
// one: no scratch, at most 128 registers.
// A translation unit of its own: its ISA census (`make asm_srtp`) is read apart from the others', whose instruction streams stay what they were.
#include "aesgcm_keytab.h"
#include "aesgcm_lanes.h"
#include "aesgcm_wirecut.h"
#include "aesgcm_dispatch.h"

template <int NR, int DEC, int LG, u32 KIND>             // DEC: 0 encrypt, 1 decrypt; KIND: AESGCM_SRTP_RTP or AESGCM_SRTP_RTCP
__global__ __launch_bounds__(BATCH3_LANES(NR), (BATCH3_LANES(NR) + 255) / 256) void k_kt_srtp(const DevTables *__restrict__ tb, const KtWireXParams xp) {
    static_assert(KIND == AESGCM_SRTP_RTP || KIND == AESGCM_SRTP_RTCP, "SRTP or SRTCP");
    constexpr bool SLOTS = true, WIRE = true;
    constexpr u32 WIREX = KIND == AESGCM_SRTP_RTP ? KT_WIREX_SRTP : KT_WIREX_SRTCP;
    const KtWireXParams *const wx = &xp;
    const KtParams *const kt = &xp.w.k;
    const BatchParams &p = xp.w.k.b;
    const aesgcm_wire_fmt *const wf = &xp.w.f;
#include "aesgcm_batch3_body.inc"
}

// ------------------------------------------------------------------------------------------------ launchers
hipError_t klaunch_srtp_attributes() {
    return batch3v_each<AESGCM_SRTP_RTP, AESGCM_SRTP_RTCP>([](auto NR, auto D, auto LG, auto V) {
        return hipFuncSetAttribute(reinterpret_cast<const void *>(&k_kt_srtp<NR(), D(), LG(), V()>), hipFuncAttributeMaxDynamicSharedMemorySize, BATCH3_LDS_BYTES_LG(LG()));
    });
}

hipError_t klaunch_kt_srtp(unsigned kind, int nr, int dec, int lg, unsigned wgs, hipStream_t st, const DevTables *tb, const KtWireXParams &p) {
    if (kind != AESGCM_SRTP_RTP && kind != AESGCM_SRTP_RTCP) return hipErrorInvalidValue;
    batch3v_dispatch<AESGCM_SRTP_RTP, AESGCM_SRTP_RTCP>(nr, dec, lg, (int)kind, [&](auto NR, auto D, auto LG, auto V) {
        hipLaunchKernelGGL((k_kt_srtp<NR(), D(), LG(), V()>), dim3(wgs), dim3(BATCH3_LANES(NR())), BATCH3_LDS_BYTES_LG(LG()), st, tb, p);
    });
    return hipGetLastError();
}
