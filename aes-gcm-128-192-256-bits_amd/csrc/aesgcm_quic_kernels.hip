// aesgcm_quic_kernels.hip -- key tables on QUIC packets in wire format (gfx950, RFC 9001 section 5): aesgcm_keytab_quic_crypt_dev's two kernels and their launchers; the
// host side is aesgcm_keytab.hip.
//
//   k_kt_quic<NR,DEC,LG>    the AEAD: k_kt_tls's TLS 1.3 path (aesgcm_batch3_body.inc, SLOTS = WIRE = true, WIREX = KT_WIREX_QUIC) with a header whose length differs from
//                           packet to packet: AAD = bytes [0, pn_off[p] + pn_len), pn_len = (first byte & 3) + 1, the first byte read through p.aad where the header lies
//                           UNPROTECTED (encrypt: d_in; decrypt: d_out, where k_kt_quic_hp left it).  Nonce = the slot's 12-byte IV (KtSlot::xpn) XOR seq[p], the full packet
//                           number (decrypt: as k_kt_quic_hp decoded it into d_pn_out).  It copies no header: that is the other kernel's.
//   k_kt_quic_hp<NR,DEC>    header protection (RFC 9001 5.4), a lane per packet: mask = AES-ECB of the 16 ciphertext bytes at pn_off + 4 under the round keys of the packet's
//                           hp slot; the first byte's low bits and the pn_len packet-number bytes are XORed with it, byte by byte, inside the packet.  Decrypt: it also
//                           decodes the full number from the truncated one and the expected one (RFC 9000 A.3) into pn_out[p].  Out of place it writes the whole header.
// Encrypt runs k_kt_quic, then k_kt_quic_hp (the sample is fresh ciphertext); decrypt the other way round (the AEAD needs the unmasked header and the number).  Both refuse
// the same packets by the same functions (aesgcm_wirecut.h: wire_front, quic_pn_bad), so a refused packet is touched by neither; k_kt_quic alone reports it (status word,
// auth 0).  18 + 6 instances; every k_kt_quic one: no scratch, at most 128 registers.
// A translation unit of its own: its ISA census (`make asm_quic`) is read apart from the others', whose instruction streams stay what they were.
#include "aesgcm_keytab.h"
#include "aesgcm_lanes.h"
#include "aesgcm_wirecut.h"
#include "aesgcm_mask.h"
#include "aesgcm_dispatch.h"

template <int NR, int DEC, int LG>                       // DEC: 0 encrypt, 1 decrypt
__global__ __launch_bounds__(BATCH3_LANES(NR), (BATCH3_LANES(NR) + 255) / 256) void k_kt_quic(const DevTables *__restrict__ tb, const KtWireXParams xp) {
    constexpr bool SLOTS = true, WIRE = true;
    constexpr u32 WIREX = KT_WIREX_QUIC;
    const KtWireXParams *const wx = &xp;
    const KtParams *const kt = &xp.w.k;
    const BatchParams &p = xp.w.k.b;
    const aesgcm_wire_fmt *const wf = &xp.w.f;
#include "aesgcm_batch3_body.inc"
}

// RFC 9000 A.3 (DecodePacketNumber): the shared decode (aesgcm_mask.h) with QUIC's number space, whose last number is 2^62 - 1
HD u64 quic_decode_pn(u64 expected, u32 truncated, u32 pn_nbits) { return wire_decode_num(expected, truncated, pn_nbits, ((u64)1 << 62) - 1u); }

template <int NR, int DEC>
__global__ __launch_bounds__(256) void k_kt_quic_hp(const DevTables *__restrict__ tb, const KtQuicHpParams q) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const u32 tid = threadIdx.x;
    main_fill_lds(smem, nullptr, tb, tid, false, 256u);          // T0 | T2
    __syncthreads();
    const u32 i = blockIdx.x * 256u + tid;
    if (i >= q.n_pkts) return;
    // the refusals are k_kt_quic's, by the functions its cut calls (aesgcm_wirecut.h: cut_quic): a refused packet's number is not read and nothing of it is written
    MaskPkt m;
    if (!mask_take(q, i, QUIC_TAIL, m)) return;
    const u64 pn = q.pn[i];
    if (quic_pn_bad(pn, DEC)) return;
    const unsigned char *const src = m.src;
    unsigned char *const dst = m.dst;
    const u32 po = m.po;
    // mask = AES-ECB(hp key, sample): the sample is ciphertext -- encrypt: what k_kt_quic has just written to `out`; decrypt: the protected packet's
    u32 s0, s1, s2, s3;
    mask_of_sample<NR>(m.ms, (DEC ? src : (const unsigned char *)dst) + po + 4u, smem, (tid & 31u) << 2, s0, s1, s2, s3);
    const u32 f_in = src[0];
    const u32 first = f_in ^ (s0 & (f_in & 0x80u ? 0x0Fu : 0x1Fu));      // (the form bit itself is never masked)
    const u32 pn_len = ((DEC ? first : f_in) & 3u) + 1u;
    if (q.in != q.out) wire_copy_front(dst, src, po, 0u, 1u);    // out of place: the header in front of the packet number, by this one lane
    dst[0] = (unsigned char)first;
    const u32 mk = (s0 >> 8) | (s1 << 24);                        // mask[1 .. 4]
    u32 trunc = 0;
    for (u32 k = 0; k < pn_len; k++) {
        const u32 x = src[po + k] ^ ((mk >> (8u * k)) & 0xFFu);
        dst[po + k] = (unsigned char)x;
        trunc = (trunc << 8) | x;
    }
    if (DEC) q.pn_out[i] = quic_decode_pn(pn, trunc, 8u * pn_len);
}

// ------------------------------------------------------------------------------------------------ launchers
#define KT_QUIC_HP_LDS (AESGCM_LDS_AES_OFF + AESGCM_LDS_AES)
hipError_t klaunch_quic_attributes() {
    const hipError_t e = batch3_each([](auto NR, auto D, auto LG) { return hipFuncSetAttribute(reinterpret_cast<const void *>(&k_kt_quic<NR(), D(), LG()>), hipFuncAttributeMaxDynamicSharedMemorySize, BATCH3_LDS_BYTES_LG(LG())); });
    return e != hipSuccess ? e : mask_each([](auto NR, auto D) { return hipFuncSetAttribute(reinterpret_cast<const void *>(&k_kt_quic_hp<NR(), D()>), hipFuncAttributeMaxDynamicSharedMemorySize, KT_QUIC_HP_LDS); });
}

hipError_t klaunch_kt_quic(int nr, int dec, int lg, unsigned wgs, hipStream_t st, const DevTables *tb, const KtWireXParams &p) {
    batch3_dispatch(nr, dec, lg, [&](auto NR, auto D, auto LG) { hipLaunchKernelGGL((k_kt_quic<NR(), D(), LG()>), dim3(wgs), dim3(BATCH3_LANES(NR())), BATCH3_LDS_BYTES_LG(LG()), st, tb, p); });
    return hipGetLastError();
}

hipError_t klaunch_kt_quic_hp(int nr, int dec, hipStream_t st, const DevTables *tb, const KtQuicHpParams &p) {
    const unsigned wgs = (p.n_pkts + 255u) / 256u;
    mask_dispatch(nr, dec, [&](auto NR, auto D) { hipLaunchKernelGGL((k_kt_quic_hp<NR(), D()>), dim3(wgs), dim3(256), KT_QUIC_HP_LDS, st, tb, p); });
    return hipGetLastError();
}
