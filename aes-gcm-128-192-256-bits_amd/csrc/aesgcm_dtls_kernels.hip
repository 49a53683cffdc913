// aesgcm_dtls_kernels.hip -- key tables on DTLS records in wire format (gfx950; DTLS 1.3: RFC 9147 section 4, DTLS 1.2 AES-GCM: RFC 6347 with RFC 5288):
// aesgcm_keytab_dtls_crypt_dev's two kernels and their launchers; the host side is aesgcm_keytab.hip.
//
//   k_kt_dtls<NR,DEC,LG,VER>  the AEAD (aesgcm_batch3_body.inc, SLOTS = WIRE = true, WIREX = KT_WIREX_DTLS13 / KT_WIREX_DTLS12).  VER says which record:
//                               AESGCM_DTLS_13  record = unified_hdr | payload | tag[16]: k_kt_quic's path with another header rule.  The header ends behind the
//                                               sequence-number field at pn_off[p] (1 or 2 bytes: the first byte's S bit, 0x08) and the 2 length bytes that its L bit (0x04)
//                                               announces; the first byte is never masked and is read through p.in, the AAD = the whole header through p.aad, where its
//                                               sequence bytes lie UNPROTECTED (encrypt: d_in; decrypt: d_out, where k_kt_dtls_sn left it).  Nonce = the slot's 12-byte IV
//                                               (KtSlot::xpn) XOR seq[p], the full record sequence number (decrypt: as k_kt_dtls_sn decoded it).  It copies no header.
//                               AESGCM_DTLS_12  record = hdr[13] | explicit nonce[8] | payload | tag[16]: k_kt_tls's TLS 1.2 path (format {13, 21, 13, 4, 16, 0}) with the AAD
//                                               block's first eight bytes, epoch | sequence number, loaded from the record's bytes 3 .. 10 where TLS 1.2 takes seq[p].  One
//                                               launch, no number from outside the record; header and explicit nonce pass through.
//   k_kt_dtls_sn<NR,DEC>      DTLS 1.3's record-number encryption (RFC 9147 4.2.3), a lane per record: mask = AES-ECB of the 16 ciphertext bytes behind the header under the
//                             round keys of the record's sn slot; the 1 or 2 sequence bytes are XORed with mask[0], mask[1].  Decrypt: it also decodes the full number from
//                             the truncated one and the expected one (wire_decode_num, aesgcm_mask.h) into pn_out[p].  Out of place it writes the whole header.  The
//                             refusals that read no byte, the mask and the decode are k_kt_quic_hp's, shared through aesgcm_mask.h.
// Encrypt runs k_kt_dtls, then k_kt_dtls_sn (the sample is fresh ciphertext); decrypt the other way round.  Both refuse the same records by the same functions
// (aesgcm_wirecut.h: wire_front, dtls13_hdr), so a refused record is touched by neither; k_kt_dtls alone reports it (status word, auth 0).  36 + 6 instances; the loop for fixed-size records
// (BatchParams::plain) is not compiled in; every k_kt_dtls one: no scratch, at most 128 registers.
// A translation unit of its own: its ISA census (`make asm_dtls`) is read apart from the others', whose instruction streams stay what they were.
#include "aesgcm_keytab.h"
#include "aesgcm_lanes.h"
#include "aesgcm_wirecut.h"
#include "aesgcm_mask.h"
#include "aesgcm_dispatch.h"

template <int NR, int DEC, int LG, u32 VER>              // DEC: 0 encrypt, 1 decrypt; VER: AESGCM_DTLS_13 or AESGCM_DTLS_12
__global__ __launch_bounds__(BATCH3_LANES(NR), (BATCH3_LANES(NR) + 255) / 256) void k_kt_dtls(const DevTables *__restrict__ tb, const KtWireXParams xp) {
    static_assert(VER == AESGCM_DTLS_13 || VER == AESGCM_DTLS_12, "DTLS 1.3 or DTLS 1.2");
    constexpr bool SLOTS = true, WIRE = true;
    constexpr u32 WIREX = VER == AESGCM_DTLS_13 ? KT_WIREX_DTLS13 : KT_WIREX_DTLS12;
    const KtWireXParams *const wx = &xp;
    const KtParams *const kt = &xp.w.k;
    const BatchParams &p = xp.w.k.b;
    const aesgcm_wire_fmt *const wf = &xp.w.f;
#include "aesgcm_batch3_body.inc"
}

template <int NR, int DEC>
__global__ __launch_bounds__(256) void k_kt_dtls_sn(const DevTables *__restrict__ tb, const KtQuicHpParams q) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const u32 tid = threadIdx.x;
    main_fill_lds(smem, nullptr, tb, tid, false, 256u);          // T0 | T2
    __syncthreads();
    const u32 i = blockIdx.x * 256u + tid;
    if (i >= q.n_pkts) return;
    // the refusals are k_kt_dtls's, by the functions its cut calls (aesgcm_wirecut.h: cut_dtls13): a refused record's number is not read and nothing of it is written
    MaskPkt m;
    if (!mask_take(q, i, DTLS13_TAIL, m)) return;
    const unsigned char *const src = m.src;
    unsigned char *const dst = m.dst;
    const u32 po = m.po;
    const u32 b0 = src[0];                                       // 0 0 1 C S L E E: never masked, so the same byte before and behind either pass
    bool bad = false;
    const u32 hdr = dtls13_hdr(b0, po, m.len, bad), sn_len = b0 & 0x08u ? 2u : 1u;
    if (bad) return;
    // mask = AES-ECB(sn key, sample): the first 16 ciphertext bytes -- encrypt: what k_kt_dtls has just written to `out`; decrypt: the protected record's
    u32 s0, s1, s2, s3;
    mask_of_sample<NR>(m.ms, (DEC ? src : (const unsigned char *)dst) + hdr, smem, (tid & 31u) << 2, s0, s1, s2, s3);
    if (q.in != q.out) {                                         // out of place: the whole header, by this one lane; the sequence bytes below
        wire_copy_front(dst, src, po, 0u, 1u);
        for (u32 k = po + sn_len; k < hdr; k++) dst[k] = src[k];
    }
    u32 trunc = 0;
    for (u32 k = 0; k < sn_len; k++) {
        const u32 x = src[po + k] ^ ((s0 >> (8u * k)) & 0xFFu);  // mask[0], mask[1]
        dst[po + k] = (unsigned char)x;
        trunc = (trunc << 8) | x;
    }
    if (DEC) q.pn_out[i] = wire_decode_num(q.pn[i], trunc, 8u * sn_len, ~(u64)0);
}

// ------------------------------------------------------------------------------------------------ launchers
#define KT_DTLS_SN_LDS (AESGCM_LDS_AES_OFF + AESGCM_LDS_AES)
hipError_t klaunch_dtls_attributes() {
    const hipError_t e = batch3v_each<AESGCM_DTLS_13, AESGCM_DTLS_12>([](auto NR, auto D, auto LG, auto V) {
        return hipFuncSetAttribute(reinterpret_cast<const void *>(&k_kt_dtls<NR(), D(), LG(), V()>), hipFuncAttributeMaxDynamicSharedMemorySize, BATCH3_LDS_BYTES_LG(LG()));
    });
    return e != hipSuccess ? e : mask_each([](auto NR, auto D) { return hipFuncSetAttribute(reinterpret_cast<const void *>(&k_kt_dtls_sn<NR(), D()>), hipFuncAttributeMaxDynamicSharedMemorySize, KT_DTLS_SN_LDS); });
}

hipError_t klaunch_kt_dtls(unsigned version, int nr, int dec, int lg, unsigned wgs, hipStream_t st, const DevTables *tb, const KtWireXParams &p) {
    if (version != AESGCM_DTLS_13 && version != AESGCM_DTLS_12) return hipErrorInvalidValue;
    batch3v_dispatch<AESGCM_DTLS_13, AESGCM_DTLS_12>(nr, dec, lg, (int)version, [&](auto NR, auto D, auto LG, auto V) {
        hipLaunchKernelGGL((k_kt_dtls<NR(), D(), LG(), V()>), dim3(wgs), dim3(BATCH3_LANES(NR())), BATCH3_LDS_BYTES_LG(LG()), st, tb, p);
    });
    return hipGetLastError();
}

hipError_t klaunch_kt_dtls_sn(int nr, int dec, hipStream_t st, const DevTables *tb, const KtQuicHpParams &p) {
    const unsigned wgs = (p.n_pkts + 255u) / 256u;
    mask_dispatch(nr, dec, [&](auto NR, auto D) { hipLaunchKernelGGL((k_kt_dtls_sn<NR(), D()>), dim3(wgs), dim3(256), KT_DTLS_SN_LDS, st, tb, p); });
    return hipGetLastError();
}
