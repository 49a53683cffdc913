// aesgcm_kdf_slot.h -- a key-table slot built from a key that lies in a lane's REGISTERS: what the two derivation families share (aesgcm_kdf_kernels.hip: HKDF output;
// aesgcm_srtp_kdf_kernels.hip: AES-CM PRF output, and the master key's own schedule).  No derived key passes through memory on its way into its slot.
#pragma once
#include "aesgcm_keytab.h"
#include "aesgcm_dispatch.h"

// FIPS-197 KeyExpansion on memory-order words, in place: rk[0 .. NR - 7] = the key -> rk[0 .. 4 * NR + 3].  The S-box is byte 1 of the LDS T0 entry (smem holds
// T0 | T2, main_fill_lds; lb = (lane & 31) << 2).  HD: the CPU harness tests/srtp_kdf_emul runs it over an LDS image in host memory.
template <int NR>
HD void kdf_key_schedule(u32 *rk, const unsigned char *smem, u32 lb) {
    constexpr int NK = NR - 6;
    u32 rcon = 1;
#pragma unroll
    for (int w = NK; w < 4 * (NR + 1); w++) {
        u32 t = rk[w - 1];
        if (w % NK == 0) {
            t = (t >> 8) | (t << 24);                                            // RotWord on a little-endian word
            t = ((T0_AT(smem, t, 0, lb) >> 8) & 0xFFu) | (T0_AT(smem, t, 1, lb) & 0xFF00u) |
                (T0_AT(smem, t, 2, lb) & 0xFF0000u) | ((T0_AT(smem, t, 3, lb) << 8) & 0xFF000000u);   // SubWord
            t ^= rcon;
            rcon = xtime2(rcon);
        } else if (NK == 8 && (w % NK) == 4) {
            t = ((T0_AT(smem, t, 0, lb) >> 8) & 0xFFu) | (T0_AT(smem, t, 1, lb) & 0xFF00u) |
                (T0_AT(smem, t, 2, lb) & 0xFF0000u) | ((T0_AT(smem, t, 3, lb) << 8) & 0xFF000000u);
        }
        rk[w] = rk[w - NK] ^ t;
    }
}

// A COPY of k_kt_setup's steps (aesgcm_keytab_kernels.hip) that takes the key from registers: rk[0 .. NR - 7] = the key's memory-order words.  batch_key_expand
// (aesgcm_batch.h) reads its key from memory, and lifting its schedule out for both callers moved the instruction streams of aesgcm_kernels.hip and of the keytab
// family (operand orders; profiles/kdf/isa_unchanged.txt), so those sources stay as they are and the steps are repeated here: the schedule above, H = E_K(0^128),
// H^(2^j) for j = 0 .. 6, nr, then the `set` marker; salt and xpn are left alone.
// tests/test_gpu_kdf.py and tests/test_gpu_srtp_kdf.py hold every installed slot to what aesgcm_keytab_set makes of the same key, through the packets it encrypts.
template <int NR>
__device__ __forceinline__ void kdf_slot_build(KtSlot *d, u32 *rk, const unsigned char *smem, u32 lb) {
    kdf_key_schedule<NR>(rk, smem, lb);
    u32 s0 = rk[0], s1 = rk[1], s2 = rk[2], s3 = rk[3];
    aes_rounds_lds<NR>(s0, s1, s2, s3, rk, smem, lb);            // H = E_K(0^128)
    G128 h = mo_to_be(make_uint4(s0, s1, s2, s3));
#pragma unroll
    for (int q = 0; q < NR + 1; q++) *reinterpret_cast<uint4 *>(d->rk + 4 * q) = make_uint4(rk[4 * q], rk[4 * q + 1], rk[4 * q + 2], rk[4 * q + 3]);
#pragma unroll
    for (int j = 0; j < KT_HPOW; j++) {
        d->hpow[j] = make_uint4(h.w[0], h.w[1], h.w[2], h.w[3]);
        h = gf_sqr(h);
    }
    d->nr = NR;
    __threadfence();
    d->set = KT_SET;
}
