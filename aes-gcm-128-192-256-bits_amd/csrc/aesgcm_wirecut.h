// aesgcm_wirecut.h -- everything a wire format decides about a packet, one function per format and question: its CUT (what is refused, which bytes are AAD, which
// payload, the number that is not in the packet), its NONCE, the AAD block that is BUILT in registers where the AAD is not a run of packet bytes, and the TAG's place.
// The AEAD kernels of the key tables' wire families (aesgcm_<family>_kernels.hip) call them from aesgcm_batch3_body.inc through the four wire_* templates at the end,
// picked by the body's WIREX; the two mask kernels (QUIC header protection, DTLS 1.3 record-number encryption) call the same front tests through aesgcm_mask.h, and
// tests/wirecut_emul runs all of it on the host.  Everything is HD and names no kernel.
// Two rules hold for every cut.  The tests stand in the order in which a packet is refused, and nothing of a refused packet is read past the test that refuses it
// (`bad ? 0 : ...` in front of every load; slot 0 stands in for a refused packet's key material).  A cut takes the verdict so far in `bad` and ORs its own into it, and says
// its ranges in aoff, aad_len (the AAD's packet bytes, in p.aad) and doff, pkt_len (the payload, in p.in / p.out).  They are references to the caller's variables and not
// a struct that comes back: written so, the kernels keep the block loop of the text these functions were and, within one VGPR and a handful of instructions, its register and instruction counts
// (profiles/wirecut/isa_compare.txt: no listing is byte-identical); as a struct they did not.
#pragma once
#include "aesgcm_keytab.h"

// ---------------------------------------------------------------- the frame-side accesses, all inside the frame and at any byte address.  The ICV is 8, 12 or 16 bytes: dwords.
HD uint4 wire_load_icv(const unsigned char *p, u32 tag_len) {          // zero beyond tag_len
    return make_uint4(gload4_any(p), gload4_any(p + 4), tag_len > 8u ? gload4_any(p + 8) : 0u, tag_len > 12u ? gload4_any(p + 12) : 0u);
}
HD void wire_store_icv(unsigned char *p, uint4 v, u32 tag_len) {
    gstore4_any(p, v.x); gstore4_any(p + 4, v.y);
    if (tag_len > 8u) gstore4_any(p + 8, v.z);
    if (tag_len > 12u) gstore4_any(p + 12, v.w);
}
// out of place: the `front` bytes in front of the payload pass through, copied by the frame's G lanes (l = the lane's number) in 16-byte pieces; the last piece ends at
// `front` and may overlap the one before (the same bytes twice).  Fewer than 16 bytes: byte by byte.
HD void wire_copy_front(unsigned char *dst, const unsigned char *src, u32 front, u32 l, u32 G) {
    if (front >= 16u) for (u32 o = 16u * l; o < front; o += 16u * G) { const u32 q = o + 16u <= front ? o : front - 16u; gstore16_any(dst + q, gload16_any(src + q)); }
    else for (u32 o = l; o < front; o += G) dst[o] = src[o];
}

// ---------------------------------------------------------------- the front tests of the two-kernel formats (QUIC, DTLS 1.3)
// A call of either is an AEAD kernel and a mask kernel, and a packet must be refused by both or by neither: one kernel would otherwise write into a packet the other left
// alone.  So the tests that both make are these functions and nothing else.  wire_front: the ones that read no byte of the packet -- either slot out of range, falling
// offsets, more than 65535 bytes, a number field at byte 0, fewer than `tail` bytes from the number field's start to the packet's end, either slot unset.
// kt_slot: a packet's slot in the table, slot 0 standing in for one out of range (bad) -- the first test of every kernel that reads slots.  The mask kernels make it by this function
// (through mask_take); aesgcm_batch3_body.inc states the same three lines as text, for its instruction stream's sake (see there).  wire_front: `bad` and ks come in from kt_slot.  -> the mask key's slot (slot 0 likewise)
HD const KtSlot *kt_slot(const KtSlot *tab, u32 n_slots, u32 slot, bool &bad) {
    bad = slot >= n_slots;
    return tab + (bad ? 0u : slot);
}
HD const KtSlot *wire_front(const KtSlot *tab, u32 n_slots, const KtSlot *ks, u32 hslot, u32 po, u64 b, u64 e, u32 tail, bool &bad) {
    bad |= hslot >= n_slots || e < b || e - b > 65535u || po == 0u || (u64)po + tail > e - b;
    const KtSlot *const ms = tab + (bad ? 0u : hslot);
    bad |= ks->set != KT_SET || ms->set != KT_SET;
    return ms;
}
// QUIC (RFC 9000 17.1): a packet number is below 2^62.  On encrypt a larger one refuses the packet; on decrypt the number is the decoded one and needs no test
#define QUIC_TAIL 20u                      /* the sample's 16 bytes at pn_off + 4 lie inside the packet: header and tag then fit for every pn_len */
HD bool quic_pn_bad(u64 pn, int dec) { return dec == 0 && (pn >> 62) != 0; }
// DTLS 1.3's unified header (RFC 9147 4): first byte b0 = 0 0 1 C S L E E, never masked.  The header ends behind the sequence-number field at po (2 bytes with S, 0x08,
// else 1) and the 2 length bytes that L (0x04) announces.  -> its length; refused (bad): b0 is not 001xxxxx, or the sample's 16 bytes at the header's end do not lie
// inside the record's len bytes (so header and tag fit).  A record that is refused already has no header: 0
#define DTLS13_TAIL 17u                    /* one sequence byte and the sample behind pn_off, before the first byte is read */
HD u32 dtls13_hdr(u32 b0, u32 po, u64 len, bool &bad) {
    const u32 hdr = bad ? 0u : po + (b0 & 0x08u ? 2u : 1u) + (b0 & 0x04u ? 2u : 0u);
    bad |= (b0 & 0xE0u) != 0x20u || (u64)hdr + 16u > len;
    return hdr;
}

// ---------------------------------------------------------------- the cuts
// The plain wire family -- no extension, MACsec XPN, ESP ESN, TLS 1.3 / 1.2 records, DTLS 1.2 records: the frame is header | payload | ICV as `wf` lays it out.  AAD from
// the frame's first byte, payload behind the header, the ICV last; auth-only: everything in front of the ICV is AAD.  Refused: falling offsets, 2^28 bytes or more, too
// short for header (nonce bytes included) and ICV; a TLS record (hdr[5] | (1.2: explicit nonce[8]) | payload | tag[16]) of more than 5 + 65535 bytes -- its length field
// says what follows its five header bytes -- and a DTLS 1.2 record (RFC 6347: hdr[13] | explicit nonce[8] | payload | tag[16]) of more than 13 + 65535.  (The slot's
// `set` is the body's test, behind this one.)  ESN, TLS 1.2 and DTLS 1.2 build their one AAD block in registers (wire_aad_block): only its length is said here
template <u32 WIREX>
HD void cut_wire(const BatchParams &p, const aesgcm_wire_fmt *wf, u32 pkt, bool &bad, u64 &aoff, u64 &doff, u32 &aad_len, u32 &pkt_len, const unsigned char *&ivp) {
    constexpr bool x_esn = WIREX == AESGCM_WIREX_ESN, x_tls = WIREX == KT_WIREX_TLS13 || WIREX == KT_WIREX_TLS12, x_t12 = WIREX == KT_WIREX_TLS12, x_d12 = WIREX == KT_WIREX_DTLS12;
    const u64 b = p.data_off[pkt], e = p.data_off[pkt + 1];
    const bool auth_only = !x_esn && (wf->flags & AESGCM_WIRE_AUTH_ONLY) != 0;                   // (ESN: never -- aesgcm_wire_xfmt_check)
    const u32 nonce_end = wf->iv_off + 12u - wf->salt_len, front = auth_only && nonce_end > wf->hdr_len ? nonce_end : wf->hdr_len;
    bad |= e < b || e - b >= ((u64)1 << 28) || e - b < (u64)(front + wf->tag_len);
    if constexpr (x_tls) bad |= e - b > 5u + 65535u;
    if constexpr (x_d12) bad |= e - b > 13u + 65535u;
    const u32 body = bad ? 0u : (u32)(e - b) - wf->tag_len;                  // the bytes in front of the ICV
    aoff = b;
    aad_len = auth_only ? body : wf->aad_len;
    pkt_len = auth_only ? 0u : body - wf->hdr_len;
    doff = b + (auth_only ? body : wf->hdr_len);
    if constexpr (x_esn) aad_len = 12u;                                      // SPI | seq-hi | seq-lo (RFC 4303): the frame's first 8 bytes around hi[pkt]
    if constexpr (x_t12) aad_len = 13u;                                      // seq | type, version | payload length (RFC 5246 6.2.3.3): seq[pkt], three header bytes, pkt_len
    if constexpr (x_d12) aad_len = 13u;                                      // epoch, seq | type, version | payload length (RFC 6347 4.1.2.1): eleven header bytes, pkt_len
    ivp = p.in + b + wf->iv_off;                                             // where the nonce's frame bytes start
}

// A QUIC packet (RFC 9001 5.3): header | payload | tag[16].  AAD = the header up to and including the packet-number field, which starts at wx->pn_off[pkt] and whose
// length, (first byte & 3) + 1, is in the first byte -- read through p.aad, where the header lies unprotected; payload behind it; the tag last.  The header itself is
// the mask kernel's business.  Refused: wire_front (tail QUIC_TAIL) and quic_pn_bad.  A refused packet's number (-> num) and first byte are not read
HD void cut_quic(const BatchParams &p, const KtParams *kt, const KtWireXParams *wx, const KtSlot *ks, u32 pkt, int dec, bool &bad, u64 &aoff, u64 &doff, u32 &aad_len, u32 &pkt_len,
                 u64 &num) {
    const u64 b = p.data_off[pkt], e = p.data_off[pkt + 1];
    const u32 hslot = wx->hp_slots[pkt], po = wx->pn_off[pkt];
    wire_front(kt->tab, kt->n_slots, ks, hslot, po, b, e, QUIC_TAIL, bad);
    num = bad ? (u64)0 : wx->seq[pkt];
    bad |= quic_pn_bad(num, dec);
    const u32 hdr = bad ? 0u : po + (p.aad[b] & 3u) + 1u;
    aoff = b;
    aad_len = hdr;
    pkt_len = bad ? 0u : (u32)(e - b) - 16u - hdr;
    doff = b + hdr;
}

// A DTLS 1.3 record (RFC 9147 4): unified_hdr | payload | tag[16], QUIC's structure.  AAD = the unified header with the sequence-number bytes unprotected, read through
// p.aad; payload behind it; the tag last.  Refused: wire_front (tail DTLS13_TAIL; only then is the first byte read, through p.in: it is never masked, and the mask
// kernel writes nothing of a record it refuses), then dtls13_hdr.  A refused record's number (-> num) is not read
HD void cut_dtls13(const BatchParams &p, const KtParams *kt, const KtWireXParams *wx, const KtSlot *ks, u32 pkt, bool &bad, u64 &aoff, u64 &doff, u32 &aad_len, u32 &pkt_len, u64 &num) {
    const u64 b = p.data_off[pkt], e = p.data_off[pkt + 1];
    const u32 hslot = wx->hp_slots[pkt], po = wx->pn_off[pkt];
    wire_front(kt->tab, kt->n_slots, ks, hslot, po, b, e, DTLS13_TAIL, bad);
    const u32 b0 = bad ? 0u : p.in[b];
    const u32 hdr = dtls13_hdr(b0, po, e - b, bad);
    num = bad ? (u64)0 : wx->seq[pkt];
    aoff = b;
    aad_len = bad ? 0u : hdr;
    pkt_len = bad ? 0u : (u32)(e - b) - 16u - hdr;
    doff = b + (bad ? 0u : hdr);
}

// An SRTCP packet (RFC 7714 9; RFC 3711 3.4): rtcp_hdr[8] | payload | tag[16] | W[4] | mki, W = E | 31-bit index; `tail` = what follows the payload: the tag, W, the MKI's
// wx->mki_len bytes.  Refused, in this order: the slot, the offsets, more than 65535 bytes, too short for the fixed header and the tail (only then is the first byte read),
// a version other than 2.  E set: AAD = the 8 header bytes | W, payload behind the header.  E clear: nothing is encrypted, AAD = everything in front of the tag | W, and all
// of it passes through (doff = where the tag starts, as an auth-only frame's).  Either way the AAD is in two pieces, packet bytes and W (aad_srtcp).  E is per packet.
// (An SRTP packet's cut, its sibling, is text in aesgcm_batch3_body.inc: see there.)
HD void cut_srtcp(const BatchParams &p, const KtWireXParams *wx, const KtSlot *ks, u32 pkt, bool &bad, u64 &aoff, u64 &doff, u32 &aad_len, u32 &pkt_len) {
    const u64 b = p.data_off[pkt], e = p.data_off[pkt + 1];
    const u32 tail = 16u + wx->mki_len + 4u;
    bad |= ks->set != KT_SET;
    bad |= e < b || e - b > 65535u || e - b < (u64)(8u + tail);
    const u32 L = bad ? 0u : (u32)(e - b);
    const u32 b0 = bad ? 0x80u : p.in[b];
    bad |= (b0 & 0xC0u) != 0x80u;
    aoff = b;
    const u32 body = bad ? 0u : L - tail;                                // the bytes in front of the tag: 8 or more
    const bool enc = !bad && (p.in[b + body + 16u] & 0x80u) != 0;
    aad_len = bad ? 0u : enc ? 12u : body + 4u;
    pkt_len = enc ? body - 8u : 0u;
    doff = b + (enc ? 8u : body);
}

// An SSH binary packet under AES-GCM (RFC 5647 7.2 / 7.3; OpenSSH PROTOCOL 1.6): packet_length[4] | body | tag[16].  AAD = the four length bytes, which stay in the
// clear; payload = the body (padding_length, payload, padding: not interpreted), a whole number of cipher blocks and at least one; the tag last.  Refused, in this
// order: the slot, falling offsets, 2^28 bytes or more, fewer than 4 + 16 + 16, a body that is no multiple of 16, the slot unset -- and only then is the length field
// read, in both directions (on encrypt the caller wrote it): it must say the body's length.  A refused packet's number is not read (wire_nonce)
HD void cut_ssh(const BatchParams &p, const KtSlot *ks, u32 pkt, bool &bad, u64 &aoff, u64 &doff, u32 &aad_len, u32 &pkt_len) {
    const u64 b = p.data_off[pkt], e = p.data_off[pkt + 1];
    bad |= e < b || e - b >= ((u64)1 << 28) || e - b < 36u || ((e - b - 20u) & 15u) != 0;
    bad |= ks->set != KT_SET;
    const u32 body = bad ? 0u : (u32)(e - b) - 20u;
    const u32 field = bad ? 0u : bswap32(gload4_any(p.in + b));
    bad |= field != body;
    aoff = b;
    aad_len = bad ? 0u : 4u;
    pkt_len = bad ? 0u : body;
    doff = b + (bad ? 0u : 4u);
}

// ---------------------------------------------------------------- the nonces, as three memory-order words.  `bad`: a refused packet's bytes and numbers are not read
// salt_len (0, 4 or 8) bytes of the slot's salt, then the frame's bytes at ivp -- whole words either way (the formats without an extension, and ESP with ESN)
HD void nonce_salted(const KtSlot *ks, const unsigned char *ivp, u32 sw, bool bad, u32 &iv0, u32 &iv1, u32 &iv2) {
    const u32 f0 = bad ? 0u : gload4_any(ivp), f1 = bad || sw > 1u ? 0u : gload4_any(ivp + 4), f2 = bad || sw > 0u ? 0u : gload4_any(ivp + 8);
    iv0 = sw ? ks->salt[0] : f0;
    iv1 = sw > 1u ? ks->salt[1] : sw ? f0 : f1;
    iv2 = sw > 1u ? f0 : sw ? f1 : f2;
}
// MACsec XPN (802.1AEbw): the slot's 12-byte salt XOR (SSCI | PN), big-endian: hi, then the four frame bytes at ivp (salt_len is 8 -- aesgcm_wire_xfmt_check).  The classic
// salt is not used
HD void nonce_xpn(const KtSlot *ks, const unsigned char *ivp, const u32 *hi, bool bad, u32 &iv0, u32 &iv1, u32 &iv2) {
    const u32 f0 = bad ? 0u : gload4_any(ivp);
    iv0 = ks->xpn[0] ^ ks->xpn[3]; iv1 = ks->xpn[1] ^ (bad ? 0u : bswap32(*hi)); iv2 = ks->xpn[2] ^ f0;
}
// TLS 1.2 (RFC 5288), and DTLS 1.2 the same: the slot IV's first four bytes (aesgcm_keytab_set_tls_iv), then the record's explicit eight at ivp
HD void nonce_tls12(const KtSlot *ks, const unsigned char *ivp, bool bad, u32 &iv0, u32 &iv1, u32 &iv2) {
    iv0 = ks->xpn[0]; iv1 = bad ? 0u : gload4_any(ivp); iv2 = bad ? 0u : gload4_any(ivp + 4);
}
// TLS 1.3 (RFC 8446 5.3): the slot's 12-byte IV XOR the sequence number, big-endian, right-aligned; no nonce byte is read from the record.  QUIC (RFC 9001 5.3): the same
// with the packet number; DTLS 1.3 (RFC 9147 4.2.1 -> RFC 8446 5.3): with the record's sequence number
HD void nonce_iv_xor_num(const KtSlot *ks, u64 num, u32 &iv0, u32 &iv1, u32 &iv2) {
    iv0 = ks->xpn[0]; iv1 = ks->xpn[1] ^ bswap32((u32)(num >> 32)); iv2 = ks->xpn[2] ^ bswap32((u32)num);
}
// SSH (RFC 5647 7.1): the slot's 12-byte IV = fixed[4] | invocation_counter[8], the counter a big-endian integer that is INCREMENTED once per packet: the nonce is
// fixed | be64(counter + num mod 2^64), num = the packets sent under the key before this one.  The carry runs through the counter's 64 bits and never into the fixed field
HD void nonce_iv_add_num(const KtSlot *ks, u64 num, u32 &iv0, u32 &iv1, u32 &iv2) {
    const u64 c = (((u64)bswap32(ks->xpn[1]) << 32) | bswap32(ks->xpn[2])) + num;
    iv0 = ks->xpn[0]; iv1 = bswap32((u32)(c >> 32)); iv2 = bswap32((u32)c);
}
// SRTCP (RFC 7714 9.1): the salt XOR (00 00 | SSRC | 00 00 | 0, the 31-bit index) -- SSRC = the packet's bytes 4 .. 7, the index = W without its E bit (the top bit of
// W's first byte); w_at = where W lies: 16 bytes behind the payload, or behind the AAD's packet bytes when there is none
HD void nonce_srtcp(const KtSlot *ks, const unsigned char *pk, const unsigned char *w_at, bool bad, u32 &iv0, u32 &iv1, u32 &iv2) {
    const u32 ssrc = bad ? 0u : gload4_any(pk + 4), w = bad ? 0u : gload4_any(w_at) & 0xFFFFFF7Fu;
    iv0 = ks->xpn[0] ^ (ssrc << 16); iv1 = ks->xpn[1] ^ (ssrc >> 16); iv2 = ks->xpn[2] ^ w;
}

// ---------------------------------------------------------------- the AAD blocks that are built in registers
// ESP with extended sequence numbers (RFC 4303): SPI | seq-hi | seq-lo, the frame's first 8 bytes around the number that is not in the frame
HD uint4 aad_esn(const unsigned char *aad, u32 hi) { return make_uint4(gload4_any(aad), bswap32(hi), gload4_any(aad + 4), 0u); }
// TLS 1.2 (RFC 5246 6.2.3.3): be64(seq) | type, version (the record's first three bytes) | be16(payload length), the length from the offsets (pkt_len < 2^16: the cut's
// test), not from the header's own two bytes
HD uint4 aad_tls12(const unsigned char *aad, u64 sq, u32 pkt_len) {
    return make_uint4(bswap32((u32)(sq >> 32)), bswap32((u32)sq), (gload4_any(aad) & 0x00FFFFFFu) | ((pkt_len >> 8) << 24), pkt_len & 0xFFu);
}
// DTLS 1.2 (RFC 6347 4.1.2.1): epoch | sequence number as the record's bytes 3 .. 10 carry them, then as TLS 1.2's
HD uint4 aad_dtls12(const unsigned char *aad, u32 pkt_len) {
    return make_uint4(gload4_any(aad + 3), gload4_any(aad + 7), (gload4_any(aad) & 0x00FFFFFFu) | ((pkt_len >> 8) << 24), pkt_len & 0xFFu);
}
// SRTCP's AAD is in two pieces: packet bytes, then W from behind the tag (w_at), fetched by the lane that needs it; `off` = the block's offset in the AAD.  12 bytes (E
// set; E clear and a bare header): the one block header | W.  Longer (E clear): aad_len - 4 packet bytes; a block that lies inside them is a plain load, the others take
// what is left of the packet bytes and as much of W as fits -- W may split over the last two blocks
HD uint4 aad_srtcp(const unsigned char *aad, const unsigned char *w_at, u32 aad_len, u32 off) {
    const u32 body = aad_len - 4u;
    if (aad_len == 12u) return make_uint4(gload4_any(aad), gload4_any(aad + 4), gload4_any(w_at), 0u);
    if (off + 16u <= body) return gload16_any(aad + off);
    return load_block_split(aad + off, off < body ? body - off : 0u, w_at, off > body ? off - body : 0u);
}

// ---------------------------------------------------------------- what aesgcm_batch3_body.inc calls, one each for cut, nonce, built AAD block and tag place
template <u32 WIREX>
HD void wire_cut(const BatchParams &p, const KtParams *kt, const aesgcm_wire_fmt *wf, const KtWireXParams *wx, const KtSlot *ks, u32 pkt, int dec, bool &bad, u64 &aoff, u64 &doff,
                 u32 &aad_len, u32 &pkt_len, u64 &num, const unsigned char *&ivp) {
    static_assert(WIREX != KT_WIREX_SRTP, "SRTP's cut is text in the body");
    if constexpr (WIREX == KT_WIREX_QUIC) cut_quic(p, kt, wx, ks, pkt, dec, bad, aoff, doff, aad_len, pkt_len, num);
    else if constexpr (WIREX == KT_WIREX_DTLS13) cut_dtls13(p, kt, wx, ks, pkt, bad, aoff, doff, aad_len, pkt_len, num);
    else if constexpr (WIREX == KT_WIREX_SRTCP) cut_srtcp(p, wx, ks, pkt, bad, aoff, doff, aad_len, pkt_len);
    else if constexpr (WIREX == KT_WIREX_SSH) cut_ssh(p, ks, pkt, bad, aoff, doff, aad_len, pkt_len);
    else cut_wire<WIREX>(p, wf, pkt, bad, aoff, doff, aad_len, pkt_len, ivp);
}

// ivp: cut_wire's; pk, in: the packet's first byte and its payload's; pkt_len, num: the cut's; bad: the cut's verdict and the body's own (the slot's `set`)
template <u32 WIREX>
HD void wire_nonce(const aesgcm_wire_fmt *wf, const KtWireXParams *wx, const KtSlot *ks, const unsigned char *ivp, const unsigned char *pk, const unsigned char *in, u32 pkt_len,
                   u64 num, u32 pkt, bool bad, u32 &iv0, u32 &iv1, u32 &iv2) {
    if constexpr (WIREX == AESGCM_WIREX_XPN) nonce_xpn(ks, ivp, wx->hi + pkt, bad, iv0, iv1, iv2);
    else if constexpr (WIREX == KT_WIREX_TLS12 || WIREX == KT_WIREX_DTLS12) nonce_tls12(ks, ivp, bad, iv0, iv1, iv2);
    else if constexpr (WIREX == KT_WIREX_TLS13) nonce_iv_xor_num(ks, bad ? (u64)0 : wx->seq[pkt], iv0, iv1, iv2);         // (a refused record's number is not read)
    else if constexpr (WIREX == KT_WIREX_QUIC || WIREX == KT_WIREX_DTLS13) nonce_iv_xor_num(ks, num, iv0, iv1, iv2);
    else if constexpr (WIREX == KT_WIREX_SSH) nonce_iv_add_num(ks, bad ? (u64)0 : wx->seq[pkt], iv0, iv1, iv2);           // (likewise)
    else if constexpr (WIREX == KT_WIREX_SRTCP) nonce_srtcp(ks, pk, in + pkt_len + 16u, bad, iv0, iv1, iv2);
    else nonce_salted(ks, ivp, wf->salt_len >> 2, bad, iv0, iv1, iv2);
}
// out of place the AEAD copies the bytes in front of the payload (header; auth-only: all but the ICV) -- but for QUIC and DTLS 1.3, whose mask kernel writes the header
HD constexpr bool wire_copies_front(u32 wirex) { return wirex != KT_WIREX_QUIC && wirex != KT_WIREX_DTLS13; }

// the formats whose AAD is built, and those among them whose block takes a number from outside the frame (`num`: ESN's hi, TLS 1.2's seq)
HD constexpr bool wire_aad_built(u32 wirex) { return wirex == AESGCM_WIREX_ESN || wirex == KT_WIREX_TLS12 || wirex == KT_WIREX_DTLS12 || wirex == KT_WIREX_SRTCP; }
HD constexpr bool wire_aad_num(u32 wirex) { return wirex == AESGCM_WIREX_ESN || wirex == KT_WIREX_TLS12; }
// aad, in: the AAD's packet bytes and the payload; off: the block's offset in the AAD; xpkt: the packet, for the formats of wire_aad_num
template <u32 WIREX>
HD uint4 wire_aad_block(const KtWireXParams *wx, const unsigned char *aad, const unsigned char *in, u32 aad_len, u32 pkt_len, u32 off, u32 xpkt) {
    static_assert(wire_aad_built(WIREX), "the other formats' AAD is a run of packet bytes");
    if constexpr (WIREX == AESGCM_WIREX_ESN) return aad_esn(aad, wx->hi[xpkt]);
    else if constexpr (WIREX == KT_WIREX_TLS12) return aad_tls12(aad, wx->seq[xpkt], pkt_len);
    else if constexpr (WIREX == KT_WIREX_DTLS12) return aad_dtls12(aad, pkt_len);
    else return aad_srtcp(aad, in + pkt_len + 16u, aad_len, off);
}

// Where the ICV starts: the tag's first tag_len bytes are the frame's last, or (SRTP, SRTCP) stand in front of the trail -- SRTCP's W and the MKI, which pass through out
// of place, copied by the one lane that calls this
template <u32 WIREX>
HD u64 wire_tag_place(const BatchParams &p, const aesgcm_wire_fmt *wf, const KtWireXParams *wx, u32 pkt) {
    const u32 tl = wf->tag_len;
    u64 at = p.data_off[pkt + 1] - tl;
    if constexpr (WIREX == KT_WIREX_SRTP || WIREX == KT_WIREX_SRTCP) {
        const u32 trail = wx->mki_len + (WIREX == KT_WIREX_SRTCP ? 4u : 0u);
        at -= trail;
        if (p.in != p.out) wire_copy_front(p.out + at + tl, p.in + at + tl, trail, 0u, 1u);
    }
    return at;
}
