// CPU harness for csrc/aesgcm_wirecut.h (__host__ __device__): it runs the SAME cut functions the key tables' wire kernels run, one packet at a time, and holds them to
// the plain restatement of each format's rules below (the RFCs' sentences, written without the kernels' "bad ? 0 : ..." form).  Every packet lies alone in a heap block
// of exactly its size and every per-packet array has exactly one entry, so that under the address sanitizer (asan.mk) a byte read past a packet -- or anything read of
// a packet past the test that refuses it, where that would leave the block -- is an error.  For QUIC and DTLS 1.3 it also runs the mask kernels' side (mask_take of
// aesgcm_mask.h, quic_pn_bad, dtls13_hdr) on the same packet and asserts the same verdict: they are the same functions today, and this guards against a later divergence.
// SRTP's cut is not here: it stayed text in aesgcm_batch3_body.inc (see there), so only the GPU tests reach it (tests/test_gpu_srtp.py); SRTCP's is.
// It takes no input and prints "WIRECUT OK <packets>"; a failed expectation prints the case and exits 1.  Test infrastructure only.
#include "../../aes-gcm-128-192-256-bits_amd/csrc/aesgcm_mask.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

static u64 g_rng = 0x77697265;
static u64 rnd() { u64 z = (g_rng += 0x9E3779B97F4A7C15ull); z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
static u32 rnd_below(u32 n) { return (u32)(rnd() % n); }

#define N_SLOTS 4u                          /* slot 3 is unset */
static KtSlot *g_tab;
static size_t g_packets;

struct Pkt {                                // one packet and what the call says about it
    std::vector<unsigned char> bytes;       // the arena: exactly the packet (falling offsets: `b` bytes)
    u64 b = 0, e = 0;
    u32 slot = 0, hslot = 1, po = 0, hi = 0, mki_len = 0;
    u64 seq = 0;
    int dec = 0;
};
struct Cut { bool bad; u64 aoff, doff, num; u32 aad_len, pkt_len; };

static void fail(const char *what, const Pkt &k, const Cut &got, const Cut &want) {
    printf("FAILED %s: b %llu e %llu slot %u hslot %u po %u dec %d first byte %02x\n  got  bad %d aoff %llu doff %llu aad_len %u pkt_len %u num %llu\n  want bad %d aoff %llu doff %llu aad_len %u pkt_len %u num %llu\n",
           what, (unsigned long long)k.b, (unsigned long long)k.e, k.slot, k.hslot, k.po, k.dec, k.bytes.empty() ? 0u : k.bytes[0], got.bad, (unsigned long long)got.aoff,
           (unsigned long long)got.doff, got.aad_len, got.pkt_len, (unsigned long long)got.num, want.bad, (unsigned long long)want.aoff, (unsigned long long)want.doff, want.aad_len,
           want.pkt_len, (unsigned long long)want.num);
    exit(1);
}

// the cut as aesgcm_batch3_body.inc makes it: the slot, the format's cut, the slot's `set`, a refused packet's lengths zero
template <u32 WIREX>
static Cut run_cut(const Pkt &k, const aesgcm_wire_fmt &f) {
    const u64 off[2] = {k.b, k.e};
    KtWireXParams xp;
    memset(&xp, 0, sizeof xp);
    BatchParams &p = xp.w.k.b;
    p.in = p.aad = k.bytes.data(); p.out = const_cast<unsigned char *>(k.bytes.data()); p.data_off = off;
    xp.w.k.slots = &k.slot; xp.w.k.tab = g_tab; xp.w.k.n_slots = N_SLOTS;
    xp.w.f = f;
    if (WIREX == KT_WIREX_QUIC || WIREX == KT_WIREX_DTLS13) { xp.seq = &k.seq; xp.pn_off = &k.po; xp.hp_slots = &k.hslot; }
    else if (WIREX == KT_WIREX_SRTCP) xp.mki_len = k.mki_len;
    else if (WIREX == KT_WIREX_TLS13 || WIREX == KT_WIREX_TLS12) xp.seq = &k.seq;
    else xp.hi = &k.hi;
    Cut c = {false, 0, 0, 0, 0, 0};
    const unsigned char *ivp = nullptr;
    const KtSlot *ks = kt_slot(g_tab, N_SLOTS, k.slot, c.bad);
    wire_cut<WIREX>(p, &xp.w.k, &xp.w.f, &xp, ks, 0u, k.dec, c.bad, c.aoff, c.doff, c.aad_len, c.pkt_len, c.num, ivp);
    c.bad |= ks->set != KT_SET;
    if (c.bad) c.pkt_len = c.aad_len = 0;
    if (!c.bad) {                           // the rest of what a format decides reads inside the packet too
        u32 iv0, iv1, iv2;
        wire_nonce<WIREX>(&xp.w.f, &xp, ks, ivp, p.in + c.aoff, p.in + c.doff, c.pkt_len, c.num, 0u, c.bad, iv0, iv1, iv2);
        if constexpr (wire_aad_built(WIREX)) for (u32 o = 0; o < c.aad_len; o += 16u) (void)wire_aad_block<WIREX>(&xp, p.aad + c.aoff, p.in + c.doff, c.aad_len, c.pkt_len, o, 0u);
        const u64 at = wire_tag_place<WIREX>(p, &xp.w.f, &xp, 0u);
        if (at < k.b || at + f.tag_len > k.e || at != c.doff + c.pkt_len) fail("the tag's place", k, c, c);
    }
    g_packets++;
    return c;
}
static void same(const char *what, const Pkt &k, const Cut &got, const Cut &want) {
    if (got.bad != want.bad) fail(what, k, got, want);
    if (!want.bad && (got.aoff != want.aoff || got.doff != want.doff || got.aad_len != want.aad_len || got.pkt_len != want.pkt_len || got.num != want.num)) fail(what, k, got, want);
    if (want.bad && (got.aad_len || got.pkt_len)) fail(what, k, got, want);
}

// the mask kernels' side of a QUIC / DTLS 1.3 packet: -> taken
static bool run_mask(const Pkt &k, bool dtls) {
    const u64 off[2] = {k.b, k.e};
    KtQuicHpParams q;
    memset(&q, 0, sizeof q);
    q.in = k.bytes.data(); q.out = const_cast<unsigned char *>(k.bytes.data()); q.pkt_off = off; q.slots = &k.slot; q.hp_slots = &k.hslot; q.pn_off = &k.po; q.pn = &k.seq;
    q.tab = g_tab; q.n_pkts = 1; q.n_slots = N_SLOTS;
    MaskPkt m;
    if (!mask_take(q, 0u, dtls ? DTLS13_TAIL : QUIC_TAIL, m)) return false;
    if (!dtls) return !quic_pn_bad(q.pn[0], k.dec);
    bool bad = false;
    (void)dtls13_hdr(m.src[0], m.po, m.len, bad);
    return !bad;
}

// ---------------------------------------------------------------- the rules, restated
static bool slots_ok(const Pkt &k, bool two) { return k.slot < 3u && (!two || k.hslot < 3u); }
static Cut ref_wire(const Pkt &k, const aesgcm_wire_fmt &f, u32 wirex) {          // kt_common.wire_split / x_split / tls_fixture: aad, payload offset and length
    Cut c = {true, 0, 0, 0, 0, 0};
    if (!slots_ok(k, false) || k.e < k.b) return c;
    const u64 len = k.e - k.b;
    const bool auth_only = (f.flags & AESGCM_WIRE_AUTH_ONLY) != 0;
    u32 front = f.hdr_len;
    if (auth_only && f.iv_off + 12u - f.salt_len > front) front = f.iv_off + 12u - f.salt_len;
    if (len >= ((u64)1 << 28) || len < front + f.tag_len) return c;
    if ((wirex == KT_WIREX_TLS13 || wirex == KT_WIREX_TLS12) && len > 5u + 65535u) return c;
    if (wirex == KT_WIREX_DTLS12 && len > 13u + 65535u) return c;
    const u32 body = (u32)len - f.tag_len;
    c.bad = false; c.aoff = k.b;
    c.aad_len = auth_only ? body : f.aad_len;
    c.doff = k.b + (auth_only ? body : f.hdr_len);
    c.pkt_len = auth_only ? 0u : body - f.hdr_len;
    if (wirex == AESGCM_WIREX_ESN) c.aad_len = 12;
    if (wirex == KT_WIREX_TLS12 || wirex == KT_WIREX_DTLS12) c.aad_len = 13;
    return c;
}
static bool ref_front(const Pkt &k, u32 tail) { return slots_ok(k, true) && k.e >= k.b && k.e - k.b <= 65535u && k.po != 0u && (u64)k.po + tail <= k.e - k.b; }
static Cut ref_quic(const Pkt &k) {
    Cut c = {true, 0, 0, 0, 0, 0};
    if (!ref_front(k, 20u) || (k.dec == 0 && k.seq >= ((u64)1 << 62))) return c;
    const u32 hdr = k.po + (k.bytes[k.b] & 3u) + 1u;
    c.bad = false; c.aoff = k.b; c.aad_len = hdr; c.doff = k.b + hdr; c.pkt_len = (u32)(k.e - k.b) - 16u - hdr; c.num = k.seq;
    return c;
}
static Cut ref_dtls13(const Pkt &k) {
    Cut c = {true, 0, 0, 0, 0, 0};
    if (!ref_front(k, 17u)) return c;
    const u32 b0 = k.bytes[k.b];
    if ((b0 >> 5) != 1u) return c;
    const u32 hdr = k.po + ((b0 & 8u) ? 2u : 1u) + ((b0 & 4u) ? 2u : 0u);
    if ((u64)hdr + 16u > k.e - k.b) return c;
    c.bad = false; c.aoff = k.b; c.aad_len = hdr; c.doff = k.b + hdr; c.pkt_len = (u32)(k.e - k.b) - 16u - hdr; c.num = k.seq;
    return c;
}
static Cut ref_rtp(const Pkt &k, bool rtcp) {
    Cut c = {true, 0, 0, 0, 0, 0};
    const u32 tail = 16u + k.mki_len + (rtcp ? 4u : 0u);
    if (!slots_ok(k, false) || k.e < k.b || k.e - k.b > 65535u || k.e - k.b < (rtcp ? 8u : 12u) + tail) return c;
    const u32 L = (u32)(k.e - k.b);
    const unsigned char *d = k.bytes.data() + k.b;
    if ((d[0] >> 6) != 2u) return c;
    c.aoff = k.b;
    if (!rtcp) {
        u32 hdr = 12u + 4u * (d[0] & 15u);
        if (hdr + tail > L) return c;
        if (d[0] & 0x10u) {
            if (hdr + 4u + tail > L) return c;
            hdr += 4u + 4u * (((u32)d[hdr + 2] << 8) | d[hdr + 3]);
            if (hdr + tail > L) return c;
        }
        c.bad = false; c.aad_len = hdr; c.doff = k.b + hdr; c.pkt_len = L - tail - hdr;
    } else {
        const u32 body = L - tail;
        const bool enc = (d[body + 16u] & 0x80u) != 0;
        c.bad = false; c.aad_len = enc ? 12u : body + 4u; c.doff = k.b + (enc ? 8u : body); c.pkt_len = enc ? body - 8u : 0u;
    }
    return c;
}

// ---------------------------------------------------------------- packets
static Pkt packet(u32 len) {
    Pkt k;
    k.bytes.reserve(len ? len : 1);                     // (never a null pointer: a call's d_in is none either)
    k.bytes.resize(len);
    for (auto &x : k.bytes) x = (unsigned char)rnd();
    k.e = len;
    k.slot = rnd_below(3); k.hslot = rnd_below(3);
    k.seq = rnd() >> 3; k.hi = (u32)rnd();
    k.dec = (int)rnd_below(2);
    return k;
}
// one in eight packets of a seeded run gets something wrong with its slots or offsets
static void spoil(Pkt &k, bool two) {
    switch (rnd_below(two ? 32 : 24)) {
    case 0: k.slot = N_SLOTS; break;
    case 1: k.slot = 3; break;
    case 2: if (k.e > 1) { k.b = k.e; k.e = k.b - 1 - rnd_below((u32)k.b - 1); k.bytes.resize(k.b); } break;        // falling
    case 3: if (two) k.hslot = N_SLOTS + rnd_below(2) * 0xFFFFFFFBu; break;
    case 4: if (two) k.hslot = 3; break;
    case 5: if (two) k.po = 0; break;
    case 6: if (two) k.seq |= (u64)1 << 62; break;
    default: break;
    }
}

template <u32 WIREX>
static void check_wire(const Pkt &k, const aesgcm_wire_fmt &f, const char *what) { same(what, k, run_cut<WIREX>(k, f), ref_wire(k, f, WIREX)); }
static void check_quic(const Pkt &k, const char *what) {
    static const aesgcm_wire_fmt f = {0, 0, 0, 0, 16, 0};
    const Cut c = run_cut<KT_WIREX_QUIC>(k, f);
    same(what, k, c, ref_quic(k));
    if (run_mask(k, false) == c.bad) fail("QUIC: the two kernels disagree", k, c, c);
}
static void check_dtls13(const Pkt &k, const char *what) {
    static const aesgcm_wire_fmt f = {0, 0, 0, 0, 16, 0};
    const Cut c = run_cut<KT_WIREX_DTLS13>(k, f);
    same(what, k, c, ref_dtls13(k));
    if (run_mask(k, true) == c.bad) fail("DTLS 1.3: the two kernels disagree", k, c, c);
}
static void check_rtp(const Pkt &k, bool rtcp, const char *what) {
    static const aesgcm_wire_fmt f = {0, 0, 0, 0, 16, 0};
    if (rtcp) same(what, k, run_cut<KT_WIREX_SRTCP>(k, f), ref_rtp(k, rtcp));
}

static void expect(bool ok, const char *what) { if (!ok) { printf("FAILED edge: %s\n", what); exit(1); } }

int main() {
    g_tab = static_cast<KtSlot *>(aligned_alloc(128, N_SLOTS * sizeof(KtSlot)));
    memset(g_tab, 0, N_SLOTS * sizeof(KtSlot));
    for (u32 s = 0; s < 3; s++) { g_tab[s].set = KT_SET; for (u32 w = 0; w < 4; w++) g_tab[s].xpn[w] = (u32)rnd(); g_tab[s].salt[0] = (u32)rnd(); g_tab[s].salt[1] = (u32)rnd(); }
    const int N = 3000;
    // ---- the plain wire family: the formats of the library's constructors (lib.py WireFormat / WireFormatX / TlsFormat / DtlsFormat)
    static const aesgcm_wire_fmt macsec = {28, 28, 16, 8, 16, 0}, macsec_nosci = {20, 20, 16, 8, 16, 0}, macsec_auth = {20, 20, 16, 8, 16, AESGCM_WIRE_AUTH_ONLY}, esp16 = {8, 16, 8, 4, 16, 0},
                                 esp12 = {8, 16, 8, 4, 12, 0}, esp8 = {8, 16, 8, 4, 8, 0}, tls13 = {5, 5, 5, 0, 16, 0}, tls12 = {13, 13, 5, 4, 16, 0}, dtls12 = {13, 21, 13, 4, 16, 0},
                                 nosalt = {12, 12, 0, 0, 16, 0};
    for (int i = 0; i < N; i++) {
        Pkt k = packet(rnd_below(8) ? rnd_below(200) : rnd_below(1600));
        spoil(k, false);
        check_wire<0u>(k, macsec, "macsec"); check_wire<0u>(k, macsec_nosci, "macsec without SCI"); check_wire<0u>(k, macsec_auth, "macsec auth-only");
        check_wire<0u>(k, esp16, "esp16"); check_wire<0u>(k, esp12, "esp12"); check_wire<0u>(k, esp8, "esp8"); check_wire<0u>(k, nosalt, "no salt");
        check_wire<AESGCM_WIREX_XPN>(k, macsec, "xpn"); check_wire<AESGCM_WIREX_XPN>(k, macsec_auth, "xpn auth-only"); check_wire<AESGCM_WIREX_ESN>(k, esp16, "esn");
        check_wire<KT_WIREX_TLS13>(k, tls13, "tls13"); check_wire<KT_WIREX_TLS12>(k, tls12, "tls12"); check_wire<KT_WIREX_DTLS12>(k, dtls12, "dtls12");
    }
    // one byte too short for header + tag, and exactly long enough; the record-length limits
    struct { const aesgcm_wire_fmt *f; u32 need; } shorts[] = {{&macsec, 44}, {&macsec_auth, 36}, {&esp16, 32}, {&esp8, 24}, {&tls13, 21}, {&tls12, 29}, {&dtls12, 37}};
    for (auto &s : shorts) {
        Pkt a = packet(s.need - 1), b = packet(s.need);
        expect(run_cut<0u>(a, *s.f).bad && !run_cut<0u>(b, *s.f).bad, "a frame one byte too short for header and ICV");
        check_wire<0u>(a, *s.f, "short"); check_wire<0u>(b, *s.f, "just long enough");
    }
    { Pkt a = packet(5 + 65535), b = packet(5 + 65536); check_wire<KT_WIREX_TLS13>(a, tls13, "tls13 longest"); check_wire<KT_WIREX_TLS13>(b, tls13, "tls13 too long");
      check_wire<KT_WIREX_TLS12>(a, tls12, "tls12 longest"); check_wire<KT_WIREX_TLS12>(b, tls12, "tls12 too long");
      expect(!run_cut<KT_WIREX_TLS13>(a, tls13).bad && run_cut<KT_WIREX_TLS13>(b, tls13).bad && !run_cut<0u>(b, tls13).bad, "a TLS record of 5 + 65535 / 65536 bytes");
      Pkt c = packet(13 + 65535), d = packet(13 + 65536); check_wire<KT_WIREX_DTLS12>(c, dtls12, "dtls12 longest"); check_wire<KT_WIREX_DTLS12>(d, dtls12, "dtls12 too long");
      expect(!run_cut<KT_WIREX_DTLS12>(c, dtls12).bad && run_cut<KT_WIREX_DTLS12>(d, dtls12).bad, "a DTLS 1.2 record of 13 + 65535 / 65536 bytes"); }
    for (int which = 0; which < 3; which++) {                               // slot = n_slots, unset slot, falling offsets
        Pkt k = packet(100);
        if (which == 0) k.slot = N_SLOTS; else if (which == 1) k.slot = 3; else { k.b = 100; k.e = 40; }
        expect(run_cut<0u>(k, macsec).bad && run_cut<AESGCM_WIREX_ESN>(k, esp16).bad && run_cut<KT_WIREX_TLS12>(k, tls12).bad, "slot = n_slots / unset slot / falling offsets");
        check_wire<0u>(k, macsec, "refused frame");
    }
    // ---- QUIC
    for (int i = 0; i < N; i++) {
        Pkt k = packet(rnd_below(300));
        k.po = rnd_below(4) ? 1 + rnd_below(40) : rnd_below((u32)k.e + 4);
        spoil(k, true);
        check_quic(k, "quic");
    }
    for (u32 po : {1u, 7u, 30u}) for (u32 room : {19u, 20u}) {             // pn_off + 19 / + 20 bytes to the end
        Pkt k = packet(po + room); k.po = po; k.dec = 1;
        check_quic(k, "quic tail");
        expect(run_cut<KT_WIREX_QUIC>(k, tls13).bad == (room == 19u), "QUIC: pn_off + 19 / + 20 bytes to the packet's end");
    }
    for (int which = 0; which < 9; which++) {
        Pkt k = packet(which == 5 ? 65535 : which == 6 ? 65536 : 120);
        k.po = 9; k.dec = which == 8 ? 1 : 0; k.seq &= ((u64)1 << 62) - 1;
        if (which == 0) k.po = 0; else if (which == 1) k.slot = N_SLOTS; else if (which == 2) k.hslot = N_SLOTS; else if (which == 3) k.slot = 3; else if (which == 4) k.hslot = 3;
        else if (which == 7 || which == 8) k.seq = (u64)1 << 62;
        check_quic(k, "quic edge");
        expect(run_cut<KT_WIREX_QUIC>(k, tls13).bad == (which != 5 && which != 8), "QUIC: pn_off 0, slots, 65535 / 65536 bytes, a number of 2^62");
    }
    { Pkt k = packet(100); k.b = 100; k.e = 50; k.po = 3; check_quic(k, "quic falling"); expect(run_cut<KT_WIREX_QUIC>(k, tls13).bad, "QUIC: falling offsets"); }
    // ---- DTLS 1.3
    for (int i = 0; i < N; i++) {
        Pkt k = packet(rnd_below(300));
        if (!k.bytes.empty() && rnd_below(8)) k.bytes[0] = (unsigned char)(0x20u | (k.bytes[0] & 0x1Fu));
        k.po = rnd_below(4) ? 1 + rnd_below(12) : rnd_below((u32)k.e + 4);
        spoil(k, true);
        k.seq = rnd();                                                      // any 64-bit number
        check_dtls13(k, "dtls13");
    }
    for (u32 b0 : {0x1Fu, 0x20u, 0x3Fu, 0x40u, 0x24u, 0x28u, 0x2Cu}) for (u32 room : {16u, 17u, 18u, 19u, 20u}) for (u32 po : {1u, 3u}) {     // the first byte; pn_off + 16 / + 17 bytes to the end
        Pkt k = packet(po + room); k.po = po; k.bytes[0] = (unsigned char)b0;
        check_dtls13(k, "dtls13 first byte and tail");
        const u32 hdr = po + ((b0 & 8u) ? 2u : 1u) + ((b0 & 4u) ? 2u : 0u);
        expect(run_cut<KT_WIREX_DTLS13>(k, tls13).bad == (b0 == 0x1Fu || b0 == 0x40u || room < 17u || hdr + 16u > po + room), "DTLS 1.3: first byte 0x1F / 0x20 / 0x3F / 0x40, pn_off + 16 / + 17");
    }
    for (int which = 0; which < 8; which++) {
        Pkt k = packet(which == 5 ? 65535 : which == 6 ? 65536 : 120);
        k.po = 1; k.bytes[0] = 0x2C;
        if (which == 0) k.po = 0; else if (which == 1) k.slot = N_SLOTS; else if (which == 2) k.hslot = N_SLOTS; else if (which == 3) k.slot = 3; else if (which == 4) k.hslot = 3;
        else if (which == 7) { k.b = 120; k.e = 119; }
        check_dtls13(k, "dtls13 edge");
        expect(run_cut<KT_WIREX_DTLS13>(k, tls13).bad == (which != 5), "DTLS 1.3: pn_off 0, slots, 65535 / 65536 bytes, falling offsets");
    }
    // ---- SRTP and SRTCP
    for (int i = 0; i < N; i++) {
        Pkt k = packet(rnd_below(260));
        k.mki_len = rnd_below(3) ? 0 : rnd_below(9);
        if (!k.bytes.empty() && rnd_below(8)) k.bytes[0] = (unsigned char)(0x80u | (k.bytes[0] & 0x3Fu));
        if (k.bytes.size() > 80 && rnd_below(2)) { const u32 at = 12u + 4u * (k.bytes[0] & 15u) + 2u; k.bytes[at] = 0; k.bytes[at + 1] = (unsigned char)rnd_below(12); }      // an extension that may fit
        spoil(k, false);
        check_rtp(k, false, "srtp"); check_rtp(k, true, "srtcp");
    }
    for (u32 mki : {0u, 4u}) {
        for (int d = -1; d <= 0; d++) {                                     // one byte too short for the fixed header and the tail
            Pkt a = packet(12 + 16 + mki + d); a.mki_len = mki; a.bytes[0] = 0x80;
            Pkt b = packet(8 + 20 + mki + d); b.mki_len = mki; b.bytes[0] = 0x80;
            check_rtp(a, false, "srtp short"); check_rtp(b, true, "srtcp short");
            expect(run_cut<KT_WIREX_SRTCP>(b, tls13).bad == (d < 0), "SRTCP: one byte too short for header and tail");
        }
        for (int d = -1; d <= 0; d++) {                                     // CC = 15 and X set, the extension's length points one byte past the tail / just fits
            const u32 xl = 3, hdr = 12 + 60 + 4 + 4 * xl;
            Pkt k = packet(hdr + 16 + mki + d); k.mki_len = mki; k.bytes[0] = 0x9F; k.bytes[12 + 60 + 2] = 0; k.bytes[12 + 60 + 3] = (unsigned char)xl;
            check_rtp(k, false, "srtp extension");
            expect(ref_rtp(k, false).bad == (d < 0), "RTP with CC = 15 and X set whose extension ends one byte past the tail (the restated rule: SRTP's cut is text in the body)");
        }
        for (u32 e_bit : {0u, 0x80u}) {                                     // SRTCP with a bare 8-byte header, E clear and set
            Pkt k = packet(8 + 16 + 4 + mki); k.mki_len = mki; k.bytes[0] = 0x80; k.bytes[24] = (unsigned char)(e_bit | 0x12);
            check_rtp(k, true, "srtcp bare header");
            const Cut c = run_cut<KT_WIREX_SRTCP>(k, tls13);
            expect(!c.bad && c.aad_len == 12u && c.pkt_len == 0u && c.doff == 8u, "SRTCP with a bare 8-byte header");
        }
        { Pkt k = packet(65535); k.mki_len = mki; k.bytes[0] = 0x80; check_rtp(k, false, "srtp 65535"); check_rtp(k, true, "srtcp 65535");
          Pkt l = packet(65536); l.mki_len = mki; l.bytes[0] = 0x80; check_rtp(l, false, "srtp 65536"); check_rtp(l, true, "srtcp 65536");
          expect(run_cut<KT_WIREX_SRTCP>(l, tls13).bad, "SRTCP: 65536 bytes"); }
    }
    for (int which = 0; which < 3; which++) {
        Pkt k = packet(100); k.bytes[0] = 0x80;
        if (which == 0) k.slot = N_SLOTS; else if (which == 1) k.slot = 3; else { k.b = 100; k.e = 99; }
        check_rtp(k, false, "srtp refused"); check_rtp(k, true, "srtcp refused");
        expect(run_cut<KT_WIREX_SRTCP>(k, tls13).bad, "SRTCP: slot = n_slots / unset slot / falling offsets");
    }
    free(g_tab);
    printf("WIRECUT OK %zu\n", g_packets);
    return 0;
}
