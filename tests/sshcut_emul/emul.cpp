// CPU harness for SSH's cut and nonce in csrc/aesgcm_wirecut.h (__host__ __device__: cut_ssh, nonce_iv_add_num), the sibling of tests/wirecut_emul for the one
// format that came after it: it runs the SAME functions k_kt_ssh runs, through the wire_cut / wire_nonce templates the body calls, one packet at a time.  Every
// packet lies alone in a heap block of exactly its size and every per-packet array has exactly one entry, so that under the address sanitizer (`make emul_asan`) a
// byte read past a packet -- or anything read of a packet past the test that refuses it, where that would leave the block -- is an error.
//   emul          seeded packets and the refusal edges against the rule restated below in plain C++ (RFC 5647 7.2 / 7.3), the add-nonce's carries; it takes no
//                 input and prints "SSHCUT OK <packets>"; a failed expectation prints the case and exits 1
//   emul script   the caller's packets, one per line of standard input -- "iv[12] seq packet", iv and packet in hex, seq decimal; the packet lies under slot 0, whose
//                 IV field holds iv as aesgcm_keytab_set_tls_iv leaves it  -> "refused" | "ok aad_len doff pkt_len nonce[12]"   (tests/test_ssh_cpu.py holds the lines
//                 to tests/ssh_fixture.py)
// Test infrastructure only; it never runs on a GPU.
#include "../../aes-gcm-128-192-256-bits_amd/csrc/aesgcm_wirecut.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

static u64 g_rng = 0x737368;
static u64 rnd() { u64 z = (g_rng += 0x9E3779B97F4A7C15ull); z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
static u32 rnd_below(u32 n) { return (u32)(rnd() % n); }

#define N_SLOTS 4u                          /* slot 3 is unset */
static KtSlot *g_tab;
static size_t g_packets;
static const aesgcm_wire_fmt g_fmt = {4, 4, 4, 0, 16, 0};      // what aesgcm_keytab_ssh_crypt_dev hands the kernel

struct Pkt {                                // one packet and what the call says about it
    std::vector<unsigned char> bytes;       // the arena: exactly the packet (falling offsets: `b` bytes)
    u64 b = 0, e = 0, seq = 0;
    u32 slot = 0;
    int dec = 0;
};
struct Cut { bool bad; u64 aoff, doff; u32 aad_len, pkt_len; };

static void fail(const char *what, const Pkt &k, const Cut &got, const Cut &want) {
    printf("FAILED %s: b %llu e %llu slot %u\n  got  bad %d aoff %llu doff %llu aad_len %u pkt_len %u\n  want bad %d aoff %llu doff %llu aad_len %u pkt_len %u\n", what,
           (unsigned long long)k.b, (unsigned long long)k.e, k.slot, got.bad, (unsigned long long)got.aoff, (unsigned long long)got.doff, got.aad_len, got.pkt_len, want.bad,
           (unsigned long long)want.aoff, (unsigned long long)want.doff, want.aad_len, want.pkt_len);
    exit(1);
}

// the cut as aesgcm_batch3_body.inc makes it: the slot, the format's cut, the slot's `set`, a refused packet's lengths zero; then the nonce and the tag's place
static Cut run_cut(const Pkt &k, u32 *nonce = nullptr) {
    const u64 off[2] = {k.b, k.e};
    KtWireXParams xp;
    memset(&xp, 0, sizeof xp);
    BatchParams &p = xp.w.k.b;
    p.in = p.aad = k.bytes.data(); p.out = const_cast<unsigned char *>(k.bytes.data()); p.data_off = off;
    xp.w.k.slots = &k.slot; xp.w.k.tab = g_tab; xp.w.k.n_slots = N_SLOTS;
    xp.w.f = g_fmt;
    xp.seq = &k.seq;
    Cut c = {false, 0, 0, 0, 0};
    u64 num = 0;
    const unsigned char *ivp = nullptr;
    const KtSlot *ks = kt_slot(g_tab, N_SLOTS, k.slot, c.bad);
    wire_cut<KT_WIREX_SSH>(p, &xp.w.k, &xp.w.f, &xp, ks, 0u, k.dec, c.bad, c.aoff, c.doff, c.aad_len, c.pkt_len, num, ivp);
    c.bad |= ks->set != KT_SET;
    if (c.bad) c.pkt_len = c.aad_len = 0;
    if (!c.bad) {
        u32 iv[3];
        wire_nonce<KT_WIREX_SSH>(&xp.w.f, &xp, ks, ivp, p.in + c.aoff, p.in + c.doff, c.pkt_len, num, 0u, c.bad, iv[0], iv[1], iv[2]);
        if (nonce) memcpy(nonce, iv, sizeof iv);
        const u64 at = wire_tag_place<KT_WIREX_SSH>(p, &xp.w.f, &xp, 0u);
        if (at < k.b || at + 16u > k.e || at != c.doff + c.pkt_len) fail("the tag's place", k, c, c);
    }
    g_packets++;
    return c;
}

// ---------------------------------------------------------------- the rule, restated: packet_length[4] | body | tag[16], the body whole cipher blocks, at least one
static Cut ref_ssh(const Pkt &k) {
    Cut c = {true, 0, 0, 0, 0};
    if (k.slot >= 3u || k.e < k.b) return c;
    const u64 len = k.e - k.b;
    if (len >= ((u64)1 << 28) || len < 36u || (len - 20u) % 16u != 0) return c;
    const unsigned char *d = k.bytes.data() + k.b;
    if ((((u32)d[0] << 24) | ((u32)d[1] << 16) | ((u32)d[2] << 8) | d[3]) != (u32)len - 20u) return c;
    c.bad = false; c.aoff = k.b; c.aad_len = 4; c.doff = k.b + 4; c.pkt_len = (u32)len - 20u;
    return c;
}
static void check(const Pkt &k, const char *what) {
    const Cut got = run_cut(k), want = ref_ssh(k);
    if (got.bad != want.bad) fail(what, k, got, want);
    if (!want.bad && (got.aoff != want.aoff || got.doff != want.doff || got.aad_len != want.aad_len || got.pkt_len != want.pkt_len)) fail(what, k, got, want);
    if (want.bad && (got.aad_len || got.pkt_len)) fail(what, k, got, want);
}
static void expect(bool ok, const char *what) { if (!ok) { printf("FAILED edge: %s\n", what); exit(1); } }

// ---------------------------------------------------------------- packets
static Pkt packet(u32 len) {
    Pkt k;
    k.bytes.reserve(len ? len : 1);                     // (never a null pointer: a call's d_in is none either)
    k.bytes.resize(len);
    for (auto &x : k.bytes) x = (unsigned char)rnd();
    k.e = len;
    k.slot = rnd_below(3);
    k.seq = rnd();
    k.dec = (int)rnd_below(2);
    return k;
}
// ... whose length field says its body's length (len >= 20)
static Pkt ssh_packet(u32 len) {
    Pkt k = packet(len);
    const u32 body = len - 20u;
    k.bytes[0] = (unsigned char)(body >> 24); k.bytes[1] = (unsigned char)(body >> 16); k.bytes[2] = (unsigned char)(body >> 8); k.bytes[3] = (unsigned char)body;
    return k;
}
// one in eight packets of the seeded run gets something wrong with its slot or offsets
static void spoil(Pkt &k) {
    switch (rnd_below(24)) {
    case 0: k.slot = N_SLOTS + rnd_below(2) * 0xFFFFFFFBu; break;
    case 1: k.slot = 3; break;
    case 2: if (k.e > 1) { k.b = k.e; k.e = k.b - 1 - rnd_below((u32)k.b - 1); k.bytes.resize(k.b); } break;        // falling
    default: break;
    }
}

static int script() {
    static char line[200000], a[64], c[190000];
    unsigned long long seq;
    while (fgets(line, sizeof line, stdin)) {
        if (sscanf(line, "%63s %llu %189999s", a, &seq, c) != 3 || strlen(a) != 24) { printf("bad script line: %.100s\n", line); return 2; }
        Pkt k;
        for (size_t i = 0; c[2 * i] && c[2 * i + 1]; i++) { unsigned b; sscanf(c + 2 * i, "%2x", &b); k.bytes.push_back((unsigned char)b); }
        k.e = k.bytes.size(); k.seq = seq;
        unsigned char iv[12];
        for (int i = 0; i < 12; i++) { unsigned b; sscanf(a + 2 * i, "%2x", &b); iv[i] = (unsigned char)b; }
        memcpy(g_tab[0].xpn, iv, 12);
        g_tab[0].xpn[3] = 0;
        u32 w[3] = {0, 0, 0};
        const Cut cut = run_cut(k, w);
        if (cut.bad) { printf("refused\n"); continue; }
        printf("ok %u %llu %u ", cut.aad_len, (unsigned long long)cut.doff, cut.pkt_len);
        for (int i = 0; i < 12; i++) printf("%02x", (w[i / 4] >> (8 * (i % 4))) & 0xFFu);
        printf("\n");
    }
    return 0;
}

int main(int argc, char **argv) {
    g_tab = static_cast<KtSlot *>(aligned_alloc(128, N_SLOTS * sizeof(KtSlot)));
    memset(g_tab, 0, N_SLOTS * sizeof(KtSlot));
    for (u32 s = 0; s < 3; s++) { g_tab[s].set = KT_SET; for (u32 w = 0; w < 3; w++) g_tab[s].xpn[w] = (u32)rnd(); }
    if (argc > 1 && !strcmp(argv[1], "script")) { const int rc = script(); free(g_tab); return rc; }
    for (int i = 0; i < 3000; i++) {
        const u32 len = rnd_below(4) ? 20u + 16u * rnd_below(12) + (rnd_below(6) ? 0u : rnd_below(16)) : rnd_below(300);      // mostly whole blocks, some ragged, some short
        Pkt k = len >= 20u ? ssh_packet(len) : packet(len);
        if (len >= 4u && !rnd_below(6)) k.bytes[rnd_below(4)] ^= (unsigned char)(1u << rnd_below(8));                        // a length field that says something else
        spoil(k);
        check(k, "ssh");
    }
    for (u32 len : {20u, 35u, 36u, 37u, 51u, 52u, 53u, 20u + 32768u}) {     // no body, one byte short of a block, one block, ragged, two blocks, a long one
        Pkt k = ssh_packet(len);
        check(k, "ssh length");
        expect(run_cut(k).bad == (len < 36u || (len - 20u) % 16u != 0), "the body is a whole number of cipher blocks and at least one");
    }
    for (int which = 0; which < 5; which++) {                               // slot = n_slots, unset slot, falling offsets, a field one more, a field with a high byte set
        Pkt k = ssh_packet(20 + 48);
        if (which == 0) k.slot = N_SLOTS; else if (which == 1) k.slot = 3; else if (which == 2) { k.b = 68; k.e = 20; } else if (which == 3) k.bytes[3]++; else k.bytes[0] = 0x80;
        check(k, "ssh refused");
        expect(run_cut(k).bad, "slot = n_slots / unset slot / falling offsets / a length field that does not say the body's length");
    }
    {   // the add-nonce: the low word's carry, the wrap at 2^64, the fixed field untouched -- against the same inputs XORed
        KtSlot s;
        memset(&s, 0, sizeof s);
        const unsigned char iv[12] = {0xA0, 0xA1, 0xA2, 0xA3, 0, 0, 0, 0, 0xFF, 0xFF, 0xFF, 0xFF};
        memcpy(s.xpn, iv, 12);
        u32 a0, a1, a2, x0, x1, x2;
        nonce_iv_add_num(&s, 1, a0, a1, a2); nonce_iv_xor_num(&s, 1, x0, x1, x2);
        expect(a0 == s.xpn[0] && a1 == bswap32(1u) && a2 == 0u && (x1 != a1 || x2 != a2), "00000000 FFFFFFFF + 1 carries into the high word; an XOR does not");
        memset(s.xpn + 1, 0xFF, 8);
        nonce_iv_add_num(&s, 3, a0, a1, a2);
        expect(a0 == s.xpn[0] && a1 == 0u && a2 == bswap32(2u), "FFFFFFFF FFFFFFFF + 3 wraps to 2 and the fixed field stays");
    }
    free(g_tab);
    printf("SSHCUT OK %zu\n", g_packets);
    return 0;
}
