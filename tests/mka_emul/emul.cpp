// CPU harness for the lane code of MACsec's MKA (csrc/aesgcm_mka.h and kdf_key_schedule of csrc/aesgcm_kdf_slot.h are __host__ __device__): it runs the SAME inverse
// cipher, CBC-MAC with a run-time block count, KDF, wrap and unwrap steps, record stores and entry verdicts that k_mka_install, k_mka_unwrap and k_mka_set run (through
// the host paths of the LDS accessors over an LDS image that main_fill_lds and mka_fill_inv wrote), and prints what they give.  tests/test_mka_cpu.py writes the scripts
// and holds every line to tests/mka_ref.py (libcrypto).  Test infrastructure only; it never runs on a GPU.
//   D key block                        the inverse cipher: D_key(block), key 16 or 32 bytes                                          -> "d hex"
//   M key msg|- align                  AES-CMAC(key, msg) through mka_cmac; the message lies at byte `align` of an allocation that ends with its last byte (a byte
//                                      read past it is the sanitizer's)                                                              -> "m hex"
//   F key K|S out_len ctx align        KDF(key, "IEEE8021 KEK" or "IEEE8021 SAK", ctx, 8 * out_len) through mka_kdf, the context placed as M's message  -> "f hex"
//   W kek key                          RFC 3394 wrap through mka_wrap                                                                -> "w hex" (len(key) + 8 bytes)
//   T cak_len n_caks                   a fresh table, every record unset, the status word ~0
//   K i idx cak keyid                  entry i of a set_dev call into record idx                                                     -> "k ok" | "k refused"
//   C idx                              record idx cleared
//   I key_len n_slots i idx slot w ctx entry i of an install call; w = 1: the call asks for wrapped output.  ctx = hex (the context lies at offset i of the call's
//                                      buffer, which ends with it), or /from/to = these two offsets as they are, into 4096 zero bytes
//                                      -> "i sak wrapped|-" | "i refused clean" ("dirty": a byte of the wrapped buffer or of the slots changed)
//   U key_len n_slots i idx slot v wrapped   entry i of an unwrap call; v = 1: the call has verdict bytes
//                                      -> "u verdict|- sak" | "u verdict|- refused clean"
//   S                                  the status word, read and cleared                                                             -> "s index" | "s none"
// An installed entry's "slot" here is the SAK's words copied into a table of stand-in slots: the real build (kdf_slot_build) is device code, and what the harness holds
// to account is that a refused entry reaches neither it nor any byte the entry names.
#include "../../aes-gcm-128-192-256-bits_amd/csrc/aesgcm_mka.h"
#include "../emul_hex.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

static DevTables g_tb;
static unsigned char g_smem[MKA_LDS_BYTES] __attribute__((aligned(16)));
static const u32 LB = (5u & 31u) << 2;

static void mo_words(const std::vector<unsigned char> &b, u32 *w) {
    for (size_t k = 0; k < b.size() / 4; k++) w[k] = (u32)b[4 * k] | ((u32)b[4 * k + 1] << 8) | ((u32)b[4 * k + 2] << 16) | ((u32)b[4 * k + 3] << 24);
}
// an allocation that ends with the bytes' last byte, the bytes at `align` of it
struct Placed {
    unsigned char *buf, *at;
    Placed(const std::vector<unsigned char> &b, unsigned align) {
        buf = (unsigned char *)malloc(align + b.size() + (b.empty() && !align ? 1 : 0));
        if (!buf) exit(3);
        at = buf + align;
        if (!b.empty()) memcpy(at, b.data(), b.size());
    }
    ~Placed() { free(buf); }
};

template <int NR> static void schedule(const std::vector<unsigned char> &key, u32 *rk) {
    mo_words(key, rk);
    kdf_key_schedule<NR>(rk, g_smem, LB);
}
template <int NR> static void inv_block(const std::vector<unsigned char> &key, const std::vector<unsigned char> &blk) {
    u32 rk[4 * (NR + 1)], s[4];
    schedule<NR>(key, rk);
    mo_words(blk, s);
    mka_aes_inv<NR>(s[0], s[1], s[2], s[3], rk, g_smem);
    printf("d "); put_mo(s, 16); printf("\n");
}
template <int NR> static void cmac(const std::vector<unsigned char> &key, const unsigned char *m, u32 n) {
    u32 rk[4 * (NR + 1)], x[4];
    MkaSub sub;
    schedule<NR>(key, rk);
    mka_subkeys<NR>(rk, g_smem, LB, sub);
    mka_cmac<NR>(rk, sub, g_smem, LB, n, [&](u32 q) {
        u32 w = 0;
        for (u32 b = 0; b < 4u; b++) w |= (q + b < n ? (u32)m[q + b] : q + b == n ? 0x80u : 0u) << (8u * b);
        return w;
    }, x);
    printf("m "); put_mo(x, 16); printf("\n");
}
template <int NR, int NKO> static void kdf(const std::vector<unsigned char> &key, u32 w2, const unsigned char *c, u32 len) {
    u32 rk[4 * (NR + 1)], out[NKO];
    MkaSub sub;
    schedule<NR>(key, rk);
    mka_subkeys<NR>(rk, g_smem, LB, sub);
    mka_kdf<NR, NKO>(rk, sub, g_smem, LB, w2, c, len, out);
    printf("f "); put_mo(out, 4 * NKO); printf("\n");
}
template <int NR, int NK> static void wrap(const std::vector<unsigned char> &kek, const std::vector<unsigned char> &key) {
    u32 rk[4 * (NR + 1)], a[2], r[NK];
    schedule<NR>(kek, rk);
    mo_words(key, r);
    mka_wrap<NR, NK>(rk, g_smem, LB, a, r);
    printf("w "); put_mo(a, 8); put_mo(r, 4 * NK); printf("\n");
}

struct FakeSlot { u32 key[8]; };
static std::vector<FakeSlot> g_slots;
static bool slots_clean() {
    for (const FakeSlot &s : g_slots) for (u32 w : s.key) if (w != 0xEEEEEEEEu) return false;
    return true;
}
template <int NRC, int NRS> static void install_entry(const MkaInstallParams &p, u32 i, size_t wrapped_bytes) {
    u32 rk[4 * ((NRC > NRS ? NRC : NRS) + 1)], slot = 0;
    for (u32 &w : rk) w = 0xDDDDDDDDu;
    if (!mka_install_lane<NRC, NRS>(p, i, g_smem, LB, rk, slot)) {
        bool clean = slots_clean();
        for (size_t k = 0; k < wrapped_bytes; k++) clean = clean && p.wrapped[k] == 0xA7;
        printf(clean ? "i refused clean\n" : "i refused dirty\n");
        return;
    }
    memcpy(g_slots[slot].key, rk, 4 * (NRS - 6));
    printf("i "); put_mo(rk, 4 * (NRS - 6)); printf(" ");
    if (p.wrapped) {
        const size_t w = 4 * (NRS - 6) + 8;
        bool clean = true;
        for (size_t k = 0; k < wrapped_bytes; k++) if (k < i * w || k >= (i + 1) * w) clean = clean && p.wrapped[k] == 0xA7;
        for (size_t k = 0; k < w; k++) printf("%02x", p.wrapped[i * w + k]);
        if (!clean) printf(" dirty");
    } else printf("-");
    printf("\n");
}
template <int NRC, int NRS> static void unwrap_entry(const MkaUnwrapParams &p, u32 i) {
    u32 rk[4 * ((NRC > NRS ? NRC : NRS) + 1)], slot = 0;
    for (u32 &w : rk) w = 0xDDDDDDDDu;
    const bool ok = mka_unwrap_lane<NRC, NRS>(p, i, g_smem, LB, rk, slot);
    bool clean = slots_clean();
    for (u32 k = 0; p.verdict && k < p.n + 8u; k++) if (k != i) clean = clean && p.verdict[k] == 0xA7;
    printf("u ");
    if (p.verdict) printf("%u ", p.verdict[i]); else printf("- ");
    if (ok) { memcpy(g_slots[slot].key, rk, 4 * (NRS - 6)); put_mo(rk, 4 * (NRS - 6)); printf(clean ? "\n" : " dirty\n"); }
    else printf(clean ? "refused clean\n" : "refused dirty\n");
}
#define BY_NR(f, nrc, nrs, ...) do { if ((nrc) == 10 && (nrs) == 10) f<10, 10>(__VA_ARGS__); else if ((nrc) == 10) f<10, 14>(__VA_ARGS__); \
                                     else if ((nrs) == 10) f<14, 10>(__VA_ARGS__); else f<14, 14>(__VA_ARGS__); } while (0)

int main() {
    for (u32 x = 0; x < 256; x++) g_tb.te0[x] = te0_calc(sbox_calc(x));
    for (u32 tid = 0; tid < KDF_WG; tid++) main_fill_lds(g_smem, nullptr, &g_tb, tid, false, KDF_WG);      // T0 | T2, the kernels' own staging
    for (u32 tid = 0; tid < KDF_WG; tid++) mka_fill_inv(g_smem, tid);                                      // ... and the unwrap kernel's inverse S-box
    static char line[16384], a[8192], b[8192], c[8192];
    std::vector<u32> rec;
    u32 status = 0xFFFFFFFFu;
    MkaTable t = {};
    auto need = [&](bool ok) { if (!ok) { printf("bad script line: %.200s\n", line); exit(2); } };
    auto klen = [&](size_t n) { return n == 16 || n == 32; };
    while (fgets(line, sizeof line, stdin)) {
        unsigned n = 0, i = 0, idx = 0, kl = 0, nd = 0, al = 0, slot = 0, flag = 0;
        if (line[0] == 'D') {
            need(sscanf(line + 1, "%8191s %8191s", a, b) == 2);
            const std::vector<unsigned char> key = unhex(a), blk = unhex(b);
            need(klen(key.size()) && blk.size() == 16);
            if (key.size() == 16) inv_block<10>(key, blk); else inv_block<14>(key, blk);
        } else if (line[0] == 'M') {
            need(sscanf(line + 1, "%8191s %8191s %u", a, b, &al) == 3 && al < 16);
            const std::vector<unsigned char> key = unhex(a), msg = unhex(b);
            need(klen(key.size()));
            Placed m(msg, al);
            if (key.size() == 16) cmac<10>(key, m.at, (u32)msg.size()); else cmac<14>(key, m.at, (u32)msg.size());
        } else if (line[0] == 'F') {
            char which = 0;
            need(sscanf(line + 1, "%8191s %c %u %8191s %u", a, &which, &n, b, &al) == 5 && al < 16 && (which == 'K' || which == 'S') && klen(n));
            const std::vector<unsigned char> key = unhex(a), ctx = unhex(b);
            need(klen(key.size()) && !ctx.empty() && ctx.size() <= MKA_CTX_MAX);
            Placed m(ctx, al);
            const u32 w2 = which == 'K' ? MKA_W2_KEK : MKA_W2_SAK, len = (u32)ctx.size();
            if (key.size() == 16) { if (n == 16) kdf<10, 4>(key, w2, m.at, len); else kdf<10, 8>(key, w2, m.at, len); }
            else { if (n == 16) kdf<14, 4>(key, w2, m.at, len); else kdf<14, 8>(key, w2, m.at, len); }
        } else if (line[0] == 'W') {
            need(sscanf(line + 1, "%8191s %8191s", a, b) == 2);
            const std::vector<unsigned char> kek = unhex(a), key = unhex(b);
            need(klen(kek.size()) && klen(key.size()));
            if (kek.size() == 16) { if (key.size() == 16) wrap<10, 4>(kek, key); else wrap<10, 8>(kek, key); }
            else { if (key.size() == 16) wrap<14, 4>(kek, key); else wrap<14, 8>(kek, key); }
        } else if (line[0] == 'T') {
            need(sscanf(line + 1, "%u %u", &kl, &n) == 2 && klen(kl) && n);
            rec.assign((size_t)n * MKA_REC_WORDS, 0u);
            status = 0xFFFFFFFFu;
            t.rec = rec.data(); t.status = &status; t.n_caks = n; t.cak_len = kl;
        } else if (line[0] == 'K') {
            need(t.rec && sscanf(line + 1, "%u %u %8191s %8191s", &i, &idx, a, b) == 4);
            const std::vector<unsigned char> cak = unhex(a), keyid = unhex(b);
            need(cak.size() == t.cak_len && keyid.size() == MKA_KEYID_LEN);
            std::vector<u32> ix(i + 1, 0u);
            std::vector<unsigned char> caks((size_t)(i + 1) * t.cak_len, 0), ids((size_t)(i + 1) * MKA_KEYID_LEN, 0);      // exactly n * cak_len and n * 16 bytes: a byte read past them is the sanitizer's
            ix[i] = idx;
            memcpy(&caks[(size_t)i * t.cak_len], cak.data(), cak.size());
            memcpy(&ids[(size_t)i * MKA_KEYID_LEN], keyid.data(), keyid.size());
            MkaSetParams p;
            p.t = t; p.idx = ix.data(); p.caks = caks.data(); p.keyids = ids.data(); p.n = i + 1;
            const u32 before = status;
            status = 0xFFFFFFFFu;
            mka_set_lane(p, i);
            printf(status == i ? "k refused\n" : "k ok\n");
            status = status < before ? status : before;
        } else if (line[0] == 'C') {
            need(t.rec && sscanf(line + 1, "%u", &idx) == 1 && idx < t.n_caks);
            memset(&rec[(size_t)idx * MKA_REC_WORDS], 0, MKA_REC_WORDS * sizeof(u32));
        } else if (line[0] == 'I') {
            need(t.rec && sscanf(line + 1, "%u %u %u %u %u %u %8191s", &kl, &nd, &i, &idx, &slot, &flag, c) == 7 && klen(kl) && nd && nd <= 4096);
            std::vector<u32> ix(i + 1, 0u), sl(i + 1, 0u), off(i + 2, 0u);
            std::vector<unsigned char> ctxs;
            ix[i] = idx; sl[i] = slot;
            if (c[0] == '/') {
                unsigned from = 0, to = 0;
                need(sscanf(c, "/%u/%u", &from, &to) == 2 && from <= 4096 && to <= 4096);
                ctxs.assign(4096, 0);
                off[i] = from; off[i + 1] = to;
            } else {
                const std::vector<unsigned char> ctx = unhex(c);
                ctxs.assign(i, 0xEE);
                ctxs.insert(ctxs.end(), ctx.begin(), ctx.end());
                off[i] = i; off[i + 1] = (u32)ctxs.size();
            }
            Placed buf(ctxs, 0);
            const size_t wb = (size_t)(i + 1) * (kl + 8);
            std::vector<unsigned char> wrapped(wb, 0xA7);
            g_slots.assign(nd, FakeSlot{{0xEEEEEEEEu, 0xEEEEEEEEu, 0xEEEEEEEEu, 0xEEEEEEEEu, 0xEEEEEEEEu, 0xEEEEEEEEu, 0xEEEEEEEEu, 0xEEEEEEEEu}});
            MkaInstallParams p;
            memset(&p, 0, sizeof p);
            p.t = t; p.idx = ix.data(); p.slots = sl.data(); p.ctx = buf.at; p.ctx_off = off.data(); p.wrapped = flag ? wrapped.data() : nullptr; p.n = i + 1; p.n_slots = nd;
            BY_NR(install_entry, t.cak_len == 16 ? 10 : 14, kl == 16 ? 10 : 14, p, i, flag ? wb : 0);
        } else if (line[0] == 'U') {
            need(t.rec && sscanf(line + 1, "%u %u %u %u %u %u %8191s", &kl, &nd, &i, &idx, &slot, &flag, c) == 7 && klen(kl) && nd && nd <= 4096);
            const std::vector<unsigned char> one = unhex(c);
            need(one.size() == kl + 8);
            std::vector<u32> ix(i + 1, 0u), sl(i + 1, 0u);
            std::vector<unsigned char> all((size_t)i * (kl + 8), 0xEE), verdict(i + 1 + 8, 0xA7);
            all.insert(all.end(), one.begin(), one.end());
            ix[i] = idx; sl[i] = slot;
            Placed buf(all, 0);                                                // exactly n * (key_len + 8) bytes
            g_slots.assign(nd, FakeSlot{{0xEEEEEEEEu, 0xEEEEEEEEu, 0xEEEEEEEEu, 0xEEEEEEEEu, 0xEEEEEEEEu, 0xEEEEEEEEu, 0xEEEEEEEEu, 0xEEEEEEEEu}});
            MkaUnwrapParams p;
            memset(&p, 0, sizeof p);
            p.t = t; p.idx = ix.data(); p.slots = sl.data(); p.wrapped = buf.at; p.verdict = flag ? verdict.data() : nullptr; p.n = i + 1; p.n_slots = nd;
            BY_NR(unwrap_entry, t.cak_len == 16 ? 10 : 14, kl == 16 ? 10 : 14, p, i);
        } else if (line[0] == 'S') {
            if (status == 0xFFFFFFFFu) printf("s none\n"); else printf("s %u\n", status);
            status = 0xFFFFFFFFu;
        } else need(line[0] == '#' || line[0] == '\n');
    }
    return 0;
}
