// CPU harness for the lane code of IKEv2's prf+ (csrc/aesgcm_prfplus.h is __host__ __device__): it runs the SAME HMAC with a run-time block count, prf+ loop, window
// picks, record stores and entry verdicts that k_prfp_install and k_prfp_set run, and prints what they give.  tests/test_prfplus_cpu.py writes the scripts and holds
// every line to hmac (tests/ikev2_ref.prf_plus).  Test infrastructure only; it never runs on a GPU.
//   H hl key seed align n_t            prf+(key, seed), n_t values T(n): key hl bytes, seed 1 .. 2048 bytes, in hex; the seed lies at byte `align` of an allocation that
//                                      ends with its last byte (a byte read past it is the sanitizer's)                                -> "h hex"
//   B hl tw len                        the blocks of the message T | S | n behind the ipad block (tw = T's words, 0 or hl / 4; len = the seed's bytes)  -> "b blocks"
//   T hl n_keys                        a fresh table, every record unset, the status word ~0
//   K i idx key                        entry i of a set_dev call into record idx                                                       -> "k ok" | "k refused"
//   C idx                              record idx cleared
//   I kl n_slots i idx i2r r2i seed    entry i of an install call, both directions; a slot '-' = the call has no such array, 'x' = 0xFFFFFFFF; seed = hex (the seed
//                                      lies at offset i of the call's buffer, which ends with it), or /from/to = these two offsets as they are, into 4096 zero bytes
//                                      -> "i key_i2r salt_i2r key_r2i salt_r2i" (a direction that is not installed: "- -") | "i refused"
//   S                                  the status word, read and cleared                                                               -> "s index" | "s none"
#include "../../aes-gcm-128-192-256-bits_amd/csrc/aesgcm_prfplus.h"
#include "../emul_hex.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

template <int HL> static void plus(const std::vector<unsigned char> &key, const unsigned char *s, u32 len, u32 n_t) {
    u32 skd[HL / 4];
    be_words(key, skd);
    printf("h ");
    prfp_plus<HL>(skd, s, len, n_t, [&](u32, const u32 *t) { put_be(t, HL); });
    printf("\n");
}

template <int HL, int NK> static void install_entry(const PrfpInstallParams &p, u32 i) {
    u32 rec, slot[2], len, got[2][NK + 1];
    const unsigned char *s;
    if (!prfp_entry(p, i, rec, slot, s, len)) { kdf_refuse(p.t.status, i); printf("i refused\n"); return; }
    printf("i");
    for (u32 dir = 0; dir < 2; dir++) {
        if (slot[dir] == PRFP_NONE) { printf(" - -"); continue; }
        prfp_install_derive<HL, NK>(p, rec, dir, s, len, got[dir]);
        printf(" "); put_be(got[dir], 4 * NK); printf(" "); put_be(got[dir] + NK, 4);
    }
    printf("\n");
}
template <int HL> static void install_kl(u32 kl, const PrfpInstallParams &p, u32 i) {
    if (kl == 16) install_entry<HL, 4>(p, i); else if (kl == 24) install_entry<HL, 6>(p, i); else install_entry<HL, 8>(p, i);
}

static u32 parse_dst(const char *s) { return s[0] == 'x' ? PRFP_NONE : (u32)strtoul(s, nullptr, 10); }

int main() {
    static char line[16384], a[8192], b[8192], c[8192];
    std::vector<u32> rec;
    u32 status = 0xFFFFFFFFu;
    PrfpTable t = {};
    auto need = [&](bool ok) { if (!ok) { printf("bad script line: %.200s\n", line); exit(2); } };
    while (fgets(line, sizeof line, stdin)) {
        unsigned hl = 0, n = 0, i = 0, idx = 0, kl = 0, nd = 0, al = 0, tw = 0;
        if (line[0] == 'H') {
            need(sscanf(line + 1, "%u %8191s %8191s %u %u", &hl, a, b, &al, &n) == 5 && (hl == 32 || hl == 48 || hl == 64) && n >= 1 && n <= 8 && al < 16);
            const std::vector<unsigned char> key = unhex(a), seed = unhex(b);
            need(key.size() == hl && !seed.empty() && seed.size() <= PRFP_SEED_MAX);
            unsigned char *buf = (unsigned char *)malloc(al + seed.size());      // (malloc: 16-byte aligned, so `al` is the seed's alignment)
            need(buf != nullptr);
            memcpy(buf + al, seed.data(), seed.size());
            if (hl == 32) plus<32>(key, buf + al, (u32)seed.size(), n); else if (hl == 48) plus<48>(key, buf + al, (u32)seed.size(), n); else plus<64>(key, buf + al, (u32)seed.size(), n);
            free(buf);
        } else if (line[0] == 'B') {
            need(sscanf(line + 1, "%u %u %u", &hl, &tw, &n) == 3 && (hl == 32 || hl == 48 || hl == 64) && (tw == 0 || tw == hl / 4));
            printf("b %u\n", hl == 32 ? prfp_blocks<32>(tw, n) : hl == 48 ? prfp_blocks<48>(tw, n) : prfp_blocks<64>(tw, n));
        } else if (line[0] == 'T') {
            need(sscanf(line + 1, "%u %u", &hl, &n) == 2 && (hl == 32 || hl == 48 || hl == 64) && n);
            rec.assign((size_t)n * PRFP_REC_WORDS, 0u);
            status = 0xFFFFFFFFu;
            t.rec = rec.data(); t.status = &status; t.n_keys = n; t.hash_len = hl;
        } else if (line[0] == 'K') {
            need(t.rec && sscanf(line + 1, "%u %u %8191s", &i, &idx, a) == 3);
            const std::vector<unsigned char> key = unhex(a);
            need(key.size() == t.hash_len);
            std::vector<u32> ix(i + 1, 0u);
            std::vector<unsigned char> keys((size_t)(i + 1) * t.hash_len, 0);      // exactly n * hash_len bytes: a byte read past them is the sanitizer's
            ix[i] = idx;
            memcpy(&keys[(size_t)i * t.hash_len], key.data(), t.hash_len);
            PrfpSetParams p;
            p.t = t; p.idx = ix.data(); p.keys = keys.data(); p.n = i + 1;
            const u32 before = status;
            status = 0xFFFFFFFFu;
            prfp_set_lane(p, i);
            printf(status == i ? "k refused\n" : "k ok\n");
            status = status < before ? status : before;
        } else if (line[0] == 'C') {
            need(t.rec && sscanf(line + 1, "%u", &idx) == 1 && idx < t.n_keys);
            memset(&rec[(size_t)idx * PRFP_REC_WORDS], 0, PRFP_REC_WORDS * sizeof(u32));
        } else if (line[0] == 'I') {
            need(t.rec && sscanf(line + 1, "%u %u %u %u %8191s %8191s %8191s", &kl, &nd, &i, &idx, a, b, c) == 7 && (kl == 16 || kl == 24 || kl == 32));
            std::vector<u32> ix(i + 1, 0u), s0(i + 1, 0u), s1(i + 1, 0u), off(i + 2, 0u);
            std::vector<unsigned char> seeds;
            ix[i] = idx; s0[i] = parse_dst(a); s1[i] = parse_dst(b);
            if (c[0] == '/') {
                unsigned from = 0, to = 0;
                need(sscanf(c, "/%u/%u", &from, &to) == 2 && from <= 4096 && to <= 4096);
                seeds.assign(4096, 0);
                off[i] = from; off[i + 1] = to;
            } else {
                const std::vector<unsigned char> seed = unhex(c);
                seeds.assign(i, 0xEE);
                seeds.insert(seeds.end(), seed.begin(), seed.end());
                off[i] = i; off[i + 1] = (u32)seeds.size();
                if (seeds.empty()) seeds.push_back(0);
            }
            unsigned char *buf = (unsigned char *)malloc(seeds.size());
            need(buf != nullptr);
            memcpy(buf, seeds.data(), seeds.size());
            PrfpInstallParams p;
            memset(&p, 0, sizeof p);
            p.t = t; p.idx = ix.data(); p.seed = buf; p.seed_off = off.data(); p.slots[PRFP_I2R] = a[0] == '-' ? nullptr : s0.data();
            p.slots[PRFP_R2I] = b[0] == '-' ? nullptr : s1.data(); p.n = i + 1; p.n_slots = nd;
            need(p.slots[PRFP_I2R] || p.slots[PRFP_R2I]);
            if (t.hash_len == 32) install_kl<32>(kl, p, i); else if (t.hash_len == 48) install_kl<48>(kl, p, i); else install_kl<64>(kl, p, i);
            free(buf);
        } else if (line[0] == 'S') {
            if (status == 0xFFFFFFFFu) printf("s none\n"); else printf("s %u\n", status);
            status = 0xFFFFFFFFu;
        } else need(line[0] == '#' || line[0] == '\n');
    }
    return 0;
}
