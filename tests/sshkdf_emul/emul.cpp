// CPU harness for the lane code of SSH's key derivation (csrc/aesgcm_sshkdf.h is __host__ __device__): it runs the SAME hash with a run-time block count, record
// stores, loads and entry verdicts that k_sshk_install and k_sshk_set run, and prints what they give.  tests/test_ssh_cpu.py writes the scripts and holds every line
// to hashlib (tests/ssh_fixture.kdf).  Test infrastructure only; it never runs on a GPU.
//   H hl secret sid align letter       HASH(secret | letter | sid): secret 1 .. 2048 bytes, sid hl bytes, in hex; the secret lies at byte `align` of an allocation
//                                      that ends with its last byte, the sid in one of exactly hl bytes (a byte read past either is the sanitizer's)  -> "h hex"
//   B hl len                           the blocks the message of a secret of len bytes takes                                           -> "b blocks"
//   T hl max n_recs                    a fresh table, every record unset, the status word ~0
//   K i idx secret sid                 entry i of a set_dev call into record idx; secret = hex (it lies at offset i of the call's buffer, which ends with it), or
//                                      /from/to = these two offsets as they are, into 4096 zero bytes                                  -> "k ok" | "k refused"
//   C idx                              record idx cleared
//   I kl n_slots i idx c2s s2c         entry i of an install call, all four letters; a slot '-' = the call has no such array, 'x' = 0xFFFFFFFF
//                                      -> "i key_c2s iv_c2s key_s2c iv_s2c" (a direction that is not installed: "- -") | "i refused"
//   S                                  the status word, read and cleared                                                               -> "s index" | "s none"
#include "../../aes-gcm-128-192-256-bits_amd/csrc/aesgcm_sshkdf.h"
#include "../emul_hex.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

template <int HL> static void hash(const unsigned char *s, u32 len, const unsigned char *sid, u32 letter) {
    u32 out[HL / 4];
    sshk_hash<HL>(s, len, sid, letter, out);
    printf("h "); put_be(out, HL); printf("\n");
}

template <int HL> static void install_entry(const SshkInstallParams &p, u32 i, u32 kl) {
    u32 rec, slot[2], out[HL / 4];
    if (!sshk_entry(p, i, rec, slot)) { kdf_refuse(p.t.status, i); printf("i refused\n"); return; }
    printf("i");
    for (u32 dir = 0; dir < 2; dir++) {
        if (slot[dir] == SSHK_NONE) { printf(" - -"); continue; }
        sshk_derive<HL>(p.t, rec, SSHK_ROLE_KEY, dir, out);
        printf(" "); put_be(out, kl);
        sshk_derive<HL>(p.t, rec, SSHK_ROLE_IV, dir, out);
        printf(" "); put_be(out, 12);
    }
    printf("\n");
}

static u32 parse_dst(const char *s) { return s[0] == 'x' ? SSHK_NONE : (u32)strtoul(s, nullptr, 10); }

int main() {
    static char line[16384], a[8192], b[8192];
    std::vector<u32> rec;
    u32 status = 0xFFFFFFFFu;
    SshkTable t = {};
    auto need = [&](bool ok) { if (!ok) { printf("bad script line: %.200s\n", line); exit(2); } };
    while (fgets(line, sizeof line, stdin)) {
        unsigned hl = 0, n = 0, i = 0, idx = 0, kl = 0, nd = 0, al = 0, mx = 0;
        char letter = 0;
        if (line[0] == 'H') {
            need(sscanf(line + 1, "%u %8191s %8191s %u %c", &hl, a, b, &al, &letter) == 5 && (hl == 32 || hl == 48 || hl == 64) && al < 16);
            const std::vector<unsigned char> secret = unhex(a), sid = unhex(b);
            need(!secret.empty() && secret.size() <= SSHK_SECRET_MAX && sid.size() == hl);
            unsigned char *buf = (unsigned char *)malloc(al + secret.size()), *sb = (unsigned char *)malloc(hl);      // (malloc: 16-byte aligned, so `al` is the secret's alignment)
            need(buf != nullptr && sb != nullptr);
            memcpy(buf + al, secret.data(), secret.size());
            memcpy(sb, sid.data(), hl);
            if (hl == 32) hash<32>(buf + al, (u32)secret.size(), sb, (u32)letter); else if (hl == 48) hash<48>(buf + al, (u32)secret.size(), sb, (u32)letter);
            else hash<64>(buf + al, (u32)secret.size(), sb, (u32)letter);
            free(buf); free(sb);
        } else if (line[0] == 'B') {
            need(sscanf(line + 1, "%u %u", &hl, &n) == 2 && (hl == 32 || hl == 48 || hl == 64));
            printf("b %u\n", hl == 32 ? sshk_blocks<32>(n) : hl == 48 ? sshk_blocks<48>(n) : sshk_blocks<64>(n));
        } else if (line[0] == 'T') {
            need(sscanf(line + 1, "%u %u %u", &hl, &mx, &n) == 3 && (hl == 32 || hl == 48 || hl == 64) && mx && mx <= SSHK_SECRET_MAX && n);
            t.n_recs = n; t.hash_len = hl; t.max_secret_len = mx; t.rec_words = sshk_rec_words(mx);
            rec.assign((size_t)n * t.rec_words, 0u);
            status = 0xFFFFFFFFu;
            t.rec = rec.data(); t.status = &status;
        } else if (line[0] == 'K') {
            need(t.rec && sscanf(line + 1, "%u %u %8191s %8191s", &i, &idx, a, b) == 4);
            const std::vector<unsigned char> sid = unhex(b);
            need(sid.size() == t.hash_len);
            std::vector<u32> ix(i + 1, 0u), off(i + 2, 0u);
            std::vector<unsigned char> secrets, sids((size_t)(i + 1) * t.hash_len, 0);      // exactly n * hash_len bytes: a byte read past them is the sanitizer's
            ix[i] = idx;
            memcpy(&sids[(size_t)i * t.hash_len], sid.data(), t.hash_len);
            if (a[0] == '/') {
                unsigned from = 0, to = 0;
                need(sscanf(a, "/%u/%u", &from, &to) == 2 && from <= 4096 && to <= 4096);
                secrets.assign(4096, 0);
                off[i] = from; off[i + 1] = to;
            } else {
                const std::vector<unsigned char> secret = unhex(a);
                secrets.assign(i, 0xEE);
                secrets.insert(secrets.end(), secret.begin(), secret.end());
                off[i] = i; off[i + 1] = (u32)secrets.size();
                if (secrets.empty()) secrets.push_back(0);
            }
            unsigned char *buf = (unsigned char *)malloc(secrets.size());
            need(buf != nullptr);
            memcpy(buf, secrets.data(), secrets.size());
            SshkSetParams p;
            p.t = t; p.idx = ix.data(); p.secrets = buf; p.secret_off = off.data(); p.sids = sids.data(); p.n = i + 1;
            const u32 before = status;
            status = 0xFFFFFFFFu;
            sshk_set_lane(p, i);
            printf(status == i ? "k refused\n" : "k ok\n");
            status = status < before ? status : before;
            free(buf);
        } else if (line[0] == 'C') {
            need(t.rec && sscanf(line + 1, "%u", &idx) == 1 && idx < t.n_recs);
            memset(&rec[(size_t)idx * t.rec_words], 0, t.rec_words * sizeof(u32));
        } else if (line[0] == 'I') {
            need(t.rec && sscanf(line + 1, "%u %u %u %u %8191s %8191s", &kl, &nd, &i, &idx, a, b) == 6 && (kl == 16 || kl == 24 || kl == 32));
            std::vector<u32> ix(i + 1, 0u), s0(i + 1, 0u), s1(i + 1, 0u);
            ix[i] = idx; s0[i] = parse_dst(a); s1[i] = parse_dst(b);
            SshkInstallParams p;
            memset(&p, 0, sizeof p);
            p.t = t; p.idx = ix.data(); p.slots[SSHK_C2S] = a[0] == '-' ? nullptr : s0.data(); p.slots[SSHK_S2C] = b[0] == '-' ? nullptr : s1.data(); p.n = i + 1; p.n_slots = nd;
            need(p.slots[SSHK_C2S] || p.slots[SSHK_S2C]);
            if (t.hash_len == 32) install_entry<32>(p, i, kl); else if (t.hash_len == 48) install_entry<48>(p, i, kl); else install_entry<64>(p, i, kl);
        } else if (line[0] == 'S') {
            if (status == 0xFFFFFFFFu) printf("s none\n"); else printf("s %u\n", status);
            status = 0xFFFFFFFFu;
        } else need(line[0] == '#' || line[0] == '\n');
    }
    return 0;
}
