// CPU harness for the lane code of SRTP's key derivation (csrc/aesgcm_srtp_kdf.h and kdf_key_schedule of csrc/aesgcm_kdf_slot.h are __host__ __device__): it runs the
// SAME record store, entry verdict, x block, master key schedule and PRF blocks (through the host path of aes_rounds_lds over an LDS image that main_fill_lds wrote)
// that k_srtp_kdf_install and k_srtp_kdf_set run, and prints what they give.  tests/test_srtp_kdf_cpu.py writes the scripts and holds every line to
// tests/srtp_kdf_ref.py (libcrypto).  Test infrastructure only.
//   T key_len n_masters               a fresh table, every record unset, the status word ~0
//   M i idx key salt                  entry i of a set_dev call: key (key_len bytes) and salt (14 bytes) in hex into record idx   -> "m ok" | "m refused"
//   C idx                             record idx cleared
//   B idx label r                     the x block of record idx: x | be16(0)                                                       -> "b hex" (16 bytes)
//   I kind n_slots i idx slot r|-     entry i of an install call (r = '-': the call has no d_r), both roles                        -> "i key salt12" | "i refused"
//   S                                 the status word, read and cleared                                                            -> "s index" | "s none"
#include "../../aes-gcm-128-192-256-bits_amd/csrc/aesgcm_srtp_kdf.h"
#include "../emul_hex.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

static DevTables g_tb;
static unsigned char g_smem[AESGCM_LDS_AES_OFF + AESGCM_LDS_AES] __attribute__((aligned(16)));

// what both lanes of entry i do, short of the slot's fields: the verdict (role 0 reports), then each role's derivation
template <int NR> static void install_entry(const SkdfInstallParams &p, u32 i) {
    u32 key[8], salt[8];
    for (u32 role = 0; role < 2; role++) {
        u32 rec, slot;
        u64 r;
        if (!skdf_install_entry(p, i, rec, slot, r)) {
            if (role == SKDF_ROLE_KEY) kdf_refuse(p.t.status, i);
            if (role == SKDF_ROLE_SALT) printf("i refused\n");
            continue;
        }
        u32 rk[4 * (NR + 1)];
        skdf_derive<NR>(p.t, role, p.label[role], rec, r, rk, g_smem, (i & 31u) << 2, role == SKDF_ROLE_KEY ? key : salt);
        if (role == SKDF_ROLE_SALT) { printf("i "); put_mo(key, 4 * (NR - 6)); printf(" "); put_mo(salt, 12); printf("\n"); }
    }
}

int main() {
    for (u32 x = 0; x < 256; x++) g_tb.te0[x] = te0_calc(sbox_calc(x));
    for (u32 tid = 0; tid < KDF_WG; tid++) main_fill_lds(g_smem, nullptr, &g_tb, tid, false, KDF_WG);      // T0 | T2, the install kernel's own staging
    static char line[4096], a[2048], b[2048];
    std::vector<u32> rec;
    u32 status = 0xFFFFFFFFu;
    SkdfTable t = {};
    auto need = [&](bool ok) { if (!ok) { printf("bad script line: %s\n", line); exit(2); } };
    while (fgets(line, sizeof line, stdin)) {
        unsigned kl = 0, n = 0, i = 0, idx = 0, label = 0, kind = 0, n_slots = 0, slot = 0;
        unsigned long long r = 0;
        if (line[0] == 'T') {
            need(sscanf(line + 1, "%u %u", &kl, &n) == 2 && (kl == 16 || kl == 24 || kl == 32) && n);
            rec.assign((size_t)n * KDF_REC_WORDS, 0u);
            status = 0xFFFFFFFFu;
            t.rec = rec.data(); t.status = &status; t.n_masters = n; t.key_len = kl;
        } else if (line[0] == 'M') {
            need(t.rec && sscanf(line + 1, "%u %u %2047s %2047s", &i, &idx, a, b) == 4);
            const std::vector<unsigned char> key = unhex(a), salt = unhex(b);
            need(key.size() == t.key_len && salt.size() == SKDF_SALT_LEN);
            std::vector<u32> ix(i + 1, 0u);
            std::vector<unsigned char> keys((size_t)(i + 1) * t.key_len, 0), salts((size_t)(i + 1) * SKDF_SALT_LEN, 0);      // exactly n * key_len and n * 14 bytes: a byte read past them is the sanitizer's
            ix[i] = idx;
            memcpy(&keys[(size_t)i * t.key_len], key.data(), key.size());
            memcpy(&salts[(size_t)i * SKDF_SALT_LEN], salt.data(), salt.size());
            SkdfSetParams p;
            p.t = t; p.idx = ix.data(); p.keys = keys.data(); p.salts = salts.data(); p.n = i + 1;
            const u32 before = status;
            status = 0xFFFFFFFFu;
            skdf_set_lane(p, i);
            printf(status == i ? "m refused\n" : "m ok\n");
            status = status < before ? status : before;
        } else if (line[0] == 'C') {
            need(t.rec && sscanf(line + 1, "%u", &idx) == 1 && idx < t.n_masters);
            memset(&rec[(size_t)idx * KDF_REC_WORDS], 0, KDF_REC_WORDS * sizeof(u32));
        } else if (line[0] == 'B') {
            need(t.rec && sscanf(line + 1, "%u %u %llu", &idx, &label, &r) == 3 && idx < t.n_masters && label < 256 && r < SKDF_R_END);
            u32 x[4];
            skdf_x(t, idx, label, r, x);
            printf("b "); put_mo(x, 16); printf("\n");
        } else if (line[0] == 'I') {
            need(t.rec && sscanf(line + 1, "%u %u %u %u %u %2047s", &kind, &n_slots, &i, &idx, &slot, a) == 6);
            std::vector<u32> ix(i + 1, 0u), sl(i + 1, 0u);
            std::vector<u64> rs(i + 1, 0ull);
            ix[i] = idx; sl[i] = slot;
            if (a[0] != '-') rs[i] = strtoull(a, nullptr, 10);
            SkdfInstallParams p;
            memset(&p, 0, sizeof p);
            p.t = t; p.idx = ix.data(); p.slots = sl.data(); p.r = a[0] == '-' ? nullptr : rs.data(); p.n = i + 1; p.n_slots = n_slots;
            p.label[SKDF_ROLE_KEY] = skdf_label(kind, SKDF_ROLE_KEY); p.label[SKDF_ROLE_SALT] = skdf_label(kind, SKDF_ROLE_SALT);
            if (t.key_len == 16) install_entry<10>(p, i); else if (t.key_len == 24) install_entry<12>(p, i); else install_entry<14>(p, i);
        } else if (line[0] == 'S') {
            if (status == 0xFFFFFFFFu) printf("s none\n"); else printf("s %u\n", status);
            status = 0xFFFFFFFFu;
        } else need(line[0] == '#' || line[0] == '\n');
    }
    return 0;
}
