// CPU harness for the lane code of the TLS 1.2 PRF (csrc/aesgcm_prf12.h is __host__ __device__): it runs the SAME seed, HMACs of fixed shape, P_hash loop, window
// picks, record stores and entry verdicts that k_prf12_install, k_prf12_export and k_prf12_set run, and prints what they give.  tests/test_prf12_cpu.py writes the
// scripts and holds every line to hmac (tests/tls_fixture.prf12).  Test infrastructure only; it never runs on a GPU.
//   P hl secret label r1 r2 nbytes     P_hash(secret, label | r1 | r2): secret 48 bytes, label of 1, 13, 19 or 20 bytes, randoms 32 bytes, in hex; nbytes a multiple of 4 -> "p hex"
//   N hl ll                            the blocks of the three messages (seed, A, A | seed) under a label of ll bytes, from the lengths and the padding rule alone    -> "n b1 b2 b3"
//   T hl n_masters                     a fresh table, every record unset, the status word ~0
//   M i idx master cr sr               entry i of a set_dev call into record idx                                                   -> "m ok" | "m refused"
//   C idx                              record idx cleared
//   I kl n_slots i idx cslot sslot     entry i of an install call, all four roles; a slot '-' = the call has no such array, 'x' = 0xFFFFFFFF
//                                      -> "i ckey civ skey siv" (a direction that is not installed: "-") | "i refused"
//   E kl n_recs i idx crec srec        entry i of an export call into an SRTP master table of n_recs records, both directions: the records it stored, as
//                                      aesgcm_srtp_kdf's own store packs the same key and salt | 00 00 (compared here)            -> "e crecord srecord" | "e refused"
//   S                                  the status word, read and cleared                                                            -> "s index" | "s none"
#include "../../aes-gcm-128-192-256-bits_amd/csrc/aesgcm_prf12.h"
#include "../emul_hex.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

// P_hash with the label's length as the template argument the lane code wants.  The lengths compiled here: the two edges of the bound, 1 and 20, and the two labels
// the library uses, 13 and 19 (each instance unrolls every compression: twenty of them per hash would take the compiler many minutes)
template <int HL, int LL> static void phash_one(const u32 *ms, const Prf12Label &lab, const u32 *r, u32 n_words, u32 *out) {
    const u32 n_t = prf12_count<HL>(n_words);
    for (u32 base = 0; base < n_words; base += 8) {                      // a window of eight words at a time, as a key lane takes them; each pass runs the whole loop
        u32 win[8] = {0};
        prf12_phash<HL, LL>(ms, lab, r, n_t, [&](u32 j, const u32 *t) { prf12_pick<HL, 8>(j, t, base, win); });
        for (u32 k = 0; k < 8 && base + k < n_words; k++) out[base + k] = win[k];
    }
}
template <int HL> static bool phash_ll(u32 ll, const u32 *ms, const Prf12Label &lab, const u32 *r, u32 n_words, u32 *out) {
    if (ll == 1) phash_one<HL, 1>(ms, lab, r, n_words, out);
    else if (ll == PRF12_LL_KEY_EXPANSION) phash_one<HL, PRF12_LL_KEY_EXPANSION>(ms, lab, r, n_words, out);
    else if (ll == PRF12_LL_EXPORTER) phash_one<HL, PRF12_LL_EXPORTER>(ms, lab, r, n_words, out);
    else if (ll == PRF12_LABEL_MAX) phash_one<HL, (int)PRF12_LABEL_MAX>(ms, lab, r, n_words, out);
    else return false;
    return true;
}

template <int HL, int NK> static void install_entry(const Prf12InstallParams &p, u32 i) {
    u32 rec, slot[2], got[4][NK];
    if (!prf12_entry(p.t, p.idx, p.slots, p.n_slots, i, rec, slot)) { kdf_refuse(p.t.status, i); printf("i refused\n"); return; }
    for (u32 role = 0; role < 4; role++) if (slot[role & 1u] != PRF12_NONE) prf12_install_derive<HL, NK>(p, rec, role, got[role]);
    printf("i");
    for (u32 dir = 0; dir < 2; dir++) {
        if (slot[dir] == PRF12_NONE) { printf(" - -"); continue; }
        printf(" "); put_be(got[dir], 4 * NK); printf(" "); put_be(got[PRF12_ROLE_IV + dir], 4);
    }
    printf("\n");
}

template <int HL> static void export_entry(const Prf12ExportParams &p, u32 i) {
    u32 rec, to[2];
    if (!prf12_entry(p.t, p.idx, p.recs, p.m.n_masters, i, rec, to)) { kdf_refuse(p.t.status, i); printf("e refused\n"); return; }
    printf("e");
    for (u32 dir = 0; dir < 2; dir++) {
        if (to[dir] == PRF12_NONE) { printf(" -"); continue; }
        u32 key[8], salt[3];
        prf12_export_derive<HL>(p, rec, dir, key, salt);
        prf12_store_master(p.m, to[dir], key, salt);
        // the same key and salt | 00 00 through the SRTP unit's own store into a record of its own: the two records must be equal word for word
        unsigned char kb[32], sb[14] = {0};
        for (u32 k = 0; k < 32; k++) kb[k] = (unsigned char)(key[k / 4] >> (24 - 8 * (k % 4)));
        for (u32 k = 0; k < 12; k++) sb[k] = (unsigned char)(salt[k / 4] >> (24 - 8 * (k % 4)));
        u32 twin[KDF_REC_WORDS];
        SkdfTable one = p.m;
        one.rec = twin; one.n_masters = 1;
        skdf_store(one, 0, kb, sb);
        const u32 *mine = p.m.rec + (size_t)to[dir] * KDF_REC_WORDS;
        if (memcmp(twin, mine, sizeof twin)) { printf(" store-differs"); continue; }
        printf(" "); put_mo(mine, 4 * KDF_REC_WORDS);
    }
    printf("\n");
}

static u32 parse_dst(const char *s) { return s[0] == 'x' ? PRF12_NONE : (u32)strtoul(s, nullptr, 10); }

int main() {
    static char line[8192], a[1024], b[1024], c[1024], d[1024];
    std::vector<u32> rec;
    u32 status = 0xFFFFFFFFu;
    Prf12Table t = {};
    auto need = [&](bool ok) { if (!ok) { printf("bad script line: %s\n", line); exit(2); } };
    while (fgets(line, sizeof line, stdin)) {
        unsigned hl = 0, n = 0, i = 0, idx = 0, kl = 0, nd = 0, ll = 0;
        if (line[0] == 'P') {
            need(sscanf(line + 1, "%u %1023s %1023s %1023s %1023s %u", &hl, a, b, c, d, &n) == 6 && (hl == 32 || hl == 48) && n && n % 4 == 0 && n <= 512);
            const std::vector<unsigned char> sec = unhex(a), lab = unhex(b), r1 = unhex(c), r2 = unhex(d);
            need(sec.size() == PRF12_MASTER_LEN && !lab.empty() && lab.size() <= PRF12_LABEL_MAX && r1.size() == 32 && r2.size() == 32);
            u32 ms[12], r[16], out[128];
            be_words(sec, ms); be_words(r1, r); be_words(r2, r + 8);
            Prf12Label m;
            prf12_label(lab.data(), (u32)lab.size(), m);
            need(hl == 32 ? phash_ll<32>((u32)lab.size(), ms, m, r, n / 4, out) : phash_ll<48>((u32)lab.size(), ms, m, r, n / 4, out));
            printf("p "); put_be(out, n); printf("\n");
        } else if (line[0] == 'N') {
            // the block counts of the header's table, from the lengths alone: bytes + 0x80 + the length field, in blocks
            need(sscanf(line + 1, "%u %u", &hl, &ll) == 2 && (hl == 32 || hl == 48) && ll >= 1 && ll <= PRF12_LABEL_MAX);
            const u32 block = hl == 32 ? 64 : 128, tail = hl == 32 ? 9 : 17, sl = ll + 64;
            auto blocks = [&](u32 bytes) { return (bytes + tail + block - 1) / block; };
            printf("n %u %u %u\n", blocks(sl), blocks(hl), blocks(hl + sl));
        } else if (line[0] == 'T') {
            need(sscanf(line + 1, "%u %u", &hl, &n) == 2 && (hl == 32 || hl == 48) && n);
            rec.assign((size_t)n * PRF12_REC_WORDS, 0u);
            status = 0xFFFFFFFFu;
            t.rec = rec.data(); t.status = &status; t.n_masters = n; t.hash_len = hl;
        } else if (line[0] == 'M') {
            need(t.rec && sscanf(line + 1, "%u %u %1023s %1023s %1023s", &i, &idx, a, b, c) == 5);
            const std::vector<unsigned char> ms = unhex(a), cr = unhex(b), sr = unhex(c);
            need(ms.size() == PRF12_MASTER_LEN && cr.size() == 32 && sr.size() == 32);
            std::vector<u32> ix(i + 1, 0u);
            std::vector<unsigned char> mss((size_t)(i + 1) * 48, 0), crs((size_t)(i + 1) * 32, 0), srs((size_t)(i + 1) * 32, 0);      // exactly n * 48 / 32 bytes: a byte read past them is the sanitizer's
            ix[i] = idx;
            memcpy(&mss[(size_t)i * 48], ms.data(), 48); memcpy(&crs[(size_t)i * 32], cr.data(), 32); memcpy(&srs[(size_t)i * 32], sr.data(), 32);
            Prf12SetParams p;
            p.t = t; p.idx = ix.data(); p.masters = mss.data(); p.client_randoms = crs.data(); p.server_randoms = srs.data(); p.n = i + 1;
            const u32 before = status;
            status = 0xFFFFFFFFu;
            prf12_set_lane(p, i);
            printf(status == i ? "m refused\n" : "m ok\n");
            status = status < before ? status : before;
        } else if (line[0] == 'C') {
            need(t.rec && sscanf(line + 1, "%u", &idx) == 1 && idx < t.n_masters);
            memset(&rec[(size_t)idx * PRF12_REC_WORDS], 0, PRF12_REC_WORDS * sizeof(u32));
        } else if (line[0] == 'I' || line[0] == 'E') {
            need(t.rec && sscanf(line + 1, "%u %u %u %u %1023s %1023s", &kl, &nd, &i, &idx, a, b) == 6 && (kl == 16 || kl == 24 || kl == 32));
            std::vector<u32> ix(i + 1, 0u), cs(i + 1, 0u), ss(i + 1, 0u);
            ix[i] = idx; cs[i] = parse_dst(a); ss[i] = parse_dst(b);
            const u32 *cp = a[0] == '-' ? nullptr : cs.data(), *sp = b[0] == '-' ? nullptr : ss.data();
            need(cp || sp);
            if (line[0] == 'I') {
                Prf12InstallParams p;
                memset(&p, 0, sizeof p);
                p.t = t; p.idx = ix.data(); p.slots[PRF12_CLIENT] = cp; p.slots[PRF12_SERVER] = sp; p.n = i + 1; p.n_slots = nd;
                prf12_label((const unsigned char *)"key expansion", PRF12_LL_KEY_EXPANSION, p.label);
                if (t.hash_len == 32) { if (kl == 16) install_entry<32, 4>(p, i); else if (kl == 24) install_entry<32, 6>(p, i); else install_entry<32, 8>(p, i); }
                else { if (kl == 16) install_entry<48, 4>(p, i); else if (kl == 24) install_entry<48, 6>(p, i); else install_entry<48, 8>(p, i); }
            } else {
                need(kl != 24 && nd);
                std::vector<u32> mrec((size_t)nd * KDF_REC_WORDS, 0u);
                u32 mstatus = 0xFFFFFFFFu;
                Prf12ExportParams p;
                memset(&p, 0, sizeof p);
                p.t = t; p.idx = ix.data(); p.recs[PRF12_CLIENT] = cp; p.recs[PRF12_SERVER] = sp; p.n = i + 1;
                p.m.rec = mrec.data(); p.m.status = &mstatus; p.m.n_masters = nd; p.m.key_len = kl;
                prf12_label((const unsigned char *)"EXTRACTOR-dtls_srtp", PRF12_LL_EXPORTER, p.label);
                if (t.hash_len == 32) export_entry<32>(p, i); else export_entry<48>(p, i);
                need(mstatus == 0xFFFFFFFFu);                                // the SRTP table's status word is not this call's
            }
        } else if (line[0] == 'S') {
            if (status == 0xFFFFFFFFu) printf("s none\n"); else printf("s %u\n", status);
            status = 0xFFFFFFFFu;
        } else need(line[0] == '#' || line[0] == '\n');
    }
    return 0;
}
