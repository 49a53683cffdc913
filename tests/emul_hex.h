// emul_hex.h -- what the CPU harnesses of the three key derivations (tests/kdf_emul, tests/srtp_kdf_emul, tests/prf12_emul) share: hex in, hex out, bytes to the
// big-endian words the lane code takes.  Included behind the csrc header under test (u32).  Test infrastructure only.
#pragma once
#include <stdio.h>
#include <vector>

// a script's hex field ("-": no bytes)
static std::vector<unsigned char> unhex(const char *s) {
    std::vector<unsigned char> v;
    if (s[0] == '-') return v;
    for (size_t k = 0; s[2 * k] && s[2 * k + 1]; k++) { unsigned b; sscanf(s + 2 * k, "%2x", &b); v.push_back((unsigned char)b); }
    return v;
}
// the first `bytes` bytes of big-endian words / of memory-order words (byte k is bits 8 (k % 4) .. of word k / 4)
static void put_be(const u32 *w, size_t bytes) { for (size_t k = 0; k < bytes; k++) printf("%02x", (w[k / 4] >> (24 - 8 * (k % 4))) & 0xFFu); }
static void put_mo(const u32 *w, size_t bytes) { for (size_t k = 0; k < bytes; k++) printf("%02x", (w[k / 4] >> (8 * (k % 4))) & 0xFFu); }
static void be_words(const std::vector<unsigned char> &b, u32 *w) {
    for (size_t k = 0; k < b.size() / 4; k++) w[k] = ((u32)b[4 * k] << 24) | ((u32)b[4 * k + 1] << 16) | ((u32)b[4 * k + 2] << 8) | b[4 * k + 3];
}
