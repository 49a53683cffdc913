// CPU harness for the receive windows' lane code (csrc/aesgcm_rxwin.h is __host__ __device__): it runs the SAME functions the kernels run, phase by phase as
// aesgcm_rxwin_commit_dev launches them, with the lanes of every phase in an order shuffled by a seed -- a result that depended on which lane comes first would show.
// It knows no expectation of its own: it reads a script on stdin and prints what the lane code made of it; tests/test_rxwin_cpu.py writes the scripts and holds the
// output to tests/rxwin_ref.py.  Test infrastructure only.
//   T n_wins window                  a new table, all windows empty
//   S win next seen_hex              aesgcm_rxwin_set's conversion (rx_norm_to_ring); seen_hex = the normalised form as one hexadecimal number, bit i = next - 1 - i
//   D hex | D -                      the packet bytes of the recover calls that follow
//   R rule off len flags n           a recover call of n packets; then a line "O o_0 .. o_n" (the offsets) and a line "W w_0 .. w_(n-1)" (the windows)
//                                      -> n lines "r num hi"
//   C n seed                         a commit call; then n lines "win num auth"   -> n lines "c accept why"
//   G                                -> per window "g win next seen_hex" (rx_ring_to_norm) and "n win next_new"
//   X                                -> "x status" (and clears it)
//   L T W t bits                     -> "l ok n" (rx_lowest)          P T seq -> "p v" (rx_srtp_roc)
#include "../../aes-gcm-128-192-256-bits_amd/csrc/aesgcm_rxwin.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <string>
#include <vector>

static u64 g_rng;
static u64 splitmix() { u64 z = (g_rng += 0x9E3779B97F4A7C15ull); z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
static std::vector<u32> order(u32 n) {
    std::vector<u32> o(n);
    for (u32 i = 0; i < n; i++) o[i] = i;
    for (u32 i = n; i > 1; i--) std::swap(o[i - 1], o[splitmix() % i]);
    return o;
}

static std::vector<u64> from_hex(const char *h, u32 words) {
    std::vector<u64> v(words, 0);
    const size_t n = strlen(h);
    for (size_t k = 0; k < n; k++) {
        const char c = h[n - 1 - k];
        const u64 d = c <= '9' ? c - '0' : (c | 32) - 'a' + 10;
        if (k / 16 < words) v[k / 16] |= d << (4 * (k % 16));
    }
    return v;
}
static std::string to_hex(const std::vector<u64> &v) {
    std::string s;
    char b[20];
    for (size_t k = v.size(); k-- > 0;) { snprintf(b, sizeof b, "%016llx", (unsigned long long)v[k]); s += b; }
    return s;
}

int main() {
    RxTable t = {};
    std::vector<u64> state;
    std::vector<unsigned char> data(16, 0);
    u32 status = ~0u;
    char line[1 << 16], a[1 << 15];
    auto need = [&](bool ok) { if (!ok) { printf("bad script line: %s\n", line); exit(2); } };
    while (fgets(line, sizeof line, stdin)) {
        unsigned long long x0, x1, x2, x3, x4;
        if (line[0] == 'T') {
            need(sscanf(line + 1, "%llu %llu", &x0, &x1) == 2);
            t.n_wins = (u32)x0; t.window = (u32)x1; t.stride = rx_stride_words(t.window);
            state.assign((size_t)t.n_wins * t.stride, 0);
            t.state = state.data(); t.status = &status;
        } else if (line[0] == 'S') {
            need(sscanf(line + 1, "%llu %llu %32767s", &x0, &x1, a) == 3 && x0 < t.n_wins);
            const std::vector<u64> seen = from_hex(a, t.window / 64u);
            need(rx_norm_valid(x1, seen.data(), t.window));
            u64 *r = t.state + (size_t)x0 * t.stride;
            r[0] = r[1] = x1;
            rx_norm_to_ring(x1, seen.data(), t.window, r + RX_HDR_WORDS);
        } else if (line[0] == 'D') {
            need(sscanf(line + 1, "%32767s", a) == 1);
            data.assign(16, 0);
            if (a[0] != '-') { const size_t n = strlen(a) / 2; data.assign(n + 16, 0); for (size_t k = 0; k < n; k++) { unsigned b; sscanf(a + 2 * k, "%2x", &b); data[k] = (unsigned char)b; } }
        } else if (line[0] == 'R') {
            need(sscanf(line + 1, "%llu %llu %llu %llu %llu", &x0, &x1, &x2, &x3, &x4) == 5);
            const u32 n = (u32)x4;
            std::vector<u64> off(n + 1), num(n, 7);
            std::vector<u32> win(n), hi(n, 7);
            for (int row = 0; row < 2; row++) {
                need(fgets(line, sizeof line, stdin) && line[0] == "OW"[row]);
                char *p = line + 1;
                for (u32 k = 0; k < (row ? n : n + 1); k++) { const u64 v = strtoull(p, &p, 10); if (row) win[k] = (u32)v; else off[k] = v; }
            }
            RxRecoverParams q = {};
            q.t = t; q.f.rule = (u32)x0; q.f.num_off = (u32)x1; q.f.num_len = (u32)x2; q.f.flags = (u32)x3;
            q.win = win.data(); q.in = data.data(); q.pkt_off = off.data(); q.num_out = num.data(); q.hi_out = hi.data(); q.n_pkts = n;
            for (u32 i : order(n)) rx_recover_lane(q, i);
            for (u32 i = 0; i < n; i++) printf("r %llu %u\n", (unsigned long long)num[i], hi[i]);
        } else if (line[0] == 'C') {
            need(sscanf(line + 1, "%llu %llu", &x0, &x1) == 2);
            const u32 n = (u32)x0;
            g_rng = x1;
            std::vector<u32> win(n);
            std::vector<u64> num(n);
            std::vector<int> auth(n), why(n, 9);
            for (u32 i = 0; i < n; i++) {
                need(fgets(line, sizeof line, stdin) && sscanf(line, "%llu %llu %llu", &x2, &x3, &x4) == 3);
                win[i] = (u32)x2; num[i] = x3; auth[i] = (int)x4;
            }
            RxCommitParams c = {};
            c.t = t; c.win = win.data(); c.num = num.data(); c.auth = auth.data(); c.accept = auth.data(); c.why = why.data(); c.n_pkts = n;     // accept aliases auth
            for (u32 i : order(n)) rx_commit_max_lane(c, i);
            for (u32 i : order(n)) rx_commit_clear_lane(c, i);
            for (u32 i : order(n)) rx_commit_mark_lane(c, i);
            for (u32 i = 0; i < n; i++) printf("c %d %d\n", auth[i], why[i]);
        } else if (line[0] == 'G') {
            for (u32 w = 0; w < t.n_wins; w++) {
                const u64 *r = t.state + (size_t)w * t.stride;
                std::vector<u64> seen(t.window / 64u);
                rx_ring_to_norm(r[0], r + RX_HDR_WORDS, t.window, seen.data());
                printf("g %u %llu %s\nn %u %llu\n", w, (unsigned long long)r[0], to_hex(seen).c_str(), w, (unsigned long long)r[1]);
            }
        } else if (line[0] == 'X') {
            printf("x %u\n", status);
            status = ~0u;
        } else if (line[0] == 'L') {
            need(sscanf(line + 1, "%llu %llu %llu %llu", &x0, &x1, &x2, &x3) == 4);
            u64 n = 0;
            const bool ok = rx_lowest(x0, (u32)x1, x2, (u32)x3, n);
            printf("l %d %llu\n", ok ? 1 : 0, (unsigned long long)n);
        } else if (line[0] == 'P') {
            need(sscanf(line + 1, "%llu %llu", &x0, &x1) == 2);
            printf("p %llu\n", (unsigned long long)rx_srtp_roc(x0, (u32)x1));
        } else need(line[0] == '#' || line[0] == '\n');
    }
    return 0;
}
