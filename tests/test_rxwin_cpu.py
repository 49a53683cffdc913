"""CPU: receive windows (aesgcm_rxwin_*: anti-replay and number recovery on the device) without a GPU.  The binding and the header name the entry points and the ABI
version is still 5; aesgcm_rxwin_fmt_check refuses what it must; every call refuses its argument errors before it looks at a table or a device; the lane code of
csrc/aesgcm_rxwin.h, run by the CPU harness tests/rxwin_emul phase by phase with its lanes in shuffled orders, is held to tests/rxwin_ref.py: the LOWEST rule to the
literal pseudo-code of RFC 4303 Appendix A2.1, the SRTP rule to that of RFC 3711 Appendix A, whole recover calls with their refusals, and sequences of commit calls
to a sequential window (verdicts per (window, number), the normalised state after every call); the gfx950 assembly of the kernels (`make -C csrc asm_rxwin`) holds
exactly the four kernels, none with scratch, none above the family's 128 registers."""
import ctypes
import os
import random
import subprocess

import pytest

import aesgcm_amd  # noqa: F401
from aesgcm_amd import lib

from kt_common import asm_census, assert_in_budget

import rxwin_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "aes-gcm-128-192-256-bits_amd", "csrc")
NAMES = ("create", "set", "get", "fmt_check", "recover_dev", "commit_dev", "status", "destroy")


# ---------------------------------------------------------------- binding and header
def test_rxwin_symbols_in_binding_and_header():
    hdr = open(os.path.join(ROOT, "include", "aesgcm.h")).read()
    for n in NAMES:
        assert "aesgcm_rxwin_" + n in lib.SYMBOLS
        assert "AESGCM_API int aesgcm_rxwin_%s(" % n in hdr
    assert "#define AESGCM_ABI_VERSION 5 " in hdr
    assert "#define AESGCM_RXWIN_NONE 0xFFFFFFFFFFFFFFFFull" in hdr
    for k, v in (("WIRE  ", 1), ("LOWEST", 2), ("SRTP  ", 3), ("EXPECT", 4), ("FROM_END ", 1), ("CLEAR_TOP", 2)):
        assert "#define AESGCM_RXWIN_%s %du" % (k, v) in hdr
    assert (lib.RXWIN_WIRE, lib.RXWIN_LOWEST, lib.RXWIN_SRTP, lib.RXWIN_EXPECT, lib.RXWIN_FROM_END, lib.RXWIN_CLEAR_TOP) == (1, 2, 3, 4, 1, 2) == (R.WIRE, R.LOWEST, R.SRTP, R.EXPECT,
                                                                                                                                                  R.FROM_END, R.CLEAR_TOP)
    assert lib.RXWIN_NONE == R.NONE == 2 ** 64 - 1
    section = hdr[hdr.index("RECEIVE WINDOWS: anti-replay"):hdr.index("} aesgcm_rxwin_fmt;")]
    for word in ("RFC 4303 Appendix A2.1", "802.1AEbw 10.6.2", "RFC 3711 3.3.1", "DESCENDING", "EXACTLY ONE", "SIZE `window` FOR THE", "capture-safe", "replayProtect = false",
                 "per-window counters", "MAY BE d_auth"):
        assert word in section, word
    # the family sections point here and keep the words their own tests look for
    for word in ("anti-replay windows (not this call's: aesgcm_rxwin_*", "recovering d_hi from a replay window, anti-replay itself (neither is this call's",
                 "ROC estimation and replay windows (not this call's", "anti-replay and the expected packet number (not this call's", "anti-replay (not this call's"):
        assert word in hdr, word
    L = lib._rxwin_typed(lib.load())
    assert L.aesgcm_abi_version() == 5
    assert [len(getattr(L, "aesgcm_rxwin_" + n).argtypes) for n in NAMES] == [4, 6, 6, 1, 9, 8, 3, 1]
    for m in ("set", "get", "recover_dev", "commit_dev", "status", "recover", "commit", "close", "__enter__", "__exit__"):
        assert callable(getattr(lib.RxWindows, m)), m
    F = lib.RxFormat
    fields = lambda f: (f.rule, f.num_off, f.num_len, f.flags)
    assert [fields(f) for f in (F.macsec(), F.macsec_xpn(), F.esp(), F.esp_esn(), F.dtls12(), F.srtp(), F.srtcp(0), F.srtcp(4), F.expect())] == [
        (1, 16, 4, 0), (2, 16, 4, 0), (1, 4, 4, 0), (2, 4, 4, 0), (1, 5, 6, 0), (3, 2, 2, 0), (1, 4, 4, 3), (1, 8, 4, 3), (4, 0, 0, 0)]
    assert ctypes.sizeof(F) == 16
    for doc, words in (("INTEGRATION.md", ("## Receive windows", "recover", "commit", "aesgcm_wipe_failed_dev")), ("DESIGN.md", ("Receive windows", "next_new", "test_gpu_rxwin.py", "test_rxwin_cpu.py")),
                       ("README.md", ("Receive windows", "RxWindows"))):
        text = open(os.path.join(ROOT, doc)).read()
        for w in words:
            assert w in text, (doc, w)


def test_format_check():
    F = lib.RxFormat
    for f in (F.macsec(), F.macsec_xpn(), F.esp(), F.esp_esn(), F.dtls12(), F.srtp(), F.srtcp(), F.srtcp(128), F.expect(), F(1, 0, 2, 0), F(1, 65535, 8, 3), F(2, 0, 2, 0)):
        assert f.check() == lib.OK, f
    assert lib._rxwin_typed(lib.load()).aesgcm_rxwin_fmt_check(None) == lib.EARG
    for rule in (0, 5, 8, 0x10, 0xFFFFFFFF):
        assert F(rule, 4, 4, 0).check() == lib.EARG, rule
    for rule, lens in ((1, (0, 1, 3, 5, 7, 9, 16)), (2, (0, 1, 3, 6, 8)), (3, (0, 1, 4)), (4, (1, 2, 4, 8))):
        for n in lens:
            assert F(rule, 4, n, 0).check() == lib.EARG, (rule, n)
    for fl in (4, 8, 7, 0x80000000):
        assert F(1, 4, 4, fl).check() == lib.EARG, fl                        # an unknown flag
    for rule, n in ((2, 4), (3, 2), (4, 0)):
        for fl in (1, 2, 3):
            assert F(rule, 4, n, fl).check() == lib.EARG, (rule, fl)         # flags on rules other than WIRE
    for rule, n in ((1, 4), (2, 4), (3, 2), (4, 0)):
        assert F(rule, 65535, n, 0).check() == lib.OK
        for off in (65536, 2 ** 31, 2 ** 32 - 1):
            assert F(rule, off, n, 0).check() == lib.EARG, (rule, off)


def test_argument_errors_before_any_table_or_device():
    """w = NULL and placeholder pointers that are never followed: every call returns before it touches a table or a device"""
    L = lib._rxwin_typed(lib.load())
    P = 16                                                                   # a placeholder pointer
    esn, exp = lib.RxFormat.esp_esn(), lib.RxFormat.expect()

    def rec(fmt=esn, w=None, n=1, win=P, d_in=P, off=P, num=P, hi=P):
        return L.aesgcm_rxwin_recover_dev(w, ctypes.byref(fmt) if fmt is not None else None, n, win, d_in, off, num, hi, None)

    assert rec(fmt=None, w=P) == lib.EARG                                    # the format first
    assert rec(fmt=lib.RxFormat(9, 0, 4, 0), w=P, n=0) == lib.EARG
    assert rec(fmt=lib.RxFormat(2, 4, 4, 1), w=P, n=0) == lib.EARG
    for fmt in (esn, exp):
        assert rec(fmt) == lib.EARG                                          # w NULL
        assert rec(fmt, n=0) == lib.EARG                                     # ... whatever else
        assert rec(fmt, w=P, n=0) == lib.OK                                  # nothing to do: nothing is looked at
        assert rec(fmt, w=P, n=0, win=None, num=None) == lib.OK
        assert rec(fmt, w=P, win=None) == lib.EARG
        assert rec(fmt, w=P, num=None) == lib.EARG
        assert rec(fmt, w=P, n=2 ** 31) == lib.EARG
        assert rec(fmt, w=P, n=2 ** 31 + 5, hi=None) == lib.EARG
    assert rec(esn, w=P, d_in=None) == lib.EARG and rec(esn, w=P, off=None) == lib.EARG
    # EXPECT reads no packet: with d_in and d_pkt_off NULL the next refusal is n_pkts
    assert rec(exp, w=P, n=2 ** 31, d_in=None, off=None) == lib.EARG

    def com(w=P, n=1, win=P, num=P, auth=P, accept=P, why=P):
        return L.aesgcm_rxwin_commit_dev(w, n, win, num, auth, accept, why, None)

    assert com(w=None) == lib.EARG and com(w=None, n=0) == lib.EARG
    assert com(n=0) == lib.OK and com(n=0, win=None, num=None, auth=None, accept=None, why=None) == lib.OK
    for name in ("win", "num", "auth", "accept"):
        assert com(**{name: None}) == lib.EARG, name
    assert com(n=2 ** 31) == lib.EARG and com(n=2 ** 31, why=None) == lib.EARG

    out = ctypes.c_void_p(5)
    assert L.aesgcm_rxwin_create(None, 0, 1, 64) == lib.EARG
    for n_wins, window in ((0, 64), (2 ** 31, 64), (2 ** 40, 64), (1, 0), (1, 1), (1, 32), (1, 63), (1, 65), (1, 96), (1, 4095), (1, 8192), (1, 2 ** 32 + 64)):
        assert L.aesgcm_rxwin_create(ctypes.byref(out), 0, n_wins, window) == lib.EARG, (n_wins, window)
        assert out.value is None
    one = (ctypes.c_uint64 * 1)(0)
    assert L.aesgcm_rxwin_set(None, 0, 1, one, None, None) == lib.EARG and L.aesgcm_rxwin_set(None, 0, 0, one, None, None) == lib.EARG
    assert L.aesgcm_rxwin_get(None, 0, 1, one, None, None) == lib.EARG
    code = ctypes.c_int(7)
    assert L.aesgcm_rxwin_status(None, ctypes.byref(code), None) == lib.EARG
    assert L.aesgcm_rxwin_destroy(None) == lib.OK


# ---------------------------------------------------------------- the lane code on the CPU
@pytest.fixture(scope="module")
def emul():
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    d = os.path.join(ROOT, "tests", "rxwin_emul")
    subprocess.run(["make", "-C", d, "-s"], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)

    def run(script):
        out = subprocess.run([os.path.join(d, "emul")], input="\n".join(script) + "\n", stdout=subprocess.PIPE, text=True, timeout=300)
        assert out.returncode == 0, out.stdout[-2000:]
        return [ln.split() for ln in out.stdout.splitlines()]
    return run


def test_lowest_is_rfc4303_a21(emul):
    """every T - 1 >= W - 1 (the RFC's window lies above 0) near Tl = 0, W - 2, W - 1, 2^32 - 1 with Th = 0, 1, 2^32 - 1, Seql at every boundary +- 1"""
    M = 1 << 32
    cases = []
    for W in (64, 1024, 4096):
        for Th in (0, 1, M - 1):
            for Tl in sorted({x % M for c in (0, W - 2, W - 1, M - 1) for x in (c - 1, c, c + 1)}):
                Tm1 = Th << 32 | Tl
                if Tm1 < W - 1 or Tm1 > 2 ** 64 - 2:
                    continue
                for Seql in sorted({x % M for c in (0, Tl, Tl - W + 1, M - 1) for x in (c - 1, c, c + 1)}):
                    cases.append((W, Th, Tl, Seql))
    assert len(cases) > 400
    got = emul(["L %d %d %d 32" % ((Th << 32 | Tl) + 1, W, Seql) for W, Th, Tl, Seql in cases])
    assert len(got) == len(cases)
    refused = 0
    for (W, Th, Tl, Seql), (_, ok, n) in zip(cases, got):
        Seqh = R.rfc4303_a21(Th, Tl, W, Seql)
        assert Seqh >= 0
        full = Seqh << 32 | Seql
        assert full == R.lowest((Th << 32 | Tl) + 1, W, Seql, 32)           # the header's definition is the RFC's rule
        if full >= 2 ** 64 - 1:
            assert ok == "0", (W, Th, Tl, Seql)
            refused += 1
        else:
            assert (ok, int(n)) == ("1", full), (W, Th, Tl, Seql)
    assert refused >= 6
    # below the RFC's range the window is clamped at 0, and 16-bit fields follow the same rule
    small = [(T, W, t, bits) for W in (64, 4096) for T in (0, 1, W - 1, W, W + 1, 65535 + W, 65536 + W, 65537 + W) for bits in (16, 32)
             for t in (0, 1, 2, (T - W) % (1 << bits), (T - W - 1) % (1 << bits), (1 << bits) - 1)]
    got = emul(["L %d %d %d %d" % c for c in small])
    for (T, W, t, bits), (_, ok, n) in zip(small, got):
        assert (ok, int(n)) == ("1", R.lowest(T, W, t, bits)), (T, W, t, bits)


def test_srtp_rule_is_rfc3711_appendix_a(emul):
    cases = []
    for ROC in (0, 1, 5, 2 ** 32 - 2, 2 ** 32 - 1):
        for s_l in (0, 32767, 32768, 65535):
            for SEQ in sorted({x for c in (0, s_l, s_l + 32768, s_l - 32768, 65535, 32768) for x in (c - 1, c, c + 1) if 0 <= x <= 65535}):
                cases.append((ROC, s_l, SEQ))
    got = emul(["P %d %d" % ((ROC << 16 | s_l) + 1, SEQ) for ROC, s_l, SEQ in cases])
    wraps = 0
    for (ROC, s_l, SEQ), (_, v) in zip(cases, got):
        want = R.rfc3711_index(s_l, ROC, SEQ)
        if ROC == 0 and want == 2 ** 32 - 1:
            want, wraps = 0, wraps + 1                                       # nothing goes below ROC 0
        elif ROC == 2 ** 32 - 1 and want == 0:
            want, wraps = 2 ** 32, wraps + 1                                 # would pass 2^32 - 1: the recover call refuses the packet
        assert int(v) == want == R.srtp_v((ROC << 16 | s_l) + 1, SEQ), (ROC, s_l, SEQ)
    assert wraps >= 4
    assert emul(["P 0 0", "P 0 65535", "P 0 32769"]) == [["p", "0"]] * 3     # nothing accepted yet


def _pkts(rng, n, lo=0, hi=40):
    return [bytes(rng.randrange(256) for _ in range(rng.randrange(lo, hi))) for _ in range(n)]


def test_recover_calls_and_their_refusals(emul):
    rng = random.Random(0x7278)
    n_wins, W = 3, 64
    nexts = [0, 2 ** 32 + 5, 2 ** 64 - 2]
    fmts = [(1, 16, 4, 0), (2, 16, 4, 0), (1, 4, 4, 0), (2, 4, 4, 0), (1, 5, 6, 0), (3, 2, 2, 0), (1, 4, 4, 3), (1, 8, 4, 3), (4, 0, 0, 0), (1, 0, 8, 0), (1, 2, 2, 2), (2, 1, 2, 0)]
    script = ["T %d %d" % (n_wins, W)] + ["S %d %d 0" % (w, nx) for w, nx in enumerate(nexts)]
    want = []
    for fmt in fmts:
        pk = _pkts(rng, 24) + [b"\xff" * 24, b"\xff" * 8, b"", b"\x00" * 20]
        wins = [rng.randrange(n_wins) for _ in pk]
        wins[3], wins[7] = n_wins, 2 ** 32 - 1                                # out of range
        offs = [0]
        for p in pk:
            offs.append(offs[-1] + len(p))
        data = b"".join(pk)
        offs[11] = offs[10] - 1 if offs[10] else offs[11]                      # falling offsets (packet 10), and packet 11 then starts below where 10 ended
        script += ["D " + (data.hex() or "-"), "R %d %d %d %d %d" % (fmt + (len(pk),)), "O " + " ".join(map(str, offs)), "W " + " ".join(map(str, wins)), "X"]
        res, bad = R.recover(fmt, n_wins, W, nexts, wins, data, offs)
        want += [["r", str(n), str(h)] for n, h in res] + [["x", str(2 ** 32 - 1 if bad is None else bad)]]
        assert bad is not None and any(n != R.NONE for n, _ in res), fmt
    got = emul(script)
    assert got == want, [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w][:5]
    # the rollover counter at its end, and next at its end under EXPECT
    script = ["T 2 64", "S 0 %d 0" % (((2 ** 32 - 1) << 16 | 65000) + 1), "S 1 %d 0" % (2 ** 64 - 1), "D 800000058000fde8", "R 3 2 2 0 2", "O 0 4 8", "W 0 0", "R 4 0 0 0 2", "O 0 0 0", "W 0 1", "X"]
    assert emul(script) == [["r", str(R.NONE), str(2 ** 32 - 1)], ["r", str((2 ** 32 - 1) << 16 | 0xfde8), str(2 ** 32 - 1)],
                            ["r", str(((2 ** 32 - 1) << 16 | 65000) + 1), str(((2 ** 32 - 1) << 16 | 65000) + 1 >> 32)], ["r", str(R.NONE), str(2 ** 32 - 1)], ["x", "0"]]


@pytest.mark.parametrize("n_wins,W", [(1, 64), (3, 64), (3, 1024), (2, 4096), (64, 128)])
def test_commit_phases_in_shuffled_lane_orders(emul, n_wins, W):
    rng = random.Random(1000 * n_wins + W)
    sets, calls = R.call_sequence(rng, n_wins, W)
    for seed in (1, 2, 3):
        script = ["T %d %d" % (n_wins, W)] + ["S %d %d %x" % s for s in sets]
        for wins, nums, auths, _, _, _ in calls:
            script += ["C %d %d" % (len(wins), seed * 7919 + len(script))] + ["%d %d %d" % p for p in zip(wins, nums, auths)] + ["G", "X"]
        got = emul(script)
        at = 0
        for k, (wins, nums, auths, why, state, bad) in enumerate(calls):
            n = len(wins)
            rows = got[at:at + n]
            at += n
            assert all(r[0] == "c" for r in rows)
            gwhy = [int(r[2]) for r in rows]
            assert [int(r[1]) for r in rows] == [1 if y == R.ACCEPT else 0 for y in gwhy]
            err = R.same_verdicts(wins, nums, gwhy, why)
            assert err is None, (seed, k, err)
            for w in range(n_wins):
                g, nn = got[at], got[at + 1]
                at += 2
                assert (g[0], int(g[1]), int(g[2]), int(g[3], 16)) == ("g", w) + state[w], (seed, k, w)
                assert (nn[0], int(nn[2])) == ("n", state[w][0])              # next_new is `next` again between calls
            assert got[at] == ["x", str(2 ** 32 - 1 if bad is None else bad)], (seed, k)
            at += 1
        assert at == len(got)


def test_forged_packets_do_not_move_a_window(emul):
    script = ["T 2 64", "S 0 1000 ff", "C 4 5", "0 5000 0", "0 1000 0", "1 7 0", "0 %d 0" % (2 ** 64 - 2), "G", "X"]
    assert emul(script) == [["c", "0", "0"]] * 4 + [["g", "0", "1000", "%016x" % 0xff], ["n", "0", "1000"], ["g", "1", "0", "0" * 16], ["n", "1", "0"], ["x", str(2 ** 32 - 1)]]


@pytest.mark.parametrize("W", [128, 4096])
def test_commit_phases_on_a_ring_of_several_words(emul, W):
    """R.ring_sequence (tests/test_gpu_rxwin.py runs it on the device): the partial clear inside a word, up to a word boundary, over three words, around the ring's end"""
    sets, calls = R.ring_sequence(random.Random("ring %d" % W), 3, W, 257, first_next=0)
    script = ["T 3 %d" % W] + ["S %d %d %x" % s for s in sets]
    for wins, nums, auths, _, _, _ in calls:
        script += ["C %d %d" % (len(wins), 31 * len(script))] + ["%d %d %d" % p for p in zip(wins, nums, auths)] + ["G", "X"]
    got = emul(script)
    at = 0
    for k, (wins, nums, auths, why, state, bad) in enumerate(calls):
        rows = got[at:at + len(wins)]
        at += len(wins)
        err = R.same_verdicts(wins, nums, [int(r[2]) for r in rows], why)
        assert err is None, (k, err)
        for w in range(3):
            g = got[at]
            at += 2
            assert (g[0], int(g[1]), int(g[2]), int(g[3], 16)) == ("g", w) + state[w], (k, w)
        at += 1
    assert at == len(got)


# ---------------------------------------------------------------- the new receive flows of tests/rx_loop.py, without a device
def _wire_number(name, pkt):
    """the truncated number of a packet, by a slice written out from the standard's field position"""
    if name in ("macsec", "xpn"):
        return int.from_bytes(pkt[16:20], "big")         # IEEE 802.1AE 9.3: DA[6] SA[6] | EtherType[2] TCI-AN[1] SL[1] PN[4] SCI[8]
    if name == "esp":
        return int.from_bytes(pkt[4:8], "big")           # RFC 4303 2: SPI[4] sequence number[4]
    if name == "dtls12":
        return int.from_bytes(pkt[5:11], "big")          # RFC 6347 4.1: type[1] version[2] epoch[2] sequence_number[6] length[2]
    assert name == "srtcp_mki"
    return int.from_bytes(pkt[-8:-4], "big") & 0x7FFFFFFF  # RFC 3711 3.4 / RFC 7714 9.2: ... | E[1 bit] index[31 bits] | MKI[4]


@pytest.mark.parametrize("name", ["macsec", "esp", "xpn", "dtls12", "srtcp_mki"])
def test_new_flows_open_what_they_make_and_presets_sit_on_the_wire(name):
    import rx_loop
    flow = rx_loop.Flow(lib, name, 16, 4)
    W = 64
    f = flow.fmt
    assert f.check() == lib.OK
    bits = {"macsec": 32, "esp": 32, "xpn": 32, "dtls12": 48, "srtcp_mki": 31}[name]
    nums = [0, 1, 2 ** 30 + 3, 2 ** bits - 1, flow.top, min(flow.top, 2 ** 33 + 77)] + flow.starts(W)
    for i, num in enumerate(nums):
        w, L = i % 4, (0, 1, 16, 33, 100)[i % 5]
        plain, pkt = flow.plain(w, num, i, L), flow.make(w, num, i, L)
        t = len(pkt) - flow.trail - 16
        assert len(pkt) == len(plain) and plain[t:t + 16] == rx_loop.TAG
        # the number on the wire is the one the packet was made with: by the standard's position, and by the preset's (num_off, num_len, flags)
        assert _wire_number(name, pkt) == num & (2 ** bits - 1), (name, num)
        at = len(pkt) - f.num_off if f.flags & R.FROM_END else f.num_off
        field = int.from_bytes(pkt[at:at + f.num_len], "big")
        if f.flags & R.CLEAR_TOP:
            field &= ~(1 << (8 * f.num_len - 1))
        assert field == num & (2 ** bits - 1) and 8 * f.num_len == (bits + 7) // 8 * 8, (name, num, f)
        # open(make(...)) is the identity, under the true number alone
        out, ok, cnum = flow.open(w, (num, num >> 32), pkt)
        assert ok == 1 and cnum == num and out[:t] == plain[:t] and out[t + 16:] == plain[t + 16:] and out[t:t + 16] == pkt[t:t + 16], (name, num)
        for bit in (0, 77, 127):
            bad = bytearray(pkt)
            bad[t + bit // 8] ^= 1 << (bit % 8)
            assert flow.open(w, (num, num >> 32), bytes(bad))[1] == 0, (name, num, bit)
        if name == "xpn":
            assert flow.open(w, (num, (num >> 32) ^ 1), pkt)[1] == 0             # the upper half is in the nonce
    if name == "srtcp_mki":
        e_of = lambda num: flow.make(0, num, 0, 9)[-8] >> 7
        assert e_of(0) == 1 and e_of(2 ** 30 + 1) == 0 and e_of(2 ** 31 - 1) == 0 and e_of(2 ** 31 - 2) == 1
    if name == "dtls12":
        assert [flow.make(w, 5, 0, 9)[3:5] for w in range(4)] == [b"\0\1", b"\0\2"] * 2 and len({flow.slot(w) for w in range(4)}) == 4


def test_loop_references_of_the_new_flows():
    """the three batches of every loop tests/test_gpu_rxwin_grid.py runs, as the reference sees them: what each must contain"""
    import rx_loop
    for name, top_bits in (("macsec", 32), ("esp", 32), ("dtls12", 48), ("srtcp_mki", 31), ("xpn", None)):
        for W in (64, 1024):
            flow, starts, (b1, b2, b3) = rx_loop.loop_reference(lib, name, W, 16)
            assert starts[0] == (2 ** 32 - 20 if name == "xpn" else 0) and len(b1.wins) == len(b3.wins) == rx_loop.N
            if top_bits:
                assert flow.top == 2 ** top_bits - 1 and b3.state[flow.top_win][0] == 2 ** top_bits and (flow.top_win, flow.top) in zip(b3.wins, b3.cnum)
            if name == "srtcp_mki":
                words = [(num, int.from_bytes(pkt[-8:-4], "big")) for b in (b1, b3) for num, pkt, y in zip(b.cnum, b.pkts, b.why) if y == R.ACCEPT]
                assert (0, 0x80000000) in words and any(wd >> 30 == 1 and num == wd for num, wd in words)


# ---------------------------------------------------------------- the kernels' assembly
@pytest.fixture(scope="module")
def census():
    return asm_census("rxwin")


def test_rxwin_kernel_set(census):
    assert {n.split("(")[0] for n in census} == {"k_rxwin_recover", "k_rxwin_max", "k_rxwin_clear", "k_rxwin_mark"}, sorted(census)


def test_rxwin_kernels_scratch_free_and_in_budget(census):
    assert_in_budget(census, body="k_kt")                                    # (no kernel here runs the AES block loop)
    for name, k in census.items():
        assert k["vgpr"] <= 32, (name, k["vgpr"])                            # a lane per packet and a handful of words: nothing here may cost occupancy


def test_rxwin_source_is_a_unit_of_its_own():
    """no other translation unit names the kernels: their censuses stay what they were"""
    others = [f for f in os.listdir(CSRC) if f.endswith("_kernels.hip") and f != "aesgcm_rxwin_kernels.hip"] + ["aesgcm_kernels.hip"]
    assert len(others) >= 8
    for f in others:
        assert "k_rxwin" not in open(os.path.join(CSRC, f)).read(), f
    assert '#include "aesgcm_rxwin_kernels.hip"' in open(os.path.join(CSRC, "aesgcm_device.hip")).read()
    assert "rxwin" in [w for ln in open(os.path.join(CSRC, "Makefile")) if ln.startswith("FAMILIES") for w in ln.split()]
    note = open(os.path.join(ROOT, "profiles", "rxwin", "isa_unchanged.txt")).read()
    assert "every instruction stream identical: yes" in note
