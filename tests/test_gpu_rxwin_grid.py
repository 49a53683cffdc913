"""GPU: the receive windows (aesgcm_rxwin_*) where tests/test_gpu_rxwin.py and the loop cases of tests/test_gpu_capture.py leave a cell out.  The reference is
tests/rxwin_ref.py (the sequential window, the recovery rules from the standards' pseudo-code) and, for packets, the family fixtures over libcrypto through
tests/rx_loop.py -- never another GPU path and never the lane code, the CPU harness's copy of it included.

  loop      recover_dev -> the family's decrypt out of place -> commit_dev with d_accept = d_auth -> wipe_failed_dev on an ordinary stream, with the library's own lane
            choice, on windows of 64 and 1024 bits, for the formats that had no loop on real packets: MACsec with the 32-bit PN, ESP without ESN, MACsec XPN at 64 bits,
            DTLS 1.2 (two epochs of a connection = two windows and two slots), SRTCP with a 4-byte MKI and E set and clear in one call.  rx_loop.loop_reference's three
            batches (fresh traffic with duplicates and forgeries; the same input again; the window's edges and a full clear), windows starting at 0, in mid-range and so
            that the last call ends at the number field's last value (2^32 - 1, 2^48 - 1, 2^31 - 1).  SRTCP: an E-clear packet whose index has bit 30 set and an E-set
            packet of index 0 are both accepted (asserted), so CLEAR_TOP alone tells them apart.
  edges     per W = 64 and 4096 one table whose windows stand at the edge values of T and one recover call per format over fields at the edge values of t: LOWEST with 2
            and 4 bytes (T either side of W, of 2^bits and of 2^bits + W, near 2^64; t at 0, 1, 2^bits - 1, B - 1, B, B + 1 and T), also against RFC 4303 A2.1's literal
            pseudo-code where its domain applies; SRTP (ROC 0, 1, 2^32 - 2, 2^32 - 1; s_l either side of 32768; SEQ around s_l +- 32768); WIRE with 2, 4, 6 and 8 bytes,
            with and without CLEAR_TOP and FROM_END, fields of all ones and all zero; EXPECT with T = 2^64 - 1.  (num, hi) per packet and the status word.  The case
            asserts that its inputs hold every refusal kind, the ROC-0 clamp and a LOWEST result in the next 2^bits period.
  big       n = 2^17 packets in one commit (512 workgroups of 256 lanes: every one of the 256 CUs holds lanes of the call) on 1 and on 64 windows of 4096 bits: every
            packet a copy of one fresh number per window (exactly one ACCEPT per window); numbers uniform in [next - 2 W, next + 2 W) with about eight copies each
            and one packet in eight not authenticated; 2^17 rising numbers in front of an empty window (the last W of a window ACCEPT, all before them OLD, the seen
            bits all ones -- on 64 windows each window gets 2^11 numbers, fewer than W: all of them ACCEPT, 2^11 seen bits).  Each call a second time: no ACCEPT,
            the state as it was.
  streams   one table of 64 windows, four rounds of two commits of 2^15 packets, the even windows' on one created stream and the odd windows' on another, enqueued back
            to back with nothing between them; each call's verdicts against the reference for its windows alone, the whole table through get, and one refused
            packet per call: the status word is (EARG, the lower of the two indices).
  perturbed the comparisons report a recovered number off by 2^bits, a hi off by one, one changed verdict, one flipped seen bit, a next off by one and two ACCEPTs
            of one number.
Every window size on the commit grid (128 .. 4096 bits, the ring's partial clear placed inside a word, on a word boundary, over three words and around the ring's end)
is tests/test_gpu_rxwin.py::test_commit_grid_against_the_sequential_window.

TIMING, measured on an MI355X (pytest --durations, the whole GPU suite in one process): the 20 cases here take 4.1 s together.  The slowest are the ones that build a
reference of 2^17 packets in Python, once per module (big_reference, stream_reference): streams 0.97 s, rising-64 0.91 s, rising-1 0.82 s, dense-64 0.42 s, dense-1
0.39 s, one-64 0.24 s, one-1 0.14 s; every loop case 0.02 s, the two edge cases and the perturbed one below 0.02 s each.  The references alone, off the GPU on a slower
host: one 0.33 / 0.82 s (1 / 64 windows), dense 0.84 / 0.82 s, rising 0.23 / 0.36 s, the eight calls of streams 1.01 s, a loop's three batches 0.05 .. 0.09 s, the edges
under 0.01 s -- so reference building, packing 2^17 values and comparing them in Python are all but the whole of every big case, and the GPU's part (six launches of 512
workgroups) is milliseconds.  None is split.  The ten cases that tests/test_gpu_rxwin.py's commit grid gains take 1.1 s together (4097-4096-3 0.34 s, the 257-packet ones
0.01 .. 0.02 s); the 70 cases of tests/test_gpu_capture.py over the moved helpers 1.1 s, as before."""
import copy
import random
import struct

import pytest

import hip_graph as G
import rxwin_ref as R
from kt_common import _u32, _u64
from rx_loop import CANARY, N, POISON, _arena, loop_reference, loop_same

pytestmark = pytest.mark.gpu


def _ints(buf, n, code):
    return list(struct.unpack("<%d%s" % (n, code), bytes(buf.download(n * struct.calcsize("<" + code)))))


def _set(rw, sets):
    rw.set(0, [s[1] for s in sets], [s[2] for s in sets])


# ---------------------------------------------------------------- A: the receive loop on an ordinary stream
LOOPS = [("macsec", 64, 16), ("macsec", 1024, 24), ("esp", 64, 32), ("esp", 1024, 16), ("xpn", 64, 24), ("xpn", 1024, 32), ("dtls12", 64, 16), ("dtls12", 1024, 24),
         ("srtcp_mki", 64, 32), ("srtcp_mki", 1024, 16)]


def _decrypt(hip, flow, kt, n, p):
    if flow.name in ("macsec", "esp"):
        kt.frames_crypt_dev(1, flow.wf, n, p("slots"), p("in"), p("off"), p("out"), d_auth=p("auth"))
    elif flow.name == "xpn":
        kt.frames_crypt_x_dev(1, flow.wf, n, p("slots"), p("hi"), p("in"), p("off"), p("out"), d_auth=p("auth"))
    elif flow.name == "dtls12":
        kt.dtls_crypt_dev(1, hip.DtlsFormat.dtls12(), n, p("slots"), p("in"), p("off"), p("out"), d_auth=p("auth"))
    else:
        kt.srtp_crypt_dev(1, hip.SrtpFormat.rtcp(4), n, p("slots"), p("in"), p("off"), p("out"), d_auth=p("auth"))


def run_plain(hip, name, W, key_len):
    """the three batches behind one another on the null stream -> (flow, batches, what each left, the arena's size, label)"""
    flow, starts, batches = loop_reference(hip, name, W, key_len)
    n, size = N, max(b.off[-1] for b in batches) + 64
    label = "receive loop %s W=%d" % (name, W)
    kt, rw = flow.table(hip), hip.RxWindows(flow.n_wins, W)
    B = {k: hip.DeviceBuffer(nb) for k, nb in dict(win=4 * n, slots=4 * n, off=8 * (n + 1), num=8 * n, hi=4 * n, auth=4 * n, why=4 * n).items()}
    B["in"], B["out"] = hip.DeviceBuffer(size), hip.DeviceBuffer(size)
    p = lambda k: B[k].ptr
    got = []
    try:
        rw.set(0, starts)
        for b in batches:
            B["win"].upload(_u32(b.wins)); B["slots"].upload(_u32([flow.slot(w) for w in b.wins])); B["off"].upload(_u64(b.off))
            B["in"].upload(_arena(b.pkts, b.lead, size)); B["out"].upload(bytes([CANARY]) * size)
            for k in ("num", "hi", "auth", "why"):
                B[k].upload(bytes([POISON]) * B[k].nbytes)
            rw.recover_dev(flow.fmt, n, p("win"), p("in"), p("off"), p("num"), p("hi"))
            _decrypt(hip, flow, kt, n, p)
            rw.commit_dev(n, p("win"), p("num"), p("auth"), p("auth"), p("why"))
            hip.wipe_failed_dev(n, p("out"), p("auth"), d_data_off=p("off"))
            hip.dev_sync()
            got.append(dict(num=_ints(B["num"], n, "Q"), hi=_ints(B["hi"], n, "I"), why=_ints(B["why"], n, "i"), accept=_ints(B["auth"], n, "i"), out=bytes(B["out"].download()),
                            state=rw.get(), status=(rw.status(), kt.status())))
    finally:
        kt.close(); rw.close()
        for x in B.values():
            x.free()
    return flow, batches, got, size, label


@pytest.mark.parametrize("name, W, key_len", LOOPS)
def test_receive_loop_for_the_formats_without_one(hip, name, W, key_len):
    flow, batches, got, size, label = run_plain(hip, name, W, key_len)
    for k, (b, g) in enumerate(zip(batches, got)):
        loop_same(hip, flow, b, g, size, "%s, batch %d" % (label, k + 1))
    assert set(got[1]["out"][batches[1].lead:batches[1].off[-1]]) == {0}          # the same input again: every output byte zero
    assert got[1]["state"] == got[0]["state"] and got[2]["state"] != got[1]["state"]
    if flow.top_win is not None:
        assert got[2]["state"][0][flow.top_win] == flow.top + 1                   # the last call ended at the field's last number
    accepted = [(b.wins[i], b.cnum[i], b.pkts[i]) for b, g in zip(batches, got) for i in range(N) if g["why"][i] == R.ACCEPT]
    if name == "dtls12":
        assert {(w & 1, int.from_bytes(pkt[3:5], "big")) for w, _, pkt in accepted} == {(0, 1), (1, 2)}      # a window per epoch
    if name == "srtcp_mki":
        words = [(num, int.from_bytes(pkt[-8:-4], "big")) for _, num, pkt in accepted]
        assert (0, 0x80000000) in words, "an E-set packet of index 0"
        assert any(wd >> 30 == 1 and num == wd for num, wd in words), "an E-clear packet whose index has bit 30 set"
        assert (2 ** 31 - 1, 0x7FFFFFFF) in words, "the last index, E clear"


# ---------------------------------------------------------------- B: the recovery rules at their edges
def edge_cases(W):
    """-> (nexts, [(fmt, [(window, packet or None)])]): the table's windows stand at every T any format asks for; one list of packets per format"""
    nexts = []

    def win(T):
        if T not in nexts:
            nexts.append(T)
        return nexts.index(T)

    cases = []
    for num_len, num_off in ((2, 1), (4, 4)):
        bits = 8 * num_len
        m = 1 << bits
        items = []
        for T in (0, 1, W - 1, W, W + 1, m - 1, m, m + W - 1, m + W, m + W + 1, 2 ** 64 - m + W, 2 ** 64 - 2, 2 ** 64 - 1):
            B = max(T - W, 0)
            for t in sorted({0, 1, m - 1, (B - 1) % m, B % m, (B + 1) % m, T % m}):
                items.append((win(T), bytes([0xE0 + k for k in range(num_off)]) + t.to_bytes(num_len, "big") + b"\xEE\xEF\xF0"))
        cases.append(((R.LOWEST, num_off, num_len, 0), items))
    items = [(win(0), b"\x80\x60" + seq.to_bytes(2, "big") + b"\x01\x02") for seq in (0, 32769, 65535)]
    for ROC in (0, 1, 2 ** 32 - 2, 2 ** 32 - 1):
        for s_l in (0, 1, 32767, 32768, 32769, 65535):
            T = (ROC << 16 | s_l) + 1
            for seq in sorted({x for c in (s_l + 32768, s_l - 32768) for x in (c - 1, c, c + 1) if 0 <= x <= 65535} | {0, 65535}):
                items.append((win(T), b"\x80\x60" + seq.to_bytes(2, "big") + b"\x01\x02"))
    cases.append(((R.SRTP, 2, 2, 0), items))
    rng = random.Random("edges %d" % W)
    for num_len in (2, 4, 6, 8):
        for flags in (0, R.CLEAR_TOP, R.FROM_END, R.FROM_END | R.CLEAR_TOP):
            num_off = num_len + 2 if flags & R.FROM_END else 3
            items = []
            for field in (b"\xff" * num_len, bytes(num_len), b"\x80" + bytes(num_len - 1), b"\x7f" + b"\xff" * (num_len - 1), bytes(rng.randrange(256) for _ in range(num_len))):
                pkt = b"\x11\x22\x33\x44\x55" + field + b"\x66\x77" if flags & R.FROM_END else b"\x11\x22\x33" + field + b"\x44"
                items.append((rng.randrange(len(nexts)), pkt))
            cases.append(((R.WIRE, num_off, num_len, flags), items))
    cases.append(((R.EXPECT, 0, 0, 0), [(w, None) for w in range(len(nexts))]))
    return nexts, cases


def edge_reference(W):
    """what rxwin_ref makes of edge_cases(W): -> (nexts, [(fmt, wins, data, offs, [(num, hi)], lowest refused index or None)]); asserts that the inputs hold what they claim"""
    nexts, cases = edge_cases(W)
    out, seen = [], set()
    for fmt, items in cases:
        rule, num_off, num_len, flags = fmt
        wins = [w for w, _ in items]
        offs = [7]
        for _, pkt in items:
            offs.append(offs[-1] + len(pkt or b""))
        data = bytes(7) + b"".join(pkt or b"" for _, pkt in items)
        want, bad = R.recover(fmt, len(nexts), W, nexts, wins, data, offs)
        bits = 8 * num_len
        for (w, pkt), (num, hi) in zip(items, want):
            T = nexts[w]
            if rule == R.LOWEST:
                t = int.from_bytes(pkt[num_off:num_off + num_len], "big")
                full, B = R.lowest(T, W, t, bits), max(T - W, 0)
                seen.add("lowest refused" if full >= R.NONE else "lowest in the next period" if full >> bits == (B >> bits) + 1 else "lowest")
                assert (num, hi) == ((full, (full >> bits) & 0xFFFFFFFF) if full < R.NONE else (R.NONE, 0xFFFFFFFF))
                if bits == 32 and T >= 1 and T - 1 >= W - 1:                     # the RFC's domain: its literal pseudo-code says the same
                    Seqh = R.rfc4303_a21((T - 1) >> 32, (T - 1) & 0xFFFFFFFF, W, t)
                    rfc = Seqh << 32 | t
                    assert Seqh >= 0 and (num, hi) == ((rfc, Seqh) if rfc < R.NONE else (R.NONE, 0xFFFFFFFF)), (T, W, t)
                    seen.add("rfc4303")
            elif rule == R.SRTP:
                seq = int.from_bytes(pkt[2:4], "big")
                v = R.srtp_v(T, seq)
                if v > 0xFFFFFFFF:
                    seen.add("roc past 2^32 - 1")
                    assert num == R.NONE
                elif T and (T - 1) >> 16 == 0 and (T - 1) & 0xFFFF < 32768 and seq - ((T - 1) & 0xFFFF) > 32768:
                    seen.add("roc 0 clamp")
                    assert (num, hi) == (seq, 0)
                if T and 0 < (T - 1) >> 16 < 2 ** 32 - 1:                        # away from both ends the header's rule is RFC 3711 Appendix A's
                    assert hi == R.rfc3711_index((T - 1) & 0xFFFF, (T - 1) >> 16, seq)
                    seen.add("rfc3711")
            elif rule == R.WIRE:
                if num_len == 8 and pkt.count(0xff) >= 8:
                    seen.add("wire all ones" + (" cleared" if flags & R.CLEAR_TOP else ""))
                    assert num == (2 ** 63 - 1 if flags & R.CLEAR_TOP else R.NONE)
            elif T == R.NONE:
                seen.add("expect none")
                assert num == R.NONE
        out.append((fmt, wins, data, offs, want, bad))
    assert seen >= {"lowest refused", "lowest in the next period", "lowest", "rfc4303", "roc past 2^32 - 1", "roc 0 clamp", "rfc3711", "wire all ones", "wire all ones cleared",
                    "expect none"}, seen
    return nexts, out


def recover_same(got, status, want, bad, hip, label):
    for p, (g, w) in enumerate(zip(got, want)):
        assert g[0] == w[0], (label, "packet %d: number %d, want %d" % (p, g[0], w[0]))
        assert g[1] == w[1], (label, "packet %d: hi %d, want %d" % (p, g[1], w[1]))
    assert len(got) == len(want)
    assert status == ((hip.EARG, bad) if bad is not None else (hip.OK, 0)), (label, status, bad)


def run_edges(hip, W):
    nexts, cases = edge_reference(W)
    got = []
    with hip.RxWindows(len(nexts), W) as rw:
        rw.set(0, nexts)
        for fmt, wins, data, offs, want, bad in cases:
            n = len(wins)
            bufs = [hip.DeviceBuffer(max(len(x), 16)) for x in (_u32(wins), data, _u64(offs), bytes(8 * n), bytes(4 * n))]
            d_win, d_in, d_off, d_num, d_hi = bufs
            try:
                d_win.upload(_u32(wins)); d_in.upload(data); d_off.upload(_u64(offs)); d_num.upload(bytes([POISON]) * 8 * n); d_hi.upload(bytes([POISON]) * 4 * n)
                expect = fmt[0] == R.EXPECT
                rw.recover_dev(hip.RxFormat(*fmt), n, d_win.ptr, None if expect else d_in.ptr, None if expect else d_off.ptr, d_num.ptr, d_hi.ptr)
                hip.dev_sync()
                got.append((list(zip(_ints(d_num, n, "Q"), _ints(d_hi, n, "I"))), rw.status()))
            finally:
                for b in bufs:
                    b.free()
        assert rw.get()[0] == nexts                                              # recover changes no window
    return cases, got


@pytest.mark.parametrize("W", [64, 4096])
def test_recovery_rules_at_their_edges(hip, W):
    cases, got = run_edges(hip, W)
    assert len(cases) == 2 + 1 + 16 + 1
    for (fmt, wins, data, offs, want, bad), (g, status) in zip(cases, got):
        assert hip.RxFormat(*fmt).check() == hip.OK
        recover_same(g, status, want, bad, hip, "W=%d format %r" % (W, fmt))


# ---------------------------------------------------------------- D: calls that fill the chip
BIG_N, BIG_W = 2 ** 17, 4096
_BIG = {}


def big_reference(kind, n_wins, n=BIG_N, W=BIG_W):
    """-> (sets, wins, nums, auths, [(why, state) of the first and of the second issue]); built once per module"""
    if (kind, n_wins, n) in _BIG:
        return _BIG[kind, n_wins, n]
    rng = random.Random("big %s %d %d" % (kind, n_wins, n))
    if kind == "one":
        sets = [(w, 3 * W + 1000 * w, rng.getrandbits(W)) for w in range(n_wins)]
        wins = [rng.randrange(n_wins) for _ in range(n)]
        wins[:n_wins] = range(n_wins)
        nums = [sets[w][1] + 17 + w for w in wins]
        auths = [1] * n
    elif kind == "dense":
        sets = [(w, 10 ** 6 * (w + 1), rng.getrandbits(W)) for w in range(n_wins)]
        pool = [rng.sample(range(s[1] - 2 * W, s[1] + 2 * W), min(4 * W, n // (8 * n_wins))) for s in sets]
        wins = [rng.randrange(n_wins) for _ in range(n)]
        nums = [rng.choice(pool[w]) for w in wins]
        auths = [1 if rng.randrange(8) else 0 for _ in range(n)]
    else:
        assert kind == "rising" and n % n_wins == 0
        sets = [(w, 2 ** 32 - 50 + 2 ** 20 * w, 0) for w in range(n_wins)]
        wins = [p % n_wins for p in range(n)]
        nums = [sets[p % n_wins][1] + p // n_wins for p in range(n)]
        auths = [1] * n
    windows = {w: R.Window.from_normalised(W, nx, seen) for w, nx, seen in sets}
    issues = []
    for _ in range(2):
        why = R.commit(windows, wins, nums, auths)
        issues.append((why, [windows[w].normalised() for w in range(n_wins)]))
    (why1, state1), (why2, state2) = issues
    assert state2 == state1 and R.ACCEPT not in why2 and [y == R.NOAUTH for y in why2] == [a == 0 for a in auths]
    per = [[] for _ in range(n_wins)]
    for p, w in enumerate(wins):
        per[w].append(p)
    if kind == "one":
        assert all([why1[p] for p in ps].count(R.ACCEPT) == 1 and {why1[p] for p in ps} == {R.ACCEPT, R.REPLAY} for ps in per)
        assert [s[0] for s in state1] == [sets[w][1] + 18 + w for w in range(n_wins)]
    elif kind == "dense":
        copies = n / len({(w, x) for w, x in zip(wins, nums)})
        assert 7 <= copies <= 9 and {R.NOAUTH, R.ACCEPT, R.OLD, R.REPLAY} == set(why1), copies
    else:
        for w, ps in enumerate(per):
            keep = min(W, len(ps))
            assert [why1[p] for p in ps] == [R.OLD] * (len(ps) - keep) + [R.ACCEPT] * keep
            assert state1[w] == (nums[ps[-1]] + 1, (1 << keep) - 1)
    _BIG[kind, n_wins, n] = (sets, wins, nums, auths, issues)
    return _BIG[kind, n_wins, n]


def commit_same(wins, nums, accept, why, state, want_why, want_state, label):
    """one commit's d_accept, d_why and the table through get against the reference"""
    assert accept == [1 if y == R.ACCEPT else 0 for y in why], (label, "d_accept")
    err = R.same_verdicts(wins, nums, why, want_why)
    assert err is None, (label, "d_why", err)
    for w, (nx, seen) in enumerate(want_state):
        assert state[0][w] == nx, (label, "window %d: next %d, want %d" % (w, state[0][w], nx))
        assert state[1][w] == seen, (label, "window %d: seen bits differ at %s" % (w, [i for i in range(seen.bit_length() + 1) if (state[1][w] ^ seen) >> i & 1][:4]))
    assert len(state[0]) == len(want_state)


@pytest.mark.parametrize("n_wins", [1, 64])
@pytest.mark.parametrize("kind", ["one", "dense", "rising"])
def test_a_call_that_fills_the_chip(hip, kind, n_wins):
    sets, wins, nums, auths, issues = big_reference(kind, n_wins)
    assert len(wins) == 2 ** 17
    with hip.RxWindows(n_wins, BIG_W) as rw:
        _set(rw, sets)
        for k, (want_why, want_state) in enumerate(issues):
            accept, why = rw.commit(wins, nums, auths)
            commit_same(wins, nums, accept, why, rw.get(), want_why, want_state, "%s on %d windows, issue %d" % (kind, n_wins, k + 1))
            assert rw.status() == (hip.OK, 0)
            if k == 0 and kind == "one":
                assert sum(accept) == n_wins
            if k == 1:
                assert sum(accept) == 0


ROUNDS, STREAM_N = 4, 2 ** 15
_STREAMS = {}


def stream_reference(n_wins=64, W=BIG_W, n=STREAM_N):
    """-> (sets, [[(wins, nums, auths, why, index of the refused packet) for the even and for the odd windows], the whole table's state] per round)"""
    if not _STREAMS:
        rng = random.Random("two streams")
        sets = [(w, 5 * W + 999 * w, rng.getrandbits(W)) for w in range(n_wins)]
        windows = {w: R.Window.from_normalised(W, nx, seen) for w, nx, seen in sets}
        rounds = []
        for k in range(ROUNDS):
            calls = []
            for half in (0, 1):
                wins = [2 * rng.randrange(n_wins // 2) + half for _ in range(n)]
                nums = [max(windows[w].next + rng.randrange(-W - W // 2, W), 0) for w in wins]
                auths = [1 if rng.randrange(8) else 0 for _ in range(n)]
                bad = rng.randrange(100 + 1000 * half, n)
                wins[bad], nums[bad], auths[bad] = (n_wins, 5, 1) if (k + half) % 2 else (wins[bad], R.NONE, 1)
                mine = {w: windows[w] for w in range(half, n_wins, 2)}           # the reference run for this call's windows alone
                why = R.commit(mine, wins, nums, auths)
                assert [p for p, y in enumerate(why) if y == R.REFUSED] == [bad] and {R.ACCEPT, R.OLD, R.REPLAY, R.NOAUTH} <= set(why)
                calls.append((wins, nums, auths, why, bad))
            rounds.append((calls, [windows[w].normalised() for w in range(n_wins)]))
        _STREAMS["ref"] = (sets, rounds)
    return _STREAMS["ref"]


def test_two_streams_on_different_windows_of_one_table(hip):
    sets, rounds = stream_reference()
    n, n_wins = STREAM_N, len(sets)
    with hip.RxWindows(n_wins, BIG_W) as rw:
        _set(rw, sets)
        B = [{k: hip.DeviceBuffer(nb) for k, nb in dict(win=4 * n, num=8 * n, auth=4 * n, accept=4 * n, why=4 * n).items()} for _ in (0, 1)]
        streams = [G.stream_create(), G.stream_create()]
        try:
            for k, (calls, want_state) in enumerate(rounds):
                for b, (wins, nums, auths, _, _) in zip(B, calls):
                    b["win"].upload(_u32(wins)); b["num"].upload(_u64(nums)); b["auth"].upload(struct.pack("<%di" % n, *auths))
                    b["accept"].upload(bytes([POISON]) * 4 * n); b["why"].upload(bytes([POISON]) * 4 * n)
                hip.dev_sync()
                for b, st in zip(B, streams):                                    # back to back, nothing between them
                    rw.commit_dev(n, b["win"].ptr, b["num"].ptr, b["auth"].ptr, b["accept"].ptr, b["why"].ptr, stream=st)
                for st in streams:
                    G.synchronize(st)
                state = rw.get()
                for half, (b, (wins, nums, auths, why, bad)) in enumerate(zip(B, calls)):
                    mine = range(half, n_wins, 2)
                    commit_same(wins, nums, _ints(b["accept"], n, "i"), _ints(b["why"], n, "i"), ([state[0][w] for w in mine], [state[1][w] for w in mine]), why,
                                [want_state[w] for w in mine], "round %d, %s windows" % (k + 1, ("even", "odd")[half]))
                assert state == ([s[0] for s in want_state], [s[1] for s in want_state]), k
                assert rw.status() == (hip.EARG, min(c[4] for c in calls)) and rw.status() == (hip.OK, 0)
        finally:
            if not G.BROKEN:
                for st in streams:
                    G.stream_destroy(st)
            for b in B:
                for x in b.values():
                    x.free()


# ---------------------------------------------------------------- the comparisons themselves
def test_perturbed_references_are_reported(hip):
    """loop_same, recover_same and commit_same fail when the reference is wrong by 2^bits in a recovered number, by one in a hi, in one verdict, in one seen bit, by one in
    a next, and when one number is accepted twice"""
    flow, batches, got, size, label = run_plain(hip, "xpn", 64, 24)
    i = batches[0].why.index(R.ACCEPT)
    for what, change in (("a recovered number", lambda b: b.rec.__setitem__(4, (b.rec[4][0] + 2 ** 32, b.rec[4][1]))), ("a hi", lambda b: b.rec.__setitem__(4, (b.rec[4][0], b.rec[4][1] + 1))),
                         ("a verdict", lambda b: b.why.__setitem__(i, R.REPLAY)), ("a seen bit", lambda b: b.state.__setitem__(1, (b.state[1][0], b.state[1][1] ^ 2))),
                         ("a next", lambda b: b.state.__setitem__(1, (b.state[1][0] + 1, b.state[1][1] << 1)))):
        b = copy.deepcopy(batches[0])
        change(b)
        with pytest.raises(AssertionError):
            loop_same(hip, flow, b, got[0], size, what)
    loop_same(hip, flow, batches[0], got[0], size, "batch 1")
    with pytest.raises(AssertionError):
        loop_same(hip, flow, batches[0], got[1], size, "batch 2 against batch 1's reference")

    cases, rgot = run_edges(hip, 64)
    fmt, wins, data, offs, want, bad = cases[1]                                  # LOWEST, 4 bytes
    g, status = rgot[1]
    recover_same(g, status, want, bad, hip, "edges")
    p = next(p for p, w in enumerate(want) if w[0] != R.NONE)
    for what, w in (("a number", (want[p][0] + 2 ** 32, want[p][1])), ("a hi", (want[p][0], want[p][1] + 1))):
        with pytest.raises(AssertionError):
            recover_same(g, status, want[:p] + [w] + want[p + 1:], bad, hip, what)
    with pytest.raises(AssertionError):
        recover_same(g, status, want, None, hip, "the status word")

    sets, calls = R.ring_sequence(random.Random("perturbed"), 3, 128, 257)
    with hip.RxWindows(3, 128) as rw:
        _set(rw, sets)
        for wins, nums, auths, why, state, _ in calls[:2]:
            accept, gwhy = rw.commit(wins, nums, auths)
            gstate = rw.get()
    args = lambda **kw: dict(dict(wins=wins, nums=nums, accept=accept, why=gwhy, state=gstate, want_why=list(why), want_state=list(state), label="commit"), **kw)
    commit_same(**args())
    i = why.index(R.ACCEPT)
    flipped = list(why)
    flipped[i] = R.REPLAY
    nx, seen = state[1]
    for kw in (dict(want_why=flipped), dict(want_state=[state[0], (nx, seen ^ 1 << 70), state[2]]), dict(want_state=[state[0], (nx + 1, seen << 1 & (1 << 128) - 1), state[2]]),
               dict(want_state=[state[0], (nx + 1, seen), state[2]])):
        with pytest.raises(AssertionError):
            commit_same(**args(**kw))
    # two ACCEPTs of one number, in what the device said and in the reference alike: still reported
    groups = {}
    for p, key in enumerate(zip(wins, nums)):
        groups.setdefault(key, []).append(p)
    ps = next(ps for ps in groups.values() if sorted(why[p] for p in ps)[:2] == [R.ACCEPT, R.REPLAY])
    twice_got, twice_want = list(gwhy), list(why)
    twice_got[next(p for p in ps if gwhy[p] == R.REPLAY)] = R.ACCEPT
    twice_want[next(p for p in ps if why[p] == R.REPLAY)] = R.ACCEPT
    assert "accepted 2 times" in R.same_verdicts(wins, nums, twice_got, twice_want)
    with pytest.raises(AssertionError):
        commit_same(**args(why=twice_got, accept=[1 if y == R.ACCEPT else 0 for y in twice_got], want_why=twice_want))
