"""GPU: send counters (aesgcm_txnum_*) -- packet numbers handed out on the device, in packet order.  The reference is tests/txnum_ref.py: a dict of counters walked
in array order.  Every output array lies between guards and every byte of the packet buffer, canaries included, is compared.
  populations  1 .. 70 001 packets (one wave, a tile, a slice, several tiles per slice with a ragged last slice) all on one counter, on 3 interleaved, each on its own,
               on 255 / 256 / 257 / 65 537 counters (one, two and three digit passes; counter numbers that differ only in a high digit), in runs that straddle tile and
               slice boundaries, with out-of-range counter numbers sprinkled in; two calls, the second continues the first
  limits       a limit crossed in the middle of a tile, a fresh table, argument errors that need a table
  formats      every preset's field write; SRTCP keeps E, DTLS 1.2 writes both places
  end to end   XPN and ESN across 2^32: assign -> encrypt -> recover -> decrypt -> commit; classic MACsec refuses past 2^32 - 1; a TLS 1.3 leg
  capture      assign + encrypt in one graph, replayed over changed counters"""
import random
import struct

import pytest

import hip_graph as G
import rxwin_ref as RX
import tls_fixture as T
import txnum_ref as R
from kt_common import Guarded, Sa, _layout, _u32, _u64, _up, evp, tls_ref_encrypt, wire_ref_encrypt, x_ref_encrypt  # noqa: F401
from util import splitmix_bytes

pytestmark = pytest.mark.gpu

COUNTS = [1, 63, 64, 65, 255, 256, 257, 4097, 70001]
U32 = 0xFFFFFFFF


def _assign(hip, tc, fmt, ctrs, pkts=None, slots=None, label=""):
    """one assign_dev on guarded arrays -> (nums, his, slots afterwards, the whole packet buffer afterwards, its offsets, the buffer before)"""
    n = len(ctrs)
    num, hi, sl = Guarded(hip, 8 * n), Guarded(hip, 4 * n), Guarded(hip, 4 * n)
    sl.buf.upload(bytes([0xA7]) * (sl.ptr - sl.buf.ptr) + _u32(slots if slots is not None else [7] * n))
    d_ctr = _up(hip, _u32(ctrs))
    off, buf = _layout(pkts, 5) if pkts is not None else (None, b"")
    d_off, d_buf = (_up(hip, _u64(off)), _up(hip, buf)) if pkts is not None else (None, None)
    try:
        tc.assign_dev(fmt, n, d_ctr.ptr, d_buf.ptr if d_buf else None, d_off.ptr if d_off else None, num.ptr, hi.ptr, sl.ptr)
        hip.dev_sync()
        out = bytes(d_buf.download(len(buf))) if d_buf else b""
        return (list(struct.unpack("<%dQ" % n, num.read(label))), list(struct.unpack("<%dI" % n, hi.read(label))), list(struct.unpack("<%dI" % n, sl.read(label))), out, off, buf)
    finally:
        for b in (num.buf, hi.buf, sl.buf, d_ctr, d_off, d_buf):
            if b is not None:
                b.free()


def _check_call(hip, tc, fmt, counters, ctrs, pkts, label):
    """a call against the reference: every array, every byte, the status word, the counters afterwards"""
    tup = (fmt.num_off, fmt.num_len, fmt.dup_off, fmt.flags)
    got_num, got_hi, got_sl, out, off, buf = _assign(hip, tc, fmt, ctrs, pkts, label=label)
    nums, his, refused, want, bad = R.assign(tup, counters, ctrs, buf, off)
    assert got_num == nums, (label, [(i, g, w) for i, (g, w) in enumerate(zip(got_num, nums)) if g != w][:5])
    assert got_hi == [h & U32 for h in his] and got_sl == [U32 if r else 7 for r in refused], label
    assert out == want, (label, "packet bytes")
    assert tc.status() == ((hip.EARG, bad) if bad is not None else (hip.OK, 0)), label
    return nums, refused


def _population(kind, n, rng):
    """-> (n_ctrs, counter per packet)"""
    if kind == "one":
        return 1, [0] * n
    if kind == "three":
        return 3, [i % 3 for i in range(n)]
    if kind == "own":
        c = list(range(n))
        rng.shuffle(c)
        return n, c
    if kind == "runs":                                                        # runs of 1 .. 700 packets of one counter: they straddle tiles (256) and slices (n / 256)
        c = []
        while len(c) < n:
            c += [rng.randrange(5)] * rng.randrange(1, 701)
        return 5, c[:n]
    n_ctrs = int(kind)
    # counter numbers that differ only in one digit, the highest included, among random ones
    special = [x for x in (0, 1, 255, 256, 257, 511, 65535, 65536, 65280, 254, n_ctrs - 1) if x < n_ctrs]
    return n_ctrs, [rng.choice(special) if rng.randrange(2) else rng.randrange(n_ctrs) for _ in range(n)]


@pytest.mark.parametrize("kind", ["one", "three", "own", "runs", "255", "256", "257", "65537"])
@pytest.mark.parametrize("n", COUNTS)
def test_numbers_follow_array_order(hip, kind, n):
    rng = random.Random("pop %s %d" % (kind, n))
    n_ctrs, ctrs = _population(kind, n, rng)
    for k in range(rng.randrange(41), n, 41):
        ctrs[k] = rng.choice((n_ctrs, n_ctrs + k, U32, 2 ** 31))              # out of range, sprinkled in
    fmt = hip.TxFormat.esp_esn()
    used = sorted({c for c in ctrs if c < n_ctrs})
    counters = {c: [rng.choice((0, 2 ** 32 - 40, rng.randrange(2 ** 48))), 2 ** 63] for c in used}
    with hip.TxCounters(n_ctrs, 70001) as tc:
        assert tc.get(0, min(n_ctrs, 3)) == ([0] * min(n_ctrs, 3), [0] * min(n_ctrs, 3))
        tc.set(0, [counters.get(c, (0, 0))[0] for c in range(n_ctrs)], [counters.get(c, (0, 0))[1] for c in range(n_ctrs)])
        for call in range(2):                                                 # the second call continues where the first stopped
            pkts = [bytes([rng.randrange(256)]) * (8 + (i + call) % 3) for i in range(n)]
            _check_call(hip, tc, fmt, counters, ctrs, pkts, (kind, n, call))
            ctrs = ctrs[n // 2:] + ctrs[:n // 2]
        probe = used[:3] + used[-3:]
        assert [tc.get(c, 1) for c in probe] == [([counters[c][0]], [counters[c][1]]) for c in probe]


def test_a_limit_crossed_in_the_middle_of_a_tile_and_a_fresh_table(hip):
    fmt = hip.TxFormat.macsec_xpn()
    pkts = [bytes([i & 0xFF]) * 24 for i in range(300)]
    with hip.TxCounters(2, 300) as tc:
        # a fresh table refuses everything and writes nothing
        counters = {0: [0, 0], 1: [0, 0]}
        nums, refused = _check_call(hip, tc, fmt, counters, [i % 2 for i in range(300)], pkts, "fresh")
        assert all(refused) and tc.get() == ([0, 0], [0, 0])
        tc.set(0, [100], [230])
        counters[0] = [100, 230]
        nums, refused = _check_call(hip, tc, fmt, counters, [0] * 300, pkts, "limit")
        assert nums[:130] == list(range(100, 230)) and refused == [False] * 130 + [True] * 170       # (status = 130 and the untouched bytes: _check_call)
        assert tc.get() == ([230, 0], [230, 0])
        nums, refused = _check_call(hip, tc, fmt, counters, [0, 1, 0], pkts[:3], "after the limit")
        assert all(refused) and tc.get() == ([230, 0], [230, 0])
        # what is read off a table
        L = tc._lib
        one, two = (hip.u64 * 1)(5), (hip.u64 * 1)(4)
        assert L.aesgcm_txnum_set(tc._h, 0, 1, one, two, None) == hip.EARG and L.aesgcm_txnum_set(tc._h, 2, 1, two, one, None) == hip.EARG       # next > limit; out of range
        assert L.aesgcm_txnum_set(tc._h, 1, 2, two, one, None) == hip.EARG
        P = 16
        assert L.aesgcm_txnum_assign_dev(tc._h, fmt, 301, P, P, P, P, P, P, None) == hip.EARG                                                   # n_pkts > max_pkts
        assert tc.get() == ([230, 0], [230, 0])


@pytest.mark.parametrize("name", sorted(R.FORMATS))
def test_every_format_s_field_write(hip, name):
    rng = random.Random("fmt " + name)
    tup = R.FORMATS[name]
    fmt = hip.TxFormat(*tup)
    bits = 8 * tup[1] - (1 if tup[3] & R.KEEP_TOP else 0)
    top = (1 << bits) if tup[3] & R.WHOLE else 2 ** 63
    counters = {0: [0, 2 ** 64 - 1], 1: [max(top - 20, 0), 2 ** 64 - 1], 2: [2 ** 32 - 7, 2 ** 32 + 9]}
    n = 90
    pkts = [bytes(rng.randrange(256) for _ in range(rng.randrange(0, 64))) for _ in range(n - 2)] + [b"\x80" * 40, b"\x7f" * 40]
    ctrs = [rng.randrange(3) for _ in range(n)]
    with hip.TxCounters(3, n) as tc:
        tc.set(0, [counters[c][0] for c in range(3)], [counters[c][1] for c in range(3)])
        tup_before = [list(v) for v in counters.values()]
        nums, refused = _check_call(hip, tc, fmt, counters, ctrs, pkts if tup[1] else None, name)
        assert refused.count(False) >= 20 and (not tup[1] or refused.count(True) >= 5), name
        assert tc.get() == ([counters[c][0] for c in range(3)], [counters[c][1] for c in range(3)]) and tup_before != [list(v) for v in counters.values()]
    if name.startswith("srtcp") or name == "dtls12":                          # what the reference did, said once more on the last two packets
        c2 = {0: [5, 9]}
        _, _, _, out, _ = R.assign(tup, c2, [0, 0], pkts[-2] + pkts[-1], [0, 40, 80])
        if name == "dtls12":
            assert out[5:11] == out[15:21] == (5).to_bytes(6, "big") and out[45:51] == out[55:61] == (6).to_bytes(6, "big")
        else:
            at = 40 - tup[0]
            assert out[at:at + 4] == b"\x80\x00\x00\x05" and out[40 + at:44 + at] == b"\x00\x00\x00\x06"        # E kept set, E kept clear


# ---------------------------------------------------------------- end to end
@pytest.mark.parametrize("ext", ["esn", "xpn"])
def test_send_loop_across_2_32_is_accepted_in_order(hip, evp, ext):  # noqa: F811
    rng = random.Random("tx e2e " + ext)
    key_len, n_sa, W, n = 32, 3, 1024, 120
    xf = hip.WireFormatX.esp_esn(16) if ext == "esn" else hip.WireFormatX.macsec_xpn()
    tf = hip.TxFormat.esp_esn() if ext == "esn" else hip.TxFormat.macsec_xpn()
    rf = hip.RxFormat.esp_esn() if ext == "esn" else hip.RxFormat.macsec_xpn()
    keys, sa = splitmix_bytes(0x7F00, key_len * n_sa), Sa(n_sa, 0x7F01)
    slots = [rng.randrange(n_sa) for _ in range(n)]
    plain = [splitmix_bytes(0x7F10 + p, xf.f.hdr_len + rng.randrange(0, 200)) + b"\xAA" * 16 for p in range(n)]
    off, buf = _layout(plain, 5)
    start = 2 ** 32 - 5
    with hip.KeyTable(key_len, n_sa) as kt, hip.TxCounters(n_sa, n) as tc, hip.RxWindows(n_sa, W) as rw:
        kt.set(0, keys).set_salt(0, b"".join(sa.salt)).set_xpn(0, b"".join(sa.xsalt), b"".join(sa.ssci))
        tc.set(0, [start] * n_sa, [2 ** 64 - 1] * n_sa)
        rw.set(0, [start] * n_sa)
        d = {k: _up(hip, v) for k, v in (("ctr", _u32(slots)), ("slots", _u32(slots)), ("off", _u64(off)), ("buf", buf), ("num", bytes(8 * n)), ("hi", bytes(4 * n)), ("rnum", bytes(8 * n)),
                                         ("rhi", bytes(4 * n)), ("auth", b"\x07" * 4 * n), ("why", b"\x07" * 4 * n))}
        p = lambda k: d[k].ptr
        # the sender: numbers, then the encrypt under them
        tc.assign_dev(tf, n, p("ctr"), p("buf"), p("off"), p("num"), p("hi"), p("slots"))
        kt.frames_crypt_x_dev(0, xf, n, p("slots"), p("hi"), p("buf"), p("off"), p("buf"))
        hip.dev_sync()
        nums = list(struct.unpack("<%dQ" % n, bytes(d["num"].download(8 * n))))
        seen = {s: start for s in range(n_sa)}
        for s, x in zip(slots, nums):                                         # ascending in array order per association, from 2^32 - 5 across 2^32
            assert x == seen[s]
            seen[s] += 1
        assert max(nums) > 2 ** 32 + 20 and tc.status() == (hip.OK, 0) and kt.status() == (hip.OK, 0)
        assert list(struct.unpack("<%dI" % n, bytes(d["slots"].download(4 * n)))) == slots
        at = xf.f.iv_off if ext == "xpn" else 4
        numbered = [f[:at] + struct.pack(">I", x & U32) + f[at + 4:] for f, x in zip(plain, nums)]
        wire = x_ref_encrypt(evp, key_len, keys, sa, xf, slots, [x >> 32 for x in nums], numbered)
        assert bytes(d["buf"].download(len(buf))) == _layout(wire, 5)[1]      # libcrypto under the numbers of the reference: the same frames
        # the receiver
        rw.recover_dev(rf, n, p("slots"), p("buf"), p("off"), p("rnum"), p("rhi"))
        kt.frames_crypt_x_dev(1, xf, n, p("slots"), p("rhi"), p("buf"), p("off"), p("buf"), d_auth=p("auth"))
        rw.commit_dev(n, p("slots"), p("rnum"), p("auth"), p("auth"), p("why"))
        hip.dev_sync()
        assert list(struct.unpack("<%dQ" % n, bytes(d["rnum"].download(8 * n)))) == nums
        assert list(struct.unpack("<%di" % n, bytes(d["why"].download(4 * n)))) == [RX.ACCEPT] * n
        assert rw.get()[0] == [seen[s] for s in range(n_sa)] == tc.get()[0]
        for b in d.values():
            b.free()


def test_classic_macsec_fails_closed_past_2_32(hip, evp):  # noqa: F811
    key_len, n = 16, 12
    wf, tf = hip.WireFormat.macsec(), hip.TxFormat.macsec()
    keys, salts = splitmix_bytes(0x7F20, key_len * 2), [splitmix_bytes(0x7F21, 8), splitmix_bytes(0x7F22, 8)]
    slots = [0, 1] * (n // 2)
    plain = [splitmix_bytes(0x7F30 + i, wf.hdr_len + 20 + i) + b"\xAA" * 16 for i in range(n)]
    off, buf = _layout(plain, 5)
    with hip.KeyTable(key_len, 2) as kt, hip.TxCounters(2, n) as tc:
        kt.set(0, keys).set_salt(0, b"".join(salts))
        tc.set(0, [2 ** 32 - 3, 7], [2 ** 64 - 1, 2 ** 64 - 1])               # whatever `limit` says
        d = {k: _up(hip, v) for k, v in (("ctr", _u32(slots)), ("slots", _u32(slots)), ("off", _u64(off)), ("buf", buf), ("num", bytes(8 * n)))}
        tc.assign_dev(tf, n, d["ctr"].ptr, d["buf"].ptr, d["off"].ptr, d["num"].ptr, None, d["slots"].ptr)
        kt.frames_crypt_dev(0, wf, n, d["slots"].ptr, d["buf"].ptr, d["off"].ptr, d["buf"].ptr)
        hip.dev_sync()
        nums = list(struct.unpack("<%dQ" % n, bytes(d["num"].download(8 * n))))
        assert nums == [x for i in range(n // 2) for x in (2 ** 32 - 3 + i if i < 3 else R.NONE, 7 + i)]
        assert tc.status() == (hip.EARG, 6) and kt.status() == (hip.EARG, 6)  # the encrypt call refuses exactly the frames that got no number
        assert tc.get()[0] == [2 ** 32 + 3, 13]                               # ... whose numbers are burnt
        numbered = [f[:16] + struct.pack(">I", x & U32) + f[20:] if x != R.NONE else f for f, x in zip(plain, nums)]
        ok = [i for i, x in enumerate(nums) if x != R.NONE]
        wire = wire_ref_encrypt(evp, key_len, keys, salts, wf, [slots[i] for i in ok], [numbered[i] for i in ok])
        want = list(plain)                                                    # a refused frame: not a byte of it written, by either call
        for i, w in zip(ok, wire):
            want[i] = w
        assert bytes(d["buf"].download(len(buf))) == _layout(want, 5)[1]
        for b in d.values():
            b.free()


def test_a_tls13_leg_takes_its_sequence_numbers_from_the_counters(hip, evp):  # noqa: F811
    key_len, n = 16, 40
    keys, ivs = splitmix_bytes(0x7F40, key_len * 2), [splitmix_bytes(0x7F41, 12), splitmix_bytes(0x7F42, 12)]
    slots = [(i * i) % 2 for i in range(n)]
    recs = []
    for i in range(n):
        body = splitmix_bytes(0x7F50 + i, 1 + 3 * i) + b"\x17"
        recs.append(b"\x17\x03\x03" + struct.pack(">H", len(body) + 16) + body + b"\xAA" * 16)
    off, buf = _layout(recs, 5)
    with hip.KeyTable(key_len, 2) as kt, hip.TxCounters(2, n) as tc:
        kt.set(0, keys).set_tls_iv(0, b"".join(ivs))
        tc.set(0, [0, 1000], [2 ** 64 - 1, 1000 + 12])                        # connection 1 may send twelve records more before it must rekey
        d = {k: _up(hip, v) for k, v in (("ctr", _u32(slots)), ("slots", _u32(slots)), ("off", _u64(off)), ("buf", buf), ("seq", bytes(8 * n)))}
        tc.assign_dev(hip.TxFormat.number_only(), n, d["ctr"].ptr, None, None, d["seq"].ptr, None, d["slots"].ptr)
        kt.records_crypt_dev(0, hip.TlsFormat.tls13(), n, d["slots"].ptr, d["seq"].ptr, d["buf"].ptr, d["off"].ptr, d["buf"].ptr)
        hip.dev_sync()
        seqs = list(struct.unpack("<%dQ" % n, bytes(d["seq"].download(8 * n))))
        nums, _, refused, _, bad = R.assign(R.FORMATS["number_only"], {0: [0, 2 ** 64 - 1], 1: [1000, 1012]}, slots)
        assert seqs == nums and refused.count(True) == slots.count(1) - 12 and tc.status() == kt.status() == (hip.EARG, bad)
        ok = [i for i in range(n) if not refused[i]]
        wire = tls_ref_encrypt(evp, key_len, keys, ivs, T.TLS13, [slots[i] for i in ok], [seqs[i] for i in ok], [recs[i] for i in ok])
        want = list(recs)
        for i, w in zip(ok, wire):
            want[i] = w
        assert bytes(d["buf"].download(len(buf))) == _layout(want, 5)[1]
        assert tc.get() == ([slots.count(0), 1012], [2 ** 64 - 1, 1012])
        for b in d.values():
            b.free()


# ---------------------------------------------------------------- capture
def test_assign_and_encrypt_in_one_graph_continue_from_replay_to_replay(hip, evp):  # noqa: F811
    rng = random.Random("tx graph")
    key_len, n_sa, n = 16, 3, 300
    xf, tf = hip.WireFormatX.macsec_xpn(), hip.TxFormat.macsec_xpn()
    keys, sa = splitmix_bytes(0x7F60, key_len * n_sa), Sa(n_sa, 0x7F61)
    with hip.KeyTable(key_len, n_sa) as kt, hip.TxCounters(n_sa, n) as tc:
        kt.set(0, keys).set_salt(0, b"".join(sa.salt)).set_xpn(0, b"".join(sa.xsalt), b"".join(sa.ssci))
        size = 5 + n * (xf.f.hdr_len + 60 + 16) + 37
        d = {k: _up(hip, v) for k, v in (("ctr", bytes(4 * n)), ("slots", bytes(4 * n)), ("off", bytes(8 * (n + 1))), ("buf", bytes(size)), ("num", bytes(8 * n)), ("hi", bytes(4 * n)))}
        p = lambda k: d[k].ptr

        def enqueue(st=None):
            tc.assign_dev(tf, n, p("ctr"), p("buf"), p("off"), p("num"), p("hi"), p("slots"), stream=st)
            kt.frames_crypt_x_dev(0, xf, n, p("slots"), p("hi"), p("buf"), p("off"), p("buf"), stream=st)

        def load(seed):
            r = random.Random(seed)
            ctrs = [r.randrange(n_sa + (seed == 2)) for _ in range(n)]        # the second replay names a counter that does not exist
            plain = [splitmix_bytes(0x7F70 + 1000 * seed + i, xf.f.hdr_len + r.randrange(0, 61)) + b"\xAA" * 16 for i in range(n)]
            off, buf = _layout(plain, 5)
            d["ctr"].upload(_u32(ctrs)); d["slots"].upload(_u32([c % n_sa for c in ctrs])); d["off"].upload(_u64(off)); d["buf"].upload(buf)
            return ctrs, plain, off, buf

        # the ordinary call first, then the counters where the reference starts
        load(0)
        enqueue()
        hip.dev_sync()
        tc.status(), kt.status()
        counters = {0: [2 ** 32 - 150, 2 ** 64 - 1], 1: [9, 9 + 150], 2: [2 ** 40, 2 ** 64 - 1]}
        tc.set(0, [counters[c][0] for c in range(n_sa)], [counters[c][1] for c in range(n_sa)])
        hip.dev_sync()
        st = G.stream_create()
        with G.Graph(st, lambda: tc.assign_dev(tf, n, p("ctr"), p("buf"), p("off"), p("num"), p("hi"), p("slots"), stream=st)) as alone:
            assert alone.nodes == 3 * 1 + 2                                   # one sort pass of three launches, k_tx_heads, k_tx_assign: never launched here
        with G.Graph(st, lambda: enqueue(st)) as g:
            assert g.nodes > alone.nodes
            for seed in (1, 2, 3):
                ctrs, plain, off, buf = load(seed)
                g.launch()
                nums, his, refused, numbered_buf, bad = R.assign((16, 4, 0, 0), counters, ctrs, buf, off)
                assert list(struct.unpack("<%dQ" % n, bytes(d["num"].download(8 * n)))) == nums, seed
                assert tc.status() == kt.status() == ((hip.EARG, bad) if bad is not None else (hip.OK, 0)), seed
                ok = [i for i in range(n) if not refused[i]]
                numbered = [numbered_buf[off[i]:off[i + 1]] for i in range(n)]
                wire = x_ref_encrypt(evp, key_len, keys, sa, xf, [ctrs[i] for i in ok], [his[i] for i in ok], [numbered[i] for i in ok])
                want = list(plain)
                for i, w in zip(ok, wire):
                    want[i] = w
                assert bytes(d["buf"].download(len(buf))) == _layout(want, 5)[1], seed
                assert tc.get() == ([counters[c][0] for c in range(n_sa)], [counters[c][1] for c in range(n_sa)]), seed
            assert counters[1][0] == 159 and counters[0][0] > 2 ** 32           # a limit was reached and 2^32 crossed on the way
        G.stream_destroy(st)
        for b in d.values():
            b.free()
