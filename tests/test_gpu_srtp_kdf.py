"""GPU: SRTP's on-device key derivation (aesgcm_srtp_kdf_*).  Masters and session keys cannot be read back, so everything is checked through what the installed slots
DO: short SRTP or SRTCP packets are encrypted on the GPU under the installed slots (crypt_srtp) and must equal, every byte, srtp_fixture.protect under the session key
and salt that tests/srtp_kdf_ref.py derives over libcrypto, and must decrypt back.
  vectors      RFC 3711 B.3, RFC 6188 7.2 and 7.1 installed and used, on RFC 7714's RTP packets where the key size has one
  install      key sizes 16 / 24 / 32 x SRTP / SRTCP x 1 / 257 / 4097 entries (below a workgroup, one lane into the second, one into the seventeenth): d_r NULL, all
               zero and mixed (1 and 2^48 - 1 among them), d_idx and d_slots permuted, two to four packets per slot
  both kinds   an SRTP and an SRTCP slot of the same records, two calls on one stream
  refusals     one of each kind scattered through 257 entries: the lowest in status(), the refused entries' slots as before, every other entry installed
  guards       d_idx, d_slots and d_r between guard bytes; the slots and records next to the named ones unchanged
  re-install   the same slots under r + 1
  capture      install + encrypt in one graph, three replays, the master records changed by set_dev between them
  sender loop  TxCounters writes the SRTCP indices; the slots of both key-derivation periods installed; the reference unprotects every packet"""
import random
import struct

import pytest

import hip_graph as G
import pkt_grid as PG
import srtp_fixture as S
import srtp_kdf_ref as K
from kt_common import Guarded, _u32, _u64, _up
from util import splitmix_bytes

pytestmark = pytest.mark.gpu

RTP, RTCP = S.RTP, S.RTCP
R_MAX = (1 << 48) - 1


def _masters(seed, n, key_len):
    """n (master key, 14-byte master salt)"""
    kb, sb = splitmix_bytes(seed * 100003 + key_len, key_len * n), splitmix_bytes(seed * 100003 + key_len + 1, 14 * n)
    return [(kb[key_len * i:key_len * (i + 1)], sb[14 * i:14 * i + 14]) for i in range(n)]


def _set(table, first, masters):
    return table.set(first, [m[0] for m in masters], [m[1] for m in masters])


_SESSIONS = {}


def _session(kind, master, r):
    k = (kind, master, r)
    if k not in _SESSIONS:
        _SESSIONS[k] = K.session(kind, master[0], master[1], r)
    return _SESSIONS[k]


def _plain(kind, p, body_len):
    """packet p before protection: the headers written, 0xAA where the tag goes, SRTCP's W = E | an index"""
    fill = splitmix_bytes(0x5A0000 + p, 16 + body_len)
    if kind == RTP:
        return S.rtp_header(0, None, (p * 7919) & 0xFFFF, p * 160, 0x1000 + p, b"") + fill[16:] + b"\xAA" * 16
    return bytes([0x80, 200]) + fill[0:2] + fill[4:8] + fill[16:] + b"\xAA" * 16 + (0x80000000 | (p * 31 + 1) & 0x7FFFFFFF).to_bytes(4, "big")


def _check(hip, kt, kind, entries, label="", per=lambda i: 2):
    """entries: (the (key, salt) its slot should hold, slot); per(i) short packets under each -- the GPU's packets against the fixture's, every byte, and back"""
    rtp = kind == RTP
    fmt = hip.SrtpFormat.rtp() if rtp else hip.SrtpFormat.rtcp()
    slots, pkts, who = [], [], []
    for i, (_, slot) in enumerate(entries):
        for j in range(per(i)):
            slots.append(slot)
            pkts.append(_plain(kind, len(pkts), 5 + (3 * i + 11 * j) % 29))
            who.append(i)
    rocs = [(p * 0x9E3779B1) & 0xFFFFFFFF for p in range(len(pkts))]
    got, _ = kt.crypt_srtp(fmt, slots, pkts, rocs=rocs if rtp else None)
    for p, i in enumerate(who):
        key, salt = entries[i][0]
        assert bytes(got[p]) == S.protect(kind, key, salt, rocs[p], pkts[p]), (label, kind, kt.key_len, "entry", i, "packet", p)
    back, auth = kt.crypt_srtp(fmt, slots, got, decrypt=True, rocs=rocs if rtp else None)
    assert auth == [1] * len(pkts), label
    tail = 16 if rtp else 20
    for p in range(len(pkts)):
        assert bytes(back[p])[:-tail] == pkts[p][:-tail], (label, p)
    assert kt.status() == (hip.OK, 0), label


# ---------------------------------------------------------------- the published vectors
def test_published_vectors_installed_and_used(hip):
    rfc7714 = {len(v[2]): v for v in S.vectors() if v[1] == RTP}
    assert set(rfc7714) == {16, 32}
    for name, mk, ms, sk, ss in K.vectors():
        with hip.MasterKeyTable(len(mk), 1) as mt, hip.KeyTable(len(mk), 1) as kt:
            mt.set(0, mk, ms).install(hip.SRTP_RTP, kt, [0], [0])
            assert mt.status() == (hip.OK, 0)
            if len(mk) in rfc7714:                                              # RFC 7714's own packet and rollover counter, under the derived key
                _, _, _, _, roc, pkt, _, _ = rfc7714[len(mk)]
            else:
                roc, pkt = 0x00010203, _plain(RTP, 1, 38)
            got, _ = kt.crypt_srtp(hip.SrtpFormat.rtp(), [0], [pkt], rocs=[roc])
            assert bytes(got[0]) == S.protect_rtp(sk, ss[:12], roc, pkt), name
            back, auth = kt.crypt_srtp(hip.SrtpFormat.rtp(), [0], got, decrypt=True, rocs=[roc])
            assert auth == [1] and bytes(back[0])[:-16] == pkt[:-16], name
            assert (sk, ss[:12]) == K.session(RTP, mk, ms)
            _check(hip, kt, RTP, [((sk, ss[:12]), 0)], name)


# ---------------------------------------------------------------- install
@pytest.mark.parametrize("n", [1, 257, 4097])
@pytest.mark.parametrize("kind", [RTP, RTCP])
@pytest.mark.parametrize("key_len", [16, 24, 32])
def test_install_every_key_size_kind_and_count(hip, key_len, kind, n):
    """three calls into three groups of slots: d_r NULL, d_r all zero, d_r mixed; entry i goes from record idx[i] to slot slots[i], both permuted"""
    rng = random.Random("srtp kdf %d %d %d" % (key_len, kind, n))
    masters = _masters(n + kind, n, key_len)
    mixed = [rng.choice((0, 1, 2, 1 << 16, 1 << 32, R_MAX, rng.getrandbits(48))) for _ in range(n)]
    mixed[0], mixed[-1] = R_MAX, 1
    if n > 2:
        mixed[1] = 0
    entries = []
    with hip.MasterKeyTable(key_len, n) as mt, hip.KeyTable(key_len, 3 * n) as kt:
        _set(mt, 0, masters)
        for g, rs in enumerate((None, [0] * n, mixed)):
            idx, slots = list(range(n)), list(range(g * n, (g + 1) * n))
            rng.shuffle(idx)
            rng.shuffle(slots)
            mt.install(kind, kt, idx, slots, rs)
            entries += [(_session(kind, masters[idx[i]], rs[i] if rs else 0), slots[i]) for i in range(n)]
        assert mt.status() == (hip.OK, 0)
        _check(hip, kt, kind, entries, "n=%d" % n, per=lambda i: 2 if i < 2 * n else 2 + i % 3)


def test_twelve_byte_master_salts_are_padded_on_the_right(hip):
    masters = _masters(7, 3, 16)
    with hip.MasterKeyTable(16, 3) as mt, hip.KeyTable(16, 3) as kt:
        mt.set(0, [m[0] for m in masters], [m[1][:12] for m in masters]).install(hip.SRTP_RTCP, kt, [0, 1, 2], [2, 1, 0], [0, 1, R_MAX])
        _check(hip, kt, RTCP, [(K.session(RTCP, m[0], m[1][:12] + b"\0\0", r), s) for m, s, r in zip(masters, (2, 1, 0), (0, 1, R_MAX))], "12-byte salts")
        for bad in ([m[1][:13] for m in masters], [m[1] for m in masters[:2]]):
            with pytest.raises(hip.AesGcmError):
                mt.set(0, [m[0] for m in masters], bad)


# ---------------------------------------------------------------- both kinds of one master
@pytest.mark.parametrize("key_len", [16, 32])
def test_rtp_and_rtcp_slots_of_the_same_records(hip, key_len):
    n = 70
    masters = _masters(21, n, key_len)
    rs = [i % 3 for i in range(n)]
    with hip.MasterKeyTable(key_len, n) as mt, hip.KeyTable(key_len, 2 * n) as kt:
        _set(mt, 0, masters)
        idx, a, b = _up(hip, _u32(list(range(n)))), _up(hip, _u32(list(range(n)))), _up(hip, _u32(list(range(n, 2 * n))))
        d_r = _up(hip, _u64(rs))
        try:
            mt.install_dev(hip.SRTP_RTP, kt, n, idx.ptr, a.ptr, d_r.ptr)        # two calls behind one another on one (the null) stream
            mt.install_dev(hip.SRTP_RTCP, kt, n, idx.ptr, b.ptr, d_r.ptr)
            hip.dev_sync()
        finally:
            for d in (idx, a, b, d_r):
                d.free()
        assert mt.status() == (hip.OK, 0)
        rtp = [(_session(RTP, masters[i], rs[i]), i) for i in range(n)]
        rtcp = [(_session(RTCP, masters[i], rs[i]), n + i) for i in range(n)]
        assert all(x[0][0] != y[0][0] and x[0][1] != y[0][1] for x, y in zip(rtp, rtcp))     # the two slots of a master differ
        _check(hip, kt, RTP, rtp, "rtp slots")
        _check(hip, kt, RTCP, rtcp, "rtcp slots")
        # ... and each holds its own label's keys: an SRTCP packet under the SRTP slot is the fixture's under the SRTP key
        _check(hip, kt, RTCP, rtp[:5], "rtcp packets under rtp slots")


# ---------------------------------------------------------------- refusals
def test_refusals_scattered_through_257_entries(hip):
    """index out of range, record unset, record cleared, slot out of range, r = 2^48: each entry skipped whole, its slot still under the key it held before, every
    other entry installed, the lowest in the master table's status, the key table's untouched"""
    n, key_len, kind = 257, 24, RTP
    masters = _masters(31, n, key_len)
    old = _masters(32, n, key_len)                                               # what every slot holds before the call: keys set by hand
    with hip.MasterKeyTable(key_len, n + 2) as mt, hip.KeyTable(key_len, n) as kt:
        _set(mt, 0, masters)                                                    # records n, n + 1 stay unset
        kt.set(0, b"".join(o[0] for o in old)).set_tls_iv(0, b"".join(o[1][:12] for o in old))
        idx, slots, rs = list(range(n)), list(range(n)), [i % 5 for i in range(n)]
        random.Random(33).shuffle(slots)
        bad = {17: "idx", 64: "unset", 100: "cleared", 200: "slot", 256: "r"}
        idx[17], idx[64] = n + 2, n + 1
        mt.clear(100)
        victim_slot = slots[200]
        slots[200] = n
        rs[256] = 1 << 48
        mt.install(kind, kt, idx, slots, rs)
        assert mt.status() == (hip.EARG, 17) and mt.status() == (hip.OK, 0)     # the lowest index; reading clears
        assert kt.status() == (hip.OK, 0)                                       # the key table's own status is not touched
        slots[200] = victim_slot                                                # (the slot the entry would have named, had it been in range: as before too)
        entries = [((old[slots[i]][0], old[slots[i]][1][:12]) if i in bad else _session(kind, masters[idx[i]], rs[i]), slots[i]) for i in range(n)]
        _check(hip, kt, kind, entries, "refusals")
        # the refused entries' records are as they were: the cleared one stays refused, the others install
        mt.install(kind, kt, [100, 17, 64], [0, 1, 2], [0, 0, 0])
        assert mt.status() == (hip.EARG, 0)
        _check(hip, kt, kind, [(entries[slots.index(0)][0], 0), (_session(kind, masters[17], 0), 1), (_session(kind, masters[64], 0), 2)], "after")
        with pytest.raises(hip.AesGcmError):
            mt.install(3, kt, [0], [0])                                         # a kind that is neither constant
        with hip.KeyTable(16, 1) as other:
            with pytest.raises(hip.AesGcmError):
                mt.install(kind, other, [0], [0])                               # a key table of another key size


# ---------------------------------------------------------------- guards
@pytest.mark.parametrize("key_len,kind", [(16, RTCP), (32, RTP)])
def test_guard_bytes_slots_and_records_around_257_entries(hip, key_len, kind):
    n = 257
    masters = _masters(41, n + 2, key_len)
    rng = random.Random("guards %d" % key_len)
    idx, slots = list(range(1, n + 1)), list(range(1, n + 1))
    rng.shuffle(idx)
    rng.shuffle(slots)
    rs = [rng.choice((0, 3, R_MAX)) for _ in range(n)]
    with hip.MasterKeyTable(key_len, n + 2) as mt, hip.KeyTable(key_len, n + 2) as kt:
        _set(mt, 0, masters[:n + 1])                                            # record 0 is set and never named, record n + 1 stays unset
        mt.install(kind, kt, [0], [0], [9])                                     # slot 0 holds record 0's keys under r = 9, slot n + 1 stays unset
        g_idx, g_slots, g_r = Guarded(hip, 4 * n), Guarded(hip, 4 * n), Guarded(hip, 8 * n)
        for g, data in ((g_idx, _u32(idx)), (g_slots, _u32(slots)), (g_r, _u64(rs))):
            g.buf.upload(data, PG.GUARD)
        mt.install_dev(kind, kt, n, g_idx.ptr, g_slots.ptr, g_r.ptr)
        hip.dev_sync()
        assert g_idx.read("d_idx") == _u32(idx) and g_slots.read("d_slots") == _u32(slots) and g_r.read("d_r") == _u64(rs)
        assert mt.status() == (hip.OK, 0)
        _check(hip, kt, kind, [(_session(kind, masters[idx[i]], rs[i]), slots[i]) for i in range(n)] + [(_session(kind, masters[0], 9), 0)], "inside and the set guard")
        # the unset guard slot still refuses its packet: it comes back as it went in
        pkt = _plain(kind, 0, 20)
        fmt = hip.SrtpFormat.rtp() if kind == RTP else hip.SrtpFormat.rtcp()
        out, _ = kt.crypt_srtp(fmt, [n + 1], [pkt], rocs=[0] if kind == RTP else None)
        assert bytes(out[0]) == pkt and kt.status() == (hip.EARG, 0)
        # the records: 0 and the inner ones still hold their masters, n + 1 is still unset
        mt.install(kind, kt, [0, n + 1, idx[0]], [0, n + 1, 1], [0, 0, 1])
        assert mt.status() == (hip.EARG, 1)
        _check(hip, kt, kind, [(_session(kind, masters[0], 0), 0), (_session(kind, masters[idx[0]], 1), 1)], "records")
        for g in (g_idx, g_slots, g_r):
            g.buf.free()


# ---------------------------------------------------------------- re-install
def test_reinstall_under_the_next_r(hip):
    n, key_len = 40, 32
    masters = _masters(51, n, key_len)
    rs = [R_MAX - 1 if i == 0 else i * 1000 for i in range(n)]
    with hip.MasterKeyTable(key_len, n) as mt, hip.KeyTable(key_len, n) as kt:
        _set(mt, 0, masters)
        for step in (0, 1):
            now = [r + step for r in rs]
            mt.install(RTCP, kt, list(range(n)), list(range(n)), now)
            assert mt.status() == (hip.OK, 0)
            _check(hip, kt, RTCP, [(_session(RTCP, masters[i], now[i]), i) for i in range(n)], "r + %d" % step)
        # the old keys are gone: a packet of the first period no longer authenticates
        pkt = _plain(RTCP, 3, 24)
        wire = S.protect_rtcp(*_session(RTCP, masters[5], rs[5]), pkt)
        _, auth = kt.crypt_srtp(hip.SrtpFormat.rtcp(), [5], [wire], decrypt=True)
        assert auth == [0]


# ---------------------------------------------------------------- capture
def test_captured_install_and_encrypt_replays_over_changed_masters(hip):
    """install_dev and srtp_crypt_dev (encrypt) captured on one created stream after one ordinary call of each; between the replays set_dev puts other masters into the
    records: each replay gives the fixture's packets under that generation's session keys"""
    n, key_len, kind = 300, 16, RTP
    gens = [_masters(60 + g, n, key_len) for g in range(3)]
    rs = [(i * 7) % 11 for i in range(n)]
    pkts = [_plain(kind, p, 9 + p % 23) for p in range(n)]
    rocs = [p & 3 for p in range(n)]
    off = [0]
    for r in pkts:
        off.append(off[-1] + len(r))
    plain = b"".join(pkts)
    perm = list(range(n))
    random.Random(6).shuffle(perm)
    st = G.stream_create()
    with hip.MasterKeyTable(key_len, n) as mt, hip.KeyTable(key_len, n) as kt:
        d_idx, d_slots, d_r = _up(hip, _u32(perm)), _up(hip, _u32(perm)), _up(hip, _u64(rs))
        d_all, d_pslots, d_roc, d_off = _up(hip, _u32(list(range(n)))), _up(hip, _u32(list(range(n)))), _up(hip, _u32(rocs)), _up(hip, _u64(off))
        d_in, d_out = _up(hip, plain), _up(hip, bytes(len(plain)))
        d_keys = [_up(hip, b"".join(m[0] for m in g)) for g in gens]
        d_salts = [_up(hip, b"".join(m[1] for m in g)) for g in gens]
        fmt = hip.SrtpFormat.rtp()

        def enqueue():
            mt.install_dev(kind, kt, n, d_idx.ptr, d_slots.ptr, d_r.ptr, stream=st)
            kt.srtp_crypt_dev(0, fmt, n, d_pslots.ptr, d_in.ptr, d_off.ptr, d_out.ptr, d_roc=d_roc.ptr, stream=st)

        try:
            mt.set_dev(n, d_all.ptr, d_keys[0].ptr, d_salts[0].ptr, stream=st)
            enqueue()                                                           # the ordinary call of each
            G.synchronize(st)
            with G.Graph(st, enqueue) as graph:
                for g in range(3):
                    mt.set_dev(n, d_all.ptr, d_keys[g].ptr, d_salts[g].ptr, stream=st)       # record i = master i of generation g, outside the capture
                    G.synchronize(st)
                    graph.launch()
                    out = bytes(d_out.download(len(plain)))
                    for p in range(n):                                          # packet p under slot p = the entry e with perm[e] == p: record p, r = rs[e]
                        e = perm.index(p)
                        key, salt = _session(kind, gens[g][p], rs[e])
                        assert out[off[p]:off[p + 1]] == S.protect_rtp(key, salt, rocs[p], pkts[p]), (g, p)
            assert mt.status() == (hip.OK, 0) and kt.status() == (hip.OK, 0)
        finally:
            for b in [d_idx, d_slots, d_r, d_all, d_pslots, d_roc, d_off, d_in, d_out] + d_keys + d_salts:
                b.free()
    G.stream_destroy(st)


# ---------------------------------------------------------------- the sender loop
def test_sender_loop_with_send_counters_across_a_derivation_period(hip):
    """an SRTCP sender with key_derivation_rate 16: TxCounters writes the indices 10 .. 33 into the packets; the slots of the periods r = 0, 1, 2 are installed from
    the one master record; every packet, encrypted under its period's slot, is unprotected by the reference under that period's session key"""
    kdr, first, n, key_len = 16, 10, 24, 32
    master = _masters(71, 1, key_len)[0]
    pkts = [_plain(RTCP, p, 12 + p)[:-4] + b"\x80\0\0\0" for p in range(n)]      # E set, the index still to be written
    with hip.MasterKeyTable(key_len, 1) as mt, hip.KeyTable(key_len, 3) as kt, hip.TxCounters(1, n) as tc:
        _set(mt, 0, [master])
        tc.set(0, [first], [1 << 31])
        numbered, nums, _, refused = tc.assign(hip.TxFormat.srtcp(), [0] * n, pkts)
        assert refused == [False] * n and nums == list(range(first, first + n))
        periods = sorted({q // kdr for q in nums})
        assert periods == [0, 1, 2]
        mt.install(hip.SRTP_RTCP, kt, [0] * len(periods), periods, periods)     # slot r holds the keys of period r
        assert mt.status() == (hip.OK, 0)
        sent, _ = kt.crypt_srtp(hip.SrtpFormat.rtcp(), [q // kdr for q in nums], [bytes(x) for x in numbered])
        for p, q in enumerate(nums):
            w = bytes(sent[p])
            assert int.from_bytes(w[-4:], "big") == 0x80000000 | q
            back, ok = S.unprotect_rtcp(*_session(RTCP, master, q // kdr), w)
            assert ok and back[:-20] == pkts[p][:-20], p
            if q // kdr != 1:                                                   # ... and under no other period's key
                assert not S.unprotect_rtcp(*_session(RTCP, master, 1), w)[1], p
        assert kt.status() == (hip.OK, 0) and tc.status() == (hip.OK, 0)


# ---------------------------------------------------------------- calls that need a table
def test_set_dev_clear_and_argument_errors_with_a_table(hip):
    key_len = 24
    m = _masters(81, 3, key_len)
    with hip.MasterKeyTable(key_len, 4) as mt, hip.KeyTable(key_len, 4) as kt:
        d_idx = _up(hip, _u32([2, 9, 0]))
        d_keys, d_salts = _up(hip, b"\xEE" + b"".join(x[0] for x in m)), _up(hip, b"\xEE\xEE\xEE" + b"".join(x[1] for x in m))      # (odd addresses: no alignment to keep)
        try:
            mt.set_dev(3, d_idx.ptr, d_keys.ptr + 1, d_salts.ptr + 3)
            hip.dev_sync()
            assert mt.status() == (hip.EARG, 1)                                  # record 9 does not exist
            mt.install(RTP, kt, [2, 0], [0, 1], [4, 5])
            _check(hip, kt, RTP, [(_session(RTP, m[0], 4), 0), (_session(RTP, m[2], 5), 1)], "set_dev")
            mt.clear(2)
            mt.install(RTP, kt, [2, 0], [2, 3])
            assert mt.status() == (hip.EARG, 0)
            _check(hip, kt, RTP, [(_session(RTP, m[2], 0), 3)], "cleared")
            for call in (lambda: mt.set(4, m[0][0], m[0][1]), lambda: mt.set(3, m[0][0] + m[1][0], m[0][1] + m[1][1]), lambda: mt.clear(4), lambda: mt.clear(0, 5),
                         lambda: mt.set(0, b"x" * 23, m[0][1])):
                with pytest.raises(hip.AesGcmError):
                    call()
        finally:
            for d in (d_idx, d_keys, d_salts):
                d.free()
