"""GPU: the TLS 1.2 PRF on the device (aesgcm_prf12_*).  Master secrets and derived keys cannot be read back, so everything is checked through what the installed slots
DO: records are encrypted or decrypted on the GPU under the installed slots and must equal, every byte, what tls_fixture / dtls_fixture / srtp_fixture make under keys
that hmac derives (tls_fixture.prf12).
  recordings   the four OpenSSL connections (TLS 1.2 and DTLS 1.2, AES-128-GCM-SHA256 and AES-256-GCM-SHA384) installed from master_secret and the randoms: OpenSSL's
               own records of both directions decrypt with auth 1 and re-encrypt byte for byte
  install      2 hashes x 3 key sizes at 1 / 257 / 4097 entries (below a workgroup, one lane into the second, one into the seventeenth), indices and slots permuted
               and between guard words, the untouched slots compared before and after
  directions   client only, server only, 0xFFFFFFFF mixed per entry
  refusals     index out of range, unset, cleared, a slot out of range in either array: skipped whole, the lowest in status(), the other tables' status untouched
  exporter     OpenSSL's recorded exporter outputs (tests/golden/dtls_srtp_exporter.json) at key sizes 16 / 32; key sizes 16 / 32 x both hashes at 1 / 257 entries into a MasterKeyTable, then its install for RTP and RTCP, the packets against srtp_fixture under
               session keys that srtp_kdf_ref derives from exporter output computed with hmac; key_len 24 is EARG; refusals
  capture      install + encrypt, and export + SRTP install + encrypt, each in one linear graph replayed three times over changed masters
  loop         set_dev, install, TxCounters.assign, encrypt, decrypt under the peer's slot: launches on one stream, no host synchronisation in between"""
import random
import struct

import pytest

import dtls_fixture as D
import hip_graph as G
import pkt_grid as PG
import srtp_fixture as S
import srtp_kdf_ref as K
import tls_fixture as T
from kt_common import Guarded, _u32, _u64, _up
from oracle import libcrypto_ref as R
from util import splitmix_bytes

pytestmark = pytest.mark.gpu

HASH = {32: "sha256", 48: "sha384"}
NONE = 0xFFFFFFFF
WHO = ("client", "server")


def _masters(seed, n):
    """n (master secret, client random, server random)"""
    b = splitmix_bytes(seed * 100003 + 12, 112 * n)
    return [(b[112 * i:112 * i + 48], b[112 * i + 48:112 * i + 80], b[112 * i + 80:112 * i + 112]) for i in range(n)]


def _set(table, first, masters):
    return table.set(first, [m[0] for m in masters], [m[1] for m in masters], [m[2] for m in masters])


def _keys(hl, m, kl):
    """-> ((client key, client IV[4]), (server key, server IV[4])) by RFC 5246 6.3 for an AEAD suite"""
    block = T.prf12(HASH[hl], m[0], b"key expansion", m[2] + m[1], 2 * kl + 8)
    return tuple((block[d * kl:(d + 1) * kl], block[2 * kl + 4 * d:2 * kl + 4 * d + 4]) for d in (0, 1))


def _exported(hl, m, kl):
    """-> ((client master key, 14-byte master salt), (server ...)) by RFC 5764 4.2 with 12-byte salts, two zero bytes appended"""
    out = T.prf12(HASH[hl], m[0], b"EXTRACTOR-dtls_srtp", m[1] + m[2], 2 * kl + 24)
    return tuple((out[d * kl:(d + 1) * kl], out[2 * kl + 12 * d:2 * kl + 12 * d + 12] + b"\0\0") for d in (0, 1))


def _plain12(i, seq):
    """a TLS 1.2 AES-GCM record before protection: header | explicit nonce = the sequence number | payload | 16 placeholder bytes"""
    body = splitmix_bytes(3000 + i, 17 + i % 19)
    return b"\x17\x03\x03" + struct.pack(">H", 8 + len(body) + 16) + struct.pack(">Q", seq) + body + bytes(16)


def _protect12(key, iv4, seq, rec):
    ct, tag = R.encrypt(key, iv4 + rec[5:13], T.aad_of(T.TLS12, seq, rec), rec[13:-16])
    return rec[:13] + bytes(ct) + bytes(tag)


def _check(hip, kt, entries, label=""):
    """entries: ((key, iv4) the slot should hold, slot) -- one TLS 1.2 record each on the GPU against the formulas over libcrypto, every byte"""
    seqs = [(i * 0x9E3779B1 + 7) & 0xFFFFFFFFFFFF for i in range(len(entries))]
    recs = [_plain12(i, seqs[i]) for i in range(len(entries))]
    got, _ = kt.crypt_records(hip.TlsFormat.tls12(), [e[1] for e in entries], seqs, recs)
    for i, ((key, iv4), _) in enumerate(entries):
        assert bytes(got[i]) == _protect12(key, iv4, seqs[i], recs[i]), (label, kt.key_len, "entry", i)
    assert kt.status() == (hip.OK, 0), label


# ---------------------------------------------------------------- the recorded connections
def test_recorded_tls12_connections_from_their_master_secrets(hip):
    conns = [c for c in T.golden("tls_records.json")["connections"] if c["version"] != "1.3"]
    assert {(c["hash"], c["key_len"]) for c in conns} == {("sha256", 16), ("sha384", 32)}
    by_conn = {}
    for d in T.directions():
        if d[2] == T.TLS12:
            by_conn.setdefault(d[0]["master_secret"], {})[d[1]] = d[5]
    assert len(by_conn) == len(conns)
    for conn in conns:
        hl = {"sha256": 32, "sha384": 48}[conn["hash"]]
        with hip.MasterSecretTable(hl, 1) as mt, hip.KeyTable(conn["key_len"], 2) as kt:
            mt.set(0, bytes.fromhex(conn["master_secret"]), bytes.fromhex(conn["client_random"]), bytes.fromhex(conn["server_random"])).install(kt, [0], [0], [1])
            assert mt.status() == (hip.OK, 0)
            for slot, who in enumerate(WHO):
                recs = by_conn[conn["master_secret"]][who]
                seqs, wire = [r[0] for r in recs], [r[1] for r in recs]
                back, auth = kt.crypt_records(hip.TlsFormat.tls12(), [slot] * len(recs), seqs, wire, decrypt=True)
                assert auth == [1] * len(recs), (conn["hash"], who, auth)
                for b, (_, w, pt) in zip(back, recs):
                    assert bytes(b)[13:-16] == pt
                again, _ = kt.crypt_records(hip.TlsFormat.tls12(), [slot] * len(recs), seqs, [bytes(b)[:-16] + bytes(16) for b in back])
                assert [bytes(a) for a in again] == wire, (conn["hash"], who)


def test_recorded_dtls12_connections_from_their_master_secrets(hip):
    dirs = D.directions()
    assert {(d[0]["hash"], d[0]["key_len"]) for d in dirs} == {("sha256", 16), ("sha384", 32)}
    for conn, who, _, _, recs in dirs:
        hl = {"sha256": 32, "sha384": 48}[conn["hash"]]
        with hip.MasterSecretTable(hl, 1) as mt, hip.KeyTable(conn["key_len"], 2) as kt:
            mt.set(0, bytes.fromhex(conn["master_secret"]), bytes.fromhex(conn["client_random"]), bytes.fromhex(conn["server_random"])).install(kt, [0], [0], [1])
            slot = WHO.index(who)
            wire = [r[0] for r in recs]
            back, auth, _ = kt.crypt_dtls(hip.DtlsFormat.dtls12(), [slot] * len(recs), wire, decrypt=True)
            assert auth == [1] * len(recs), (conn["hash"], who, auth)
            for b, (w, pt) in zip(back, recs):
                assert bytes(b)[21:-16] == pt
            again, _, _ = kt.crypt_dtls(hip.DtlsFormat.dtls12(), [slot] * len(recs), [bytes(b)[:-16] + bytes(16) for b in back])
            assert [bytes(a) for a in again] == wire, (conn["hash"], who)
            assert mt.status() == (hip.OK, 0) and kt.status() == (hip.OK, 0)


# ---------------------------------------------------------------- install
@pytest.mark.parametrize("n", [1, 257, 4097])
@pytest.mark.parametrize("key_len", [16, 24, 32])
@pytest.mark.parametrize("hl", [32, 48])
def test_install_random_masters_between_guards(hip, hl, key_len, n):
    """slots 0 and 2 n + 1 are set by hand and never named; the arrays lie between guard words"""
    rng = random.Random("prf12 %d %d %d" % (hl, key_len, n))
    masters = _masters(n + hl + key_len, n)
    idx, cs, ss = list(range(n)), list(range(1, n + 1)), list(range(n + 1, 2 * n + 1))
    for v in (idx, cs, ss):
        rng.shuffle(v)
    edge = [(splitmix_bytes(5 + e, key_len), splitmix_bytes(9 + e, 4)) for e in (0, 1)]
    with hip.MasterSecretTable(hl, n) as mt, hip.KeyTable(key_len, 2 * n + 2) as kt:
        _set(mt, 0, masters)
        for e, slot in enumerate((0, 2 * n + 1)):
            kt.set(slot, edge[e][0]).set_tls_iv(slot, edge[e][1] + bytes(8))
        g = [Guarded(hip, 4 * n) for _ in range(3)]
        for gb, data in zip(g, (idx, cs, ss)):
            gb.buf.upload(_u32(data), PG.GUARD)
        mt.install_dev(kt, n, g[0].ptr, g[1].ptr, g[2].ptr)
        hip.dev_sync()
        assert [gb.read("array") for gb in g] == [_u32(idx), _u32(cs), _u32(ss)]
        assert mt.status() == (hip.OK, 0)
        entries = [(edge[0], 0), (edge[1], 2 * n + 1)]
        for i in range(n):
            ck, sk = _keys(hl, masters[idx[i]], key_len)
            entries += [(ck, cs[i]), (sk, ss[i])]
        _check(hip, kt, entries, "n=%d" % n)
        for gb in g:
            gb.buf.free()


@pytest.mark.parametrize("hl,key_len", [(32, 16), (48, 32)])
def test_one_direction_only(hip, hl, key_len):
    n = 70
    masters, old = _masters(21 + hl, n), [(splitmix_bytes(40 + i, key_len), splitmix_bytes(140 + i, 4)) for i in range(2 * n)]
    with hip.MasterSecretTable(hl, n) as mt, hip.KeyTable(key_len, 2 * n) as kt:
        _set(mt, 0, masters)

        def reset():
            kt.set(0, b"".join(o[0] for o in old)).set_tls_iv(0, b"".join(o[1] + bytes(8) for o in old))

        idx = list(range(n))
        want = lambda d, i: _keys(hl, masters[i], key_len)[d]
        reset()
        mt.install(kt, idx, list(range(n)), None)                                # client only: slots n .. 2 n - 1 keep their keys
        _check(hip, kt, [(want(0, i), i) for i in range(n)] + [(old[n + i], n + i) for i in range(n)], "client only")
        reset()
        mt.install(kt, idx, None, list(range(n, 2 * n)))
        _check(hip, kt, [(old[i], i) for i in range(n)] + [(want(1, i), n + i) for i in range(n)], "server only")
        reset()
        cs = [NONE if i % 3 == 0 else i for i in range(n)]
        ss = [NONE if i % 3 == 1 else n + i for i in range(n)]
        mt.install(kt, idx, cs, ss)
        _check(hip, kt, [(old[i] if cs[i] == NONE else want(0, i), i) for i in range(n)] + [(old[n + i] if ss[i] == NONE else want(1, i), n + i) for i in range(n)], "mixed")
        assert mt.status() == (hip.OK, 0)
        with pytest.raises(hip.AesGcmError):
            mt.install_dev(kt, 1, 16, None, None)                                # not both NULL


# ---------------------------------------------------------------- refusals
def test_refusals_scattered_through_257_entries(hip):
    n, hl, key_len = 257, 32, 24
    masters = _masters(31, n)
    old = [(splitmix_bytes(400 + i, key_len), splitmix_bytes(900 + i, 4)) for i in range(2 * n)]
    with hip.MasterSecretTable(hl, n + 2) as mt, hip.KeyTable(key_len, 2 * n) as kt, hip.MasterKeyTable(16, 1) as other:
        _set(mt, 0, masters)                                                    # records n, n + 1 stay unset
        kt.set(0, b"".join(o[0] for o in old)).set_tls_iv(0, b"".join(o[1] + bytes(8) for o in old))
        idx, cs, ss = list(range(n)), list(range(n)), list(range(n, 2 * n))
        bad = {17: "idx", 64: "unset", 100: "cleared", 200: "client slot", 230: "server slot"}
        idx[17], idx[64] = n + 2, n + 1
        mt.clear(100)
        cs[200], ss[230] = 2 * n, 2 * n + 5
        mt.install(kt, idx, cs, ss)
        assert mt.status() == (hip.EARG, 17) and mt.status() == (hip.OK, 0)     # the lowest index; reading clears
        assert kt.status() == (hip.OK, 0) and other.status() == (hip.OK, 0)     # the other tables' status words are not touched
        entries = []
        for i in range(n):
            ck, sk = (old[i], old[n + i]) if i in bad else _keys(hl, masters[idx[i]], key_len)
            entries += [(ck, i), (sk, n + i)]                                   # a refused entry's slots, the in-range one of 200 and 230 included, as before
        _check(hip, kt, entries, "refusals")
        mt.install(kt, [100, 17], None, [0, 1])                                 # no client array: the server's role reports
        assert mt.status() == (hip.EARG, 0)
        _check(hip, kt, [(entries[0][0], 0), (_keys(hl, masters[17], key_len)[1], 1)], "after")


# ---------------------------------------------------------------- the exporter
def _plain_srtp(kind, p, body_len):
    fill = splitmix_bytes(0x5A0000 + p, 16 + body_len)
    if kind == S.RTP:
        return S.rtp_header(0, None, (p * 7919) & 0xFFFF, p * 160, 0x1000 + p, b"") + fill[16:] + b"\xAA" * 16
    return bytes([0x80, 200]) + fill[0:2] + fill[4:8] + fill[16:] + b"\xAA" * 16 + (0x80000000 | (p * 31 + 1) & 0x7FFFFFFF).to_bytes(4, "big")


def _check_srtp(hip, kt, kind, entries, label=""):
    """entries: ((master key, 14-byte master salt) the slot's session keys come from, slot)"""
    rtp = kind == S.RTP
    fmt = hip.SrtpFormat.rtp() if rtp else hip.SrtpFormat.rtcp()
    pkts = [_plain_srtp(kind, p, 5 + (7 * p) % 29) for p in range(len(entries))]
    rocs = [(p * 0x9E3779B1) & 0xFFFFFFFF for p in range(len(pkts))]
    got, _ = kt.crypt_srtp(fmt, [e[1] for e in entries], pkts, rocs=rocs if rtp else None)
    for p, ((mk, ms), _) in enumerate(entries):
        key, salt = K.session(kind, mk, ms, 0)
        assert bytes(got[p]) == S.protect(kind, key, salt, rocs[p], pkts[p]), (label, kind, kt.key_len, "entry", p)
    assert kt.status() == (hip.OK, 0), label


@pytest.mark.parametrize("n", [1, 257])
@pytest.mark.parametrize("key_len", [16, 32])
@pytest.mark.parametrize("hl", [32, 48])
def test_exporter_into_a_master_key_table_and_on_into_slots(hip, hl, key_len, n):
    rng = random.Random("prf12 export %d %d %d" % (hl, key_len, n))
    masters = _masters(2 * n + hl + key_len, n)
    idx, cr, sr = list(range(n)), list(range(n)), list(range(n, 2 * n))
    for v in (idx, cr, sr):
        rng.shuffle(v)
    with hip.MasterSecretTable(hl, n) as mt, hip.MasterKeyTable(key_len, 2 * n) as mk, hip.KeyTable(key_len, 4 * n) as kt:
        _set(mt, 0, masters)
        mt.export_srtp(mk, idx, cr, sr)
        assert mt.status() == (hip.OK, 0) and mk.status() == (hip.OK, 0)
        recs = list(range(2 * n))
        mk.install(hip.SRTP_RTP, kt, recs, recs)
        mk.install(hip.SRTP_RTCP, kt, recs, [2 * n + r for r in recs])
        assert mk.status() == (hip.OK, 0)
        held = {}
        for i in range(n):
            c, s = _exported(hl, masters[idx[i]], key_len)
            held[cr[i]], held[sr[i]] = c, s
        _check_srtp(hip, kt, S.RTP, [(held[r], r) for r in recs], "rtp")
        _check_srtp(hip, kt, S.RTCP, [(held[r], 2 * n + r) for r in recs], "rtcp")


@pytest.mark.parametrize("key_len", [16, 32])
def test_exporter_outputs_that_openssl_recorded(hip, key_len):
    """tests/golden/dtls_srtp_exporter.json: the master keys and salts are cut from the bytes OpenSSL's SSL_export_keying_material gave, not computed here"""
    for c in T.golden("dtls_srtp_exporter.json")["connections"]:
        hl = {"sha256": 32, "sha384": 48}[c["hash"]]
        out = bytes.fromhex(c["exported"])[:2 * key_len + 24]
        held = [(out[d * key_len:(d + 1) * key_len], out[2 * key_len + 12 * d:2 * key_len + 12 * d + 12] + b"\0\0") for d in (0, 1)]
        with hip.MasterSecretTable(hl, 1) as mt, hip.MasterKeyTable(key_len, 2) as mk, hip.KeyTable(key_len, 4) as kt:
            mt.set(0, bytes.fromhex(c["master_secret"]), bytes.fromhex(c["client_random"]), bytes.fromhex(c["server_random"])).export_srtp(mk, [0], [0], [1])
            assert mt.status() == (hip.OK, 0)
            mk.install(hip.SRTP_RTP, kt, [0, 1], [0, 1]).install(hip.SRTP_RTCP, kt, [0, 1], [2, 3])
            _check_srtp(hip, kt, S.RTP, [(held[0], 0), (held[1], 1)], c["suite"])
            _check_srtp(hip, kt, S.RTCP, [(held[0], 2), (held[1], 3)], c["suite"])


def test_exporter_refusals_and_key_len_24(hip):
    n, hl, key_len = 40, 48, 16
    masters = _masters(77, n)
    old = [(splitmix_bytes(600 + i, key_len), splitmix_bytes(700 + i, 12) + b"\0\0") for i in range(2 * n)]
    with hip.MasterSecretTable(hl, n + 1) as mt, hip.MasterKeyTable(key_len, 2 * n) as mk, hip.KeyTable(key_len, 2 * n) as kt, hip.MasterKeyTable(24, 2) as mk24:
        _set(mt, 0, masters)
        mk.set(0, [o[0] for o in old], [o[1] for o in old])
        idx, cr, sr = list(range(n)), list(range(n)), list(range(n, 2 * n))
        bad = {3: "unset", 9: "idx", 20: "client rec", 33: "server rec"}
        idx[3], idx[9], cr[20], sr[33] = n, n + 7, 2 * n, NONE - 1
        cr[5], sr[6] = NONE, NONE                                               # not refusals: nothing installed for that direction
        mt.export_srtp(mk, idx, cr, sr)
        assert mt.status() == (hip.EARG, 3) and mk.status() == (hip.OK, 0) and kt.status() == (hip.OK, 0)
        held = {}
        for i in range(n):
            c, s = (old[i], old[n + i]) if i in bad else _exported(hl, masters[idx[i]], key_len)
            held[i], held[n + i] = (old[i] if cr[i] == NONE else c), (old[n + i] if sr[i] == NONE else s)
        mk.install(hip.SRTP_RTP, kt, list(range(2 * n)), list(range(2 * n)))
        _check_srtp(hip, kt, S.RTP, [(held[r], r) for r in range(2 * n)], "export refusals")
        with pytest.raises(hip.AesGcmError) as e:
            mt.export_srtp(mk24, [0], [0], [1])
        assert e.value.code == hip.EARG
        with pytest.raises(hip.AesGcmError):
            mt.export_srtp_dev(mk, 1, 16, None, None)


# ---------------------------------------------------------------- capture
def test_captured_install_and_encrypt_replays_over_changed_masters(hip):
    n, hl, key_len = 300, 32, 16
    gens = [_masters(60 + g, n) for g in range(3)]
    seqs = [p * 3 + 1 for p in range(n)]
    recs = [_plain12(p, seqs[p]) for p in range(n)]
    off = [0]
    for r in recs:
        off.append(off[-1] + len(r))
    plain = b"".join(recs)
    perm = list(range(n))
    random.Random(6).shuffle(perm)
    st = G.stream_create()
    with hip.MasterSecretTable(hl, n) as mt, hip.KeyTable(key_len, 2 * n) as kt:
        d_idx, d_cs, d_ss = _up(hip, _u32(perm)), _up(hip, _u32(perm)), _up(hip, _u32([n + x for x in perm]))
        d_all, d_pslots, d_seq, d_off = _up(hip, _u32(list(range(n)))), _up(hip, _u32([p if p % 2 == 0 else n + p for p in range(n)])), _up(hip, _u64(seqs)), _up(hip, _u64(off))
        d_in, d_out = _up(hip, plain), _up(hip, bytes(len(plain)))
        d_m = [[_up(hip, b"".join(m[k] for m in g)) for k in range(3)] for g in gens]
        fmt = hip.TlsFormat.tls12()

        def enqueue():
            mt.install_dev(kt, n, d_idx.ptr, d_cs.ptr, d_ss.ptr, stream=st)
            kt.records_crypt_dev(0, fmt, n, d_pslots.ptr, d_seq.ptr, d_in.ptr, d_off.ptr, d_out.ptr, stream=st)

        try:
            mt.set_dev(n, d_all.ptr, d_m[0][0].ptr, d_m[0][1].ptr, d_m[0][2].ptr, stream=st)
            enqueue()                                                           # the ordinary call of each
            G.synchronize(st)
            with G.Graph(st, enqueue) as graph:
                for g in range(3):
                    mt.set_dev(n, d_all.ptr, d_m[g][0].ptr, d_m[g][1].ptr, d_m[g][2].ptr, stream=st)      # outside the capture
                    G.synchronize(st)
                    graph.launch()
                    out = bytes(d_out.download(len(plain)))
                    for p in range(n):                                          # record p under the client's (even p) or the server's slot of master p
                        key, iv4 = _keys(hl, gens[g][p], key_len)[p % 2]
                        assert out[off[p]:off[p + 1]] == _protect12(key, iv4, seqs[p], recs[p]), (g, p)
            assert mt.status() == (hip.OK, 0) and kt.status() == (hip.OK, 0)
        finally:
            for b in [d_idx, d_cs, d_ss, d_all, d_pslots, d_seq, d_off, d_in, d_out] + [x for g in d_m for x in g]:
                b.free()
    G.stream_destroy(st)


def test_captured_export_srtp_install_and_encrypt_replays_over_changed_masters(hip):
    n, hl, key_len, kind = 100, 48, 32, S.RTCP
    gens = [_masters(90 + g, n) for g in range(3)]
    pkts = [_plain_srtp(kind, p, 9 + p % 23) for p in range(n)]
    off = [0]
    for r in pkts:
        off.append(off[-1] + len(r))
    plain = b"".join(pkts)
    st = G.stream_create()
    with hip.MasterSecretTable(hl, n) as mt, hip.MasterKeyTable(key_len, n) as mk, hip.KeyTable(key_len, n) as kt:
        d_all, d_off = _up(hip, _u32(list(range(n)))), _up(hip, _u64(off))
        d_in, d_out = _up(hip, plain), _up(hip, bytes(len(plain)))
        d_m = [[_up(hip, b"".join(m[k] for m in g)) for k in range(3)] for g in gens]
        fmt = hip.SrtpFormat.rtcp()

        def enqueue():
            mt.export_srtp_dev(mk, n, d_all.ptr, None, d_all.ptr, stream=st)     # the server's keys of master p into record p
            mk.install_dev(hip.SRTP_RTCP, kt, n, d_all.ptr, d_all.ptr, None, stream=st)
            kt.srtp_crypt_dev(0, fmt, n, d_all.ptr, d_in.ptr, d_off.ptr, d_out.ptr, stream=st)

        try:
            mt.set_dev(n, d_all.ptr, d_m[0][0].ptr, d_m[0][1].ptr, d_m[0][2].ptr, stream=st)
            enqueue()
            G.synchronize(st)
            with G.Graph(st, enqueue) as graph:
                for g in range(3):
                    mt.set_dev(n, d_all.ptr, d_m[g][0].ptr, d_m[g][1].ptr, d_m[g][2].ptr, stream=st)
                    G.synchronize(st)
                    graph.launch()
                    out = bytes(d_out.download(len(plain)))
                    for p in range(n):
                        key, salt = K.session(kind, *_exported(hl, gens[g][p], key_len)[1], 0)
                        assert out[off[p]:off[p + 1]] == S.protect(kind, key, salt, 0, pkts[p]), (g, p)
            assert mt.status() == (hip.OK, 0) and mk.status() == (hip.OK, 0) and kt.status() == (hip.OK, 0)
        finally:
            for b in [d_all, d_off, d_in, d_out] + [x for g in d_m for x in g]:
                b.free()
    G.stream_destroy(st)


# ---------------------------------------------------------------- the loop on one stream
def test_set_dev_install_assign_encrypt_decrypt_on_one_stream(hip):
    """a client's sending side and its peer's receiving side: masters from device memory (odd addresses), keys installed, sequence numbers assigned into the explicit
    nonces, records encrypted under the client's slots and decrypted under the same keys in a second table that a second install filled -- no host synchronisation
    between the launches"""
    n, hl, key_len, per = 33, 48, 32, 3
    masters = _masters(111, n)
    npk = n * per
    recs = [_plain12(p, 0) for p in range(npk)]
    off = [0]
    for r in recs:
        off.append(off[-1] + len(r))
    plain = b"".join(recs)
    st = G.stream_create()
    with hip.MasterSecretTable(hl, n) as mt, hip.KeyTable(key_len, n) as tx, hip.KeyTable(key_len, n) as rx, hip.TxCounters(n, npk) as tc:
        tc.set(0, [100 + i for i in range(n)], [1 << 40] * n)
        d_all = _up(hip, _u32(list(range(n))))
        d_m = [_up(hip, b"\xEE" + b"".join(m[k] for m in masters)) for k in range(3)]
        d_ctr = _up(hip, _u32([p // per for p in range(npk)]))
        d_off, d_num, d_auth = _up(hip, _u64(off)), _up(hip, bytes(8 * npk)), _up(hip, bytes(4 * npk))
        d_buf, d_wire, d_back = _up(hip, plain), _up(hip, bytes(len(plain))), _up(hip, bytes(len(plain)))
        fmt = hip.TlsFormat.tls12()
        try:
            tx.set(0, bytes(key_len))                                           # one ordinary call per table before the loop (per-device state)
            mt.set_dev(n, d_all.ptr, d_m[0].ptr + 1, d_m[1].ptr + 1, d_m[2].ptr + 1, stream=st)
            mt.install_dev(tx, n, d_all.ptr, d_all.ptr, None, stream=st)         # the client's write keys: its sending table
            mt.install_dev(rx, n, d_all.ptr, d_all.ptr, None, stream=st)         # ... and the server's receiving table
            tc.assign_dev(hip.TxFormat.tls12(), npk, d_ctr.ptr, d_buf.ptr, d_off.ptr, d_num.ptr, stream=st)
            tx.records_crypt_dev(0, fmt, npk, d_ctr.ptr, d_num.ptr, d_buf.ptr, d_off.ptr, d_wire.ptr, stream=st)
            rx.records_crypt_dev(1, fmt, npk, d_ctr.ptr, d_num.ptr, d_wire.ptr, d_off.ptr, d_back.ptr, d_auth=d_auth.ptr, stream=st)
            G.synchronize(st)
            wire, back = bytes(d_wire.download(len(plain))), bytes(d_back.download(len(plain)))
            auth = list(struct.unpack("<%di" % npk, bytes(d_auth.download(4 * npk))))
            assert auth == [1] * npk
            for p in range(npk):
                i, seq = p // per, 100 + p // per + p % per
                key, iv4 = _keys(hl, masters[i], key_len)[0]
                numbered = recs[p][:5] + struct.pack(">Q", seq) + recs[p][13:]
                assert wire[off[p]:off[p + 1]] == _protect12(key, iv4, seq, numbered), p
                assert back[off[p]:off[p + 1]][:-16] == numbered[:-16], p
            assert mt.status() == (hip.OK, 0) and tx.status() == (hip.OK, 0) and rx.status() == (hip.OK, 0) and tc.status() == (hip.OK, 0)
        finally:
            for b in [d_all, d_ctr, d_off, d_num, d_auth, d_buf, d_wire, d_back] + d_m:
                b.free()
    G.stream_destroy(st)
