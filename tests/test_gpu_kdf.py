"""GPU: on-device key derivation (aesgcm_kdf_*).  Secrets and keys cannot be read back, so everything is checked through what the installed slots DO: one small record
per entry is encrypted on the GPU under the installed slots (crypt_records in TLS 1.3 format, crypt_quic, crypt_dtls) and must equal, every byte, the fixtures'
protection (tls_fixture / quic_fixture / dtls_fixture over libcrypto) under keys derived in Python with hmac -- header-protection and sequence-number masks included,
which is what checks the aux slot.
  install      every preset, both hashes, key sizes 16 / 24 / 32, 1 / 257 / 4097 entries (a ragged last workgroup, several workgroups), shuffled d_idx and d_slots;
               a custom format with labels of 1 and 20 bytes; the recorded TLS 1.3 connections of tests/golden/tls_records.json from OpenSSL's own traffic secrets
  update       in place, into another record, three generations, the source keeps its generation, a key update without aux slots keeps the hp slot
  refusals     one test per kind: the refused entry's slots and record as before, its neighbours installed, the secret table's status, the key table's untouched
  guards       257 entries inside tables of 259: the outer slots and records unchanged
  capture      update in place + install + encrypt in one graph, three replays = generations 1, 2, 3
  rekey loop   TxCounters refuses the tail at its limit; update, install into a fresh slot, reset, the tail under the next generation"""
import random
import struct

import pytest

import dtls_fixture as D
import hip_graph as G
import quic_fixture as Q
import tls_fixture as T
from kt_common import _u32, _u64, _up
from oracle import libcrypto_ref as R
from util import splitmix_bytes

pytestmark = pytest.mark.gpu

HASH = {32: "sha256", 48: "sha384"}
NO_SLOT = 0xFFFFFFFF


class Proto:
    """a preset: how the fixtures derive from a secret, what a record looks like, how the fixtures protect it and how the GPU does"""

    def __init__(self, name):
        self.name = name
        self.quic = name.startswith("quic")
        self.has_aux = name != "tls13"

    def fmt(self, hip):
        return getattr(hip.KdfFormat, self.name)()

    def _x(self, hl, secret, label, L):
        if self.name == "dtls13":
            return D.hkdf_expand_label13(HASH[hl], secret, label, L)
        pre = {"tls13": b"", "quic_v1": b"quic ", "quic_v2": b"quicv2 "}[self.name]
        return T.hkdf_expand_label(HASH[hl], secret, pre + label, L)

    def keys(self, hl, secret, key_len):
        aux = self._x(hl, secret, b"sn" if self.name == "dtls13" else b"hp", key_len) if self.has_aux else None
        return self._x(hl, secret, b"key", key_len), self._x(hl, secret, b"iv", 12), aux

    def next(self, hl, secret):
        return self._x(hl, secret, b"ku" if self.quic else b"traffic upd", hl)

    def plain(self, i, num):
        """entry i's record before protection: the header written, the number's low bytes in it, 16 placeholder bytes behind the payload"""
        body = splitmix_bytes(1000 + i, 20 + i % 13)
        if self.name == "tls13":
            return b"\x17\x03\x03" + struct.pack(">H", len(body) + 17) + body + b"\x17" + bytes(16)
        if self.quic:                                                           # a short header: 0 1 S R R K P P, an 8-byte connection ID, a 2-byte packet number at offset 9
            return bytes([0x41 | ((i & 1) << 2)]) + splitmix_bytes(7, 8) + struct.pack(">H", num & 0xFFFF) + body + bytes(16)
        return D.header13(b"", num, True, True, 3, len(body) + 16) + body + bytes(16)

    def protect(self, keys, num, rec):
        key, iv, aux = keys
        if self.name == "tls13":
            ct, tag = R.encrypt(key, T.nonce_of(T.TLS13, iv, num, rec), rec[:5], rec[5:-16])
            return rec[:5] + bytes(ct) + bytes(tag)
        if self.quic:
            return Q.protect(key, iv, aux, num, 9, rec)
        return D.protect13(key, iv, aux, num, 1, rec)

    def gpu(self, hip, kt, slots, aux_slots, nums, recs):
        if self.name == "tls13":
            return kt.crypt_records(hip.TlsFormat.tls13(), slots, nums, recs)[0]
        if self.quic:
            return kt.crypt_quic(slots, aux_slots, nums, [9] * len(slots), recs)[0]
        return kt.crypt_dtls(hip.DtlsFormat.dtls13(), slots, recs, sn_slots=aux_slots, seqs=nums, sn_offs=[1] * len(slots))[0]


PROTOS = {n: Proto(n) for n in ("tls13", "quic_v1", "quic_v2", "dtls13")}


def _secrets(seed, n, hl):
    return [splitmix_bytes(seed * 100003 + i, hl) for i in range(n)]


def _check(hip, pr, kt, hl, entries, label=""):
    """entries: (secret the slots should hold keys of, slot, aux slot) -- one record each on the GPU against the fixture, every byte"""
    nums = [(i * 0x9E3779B1 + 5) & 0xFFFFFFFFFF for i in range(len(entries))]
    recs = [pr.plain(i, nums[i]) for i in range(len(entries))]
    got = pr.gpu(hip, kt, [e[1] for e in entries], [e[2] for e in entries], nums, recs)
    cache = {}
    for i, (sec, _, _) in enumerate(entries):
        if sec not in cache:
            cache[sec] = pr.keys(hl, sec, kt.key_len)
        want = pr.protect(cache[sec], nums[i], recs[i])
        assert bytes(got[i]) == want, (label, pr.name, hl, kt.key_len, "entry", i)
    assert kt.status() == (hip.OK, 0), label


def _install(hip, pr, st, kt, idx, slots, aux=None, fmt=None):
    st.install(fmt or pr.fmt(hip), kt, idx, slots, aux if pr.has_aux else None)


# ---------------------------------------------------------------- install
@pytest.mark.parametrize("key_len", [16, 24, 32])
@pytest.mark.parametrize("hl", [32, 48])
@pytest.mark.parametrize("name", sorted(PROTOS))
def test_install_every_preset_hash_and_key_size(hip, name, hl, key_len):
    pr = PROTOS[name]
    for n in (1, 257, 4097):
        rng = random.Random("%s %d %d %d" % (name, hl, key_len, n))
        secrets = _secrets(n + hl + key_len, n, hl)
        idx, slots, aux = list(range(n)), list(range(n)), list(range(n, 2 * n))
        for v in (idx, slots, aux):
            rng.shuffle(v)
        with hip.SecretTable(hl, n) as st, hip.KeyTable(key_len, 2 * n) as kt:
            st.set(0, secrets)
            _install(hip, pr, st, kt, idx, slots, aux)
            assert st.status() == (hip.OK, 0)
            _check(hip, pr, kt, hl, [(secrets[idx[i]], slots[i], aux[i]) for i in range(n)], "n=%d" % n)


@pytest.mark.parametrize("hl", [32, 48])
def test_custom_labels_of_1_and_20_bytes(hip, hl):
    """the shortest and the longest label the bound allows, as key / iv and swapped; checked as TLS 1.3 records under keys from the RFC's formula on the full label"""
    import hmac
    k1, k20 = b"k", b"abcdefghijklmnopqrs" + b"\x00"                      # (a label may hold any byte)

    def x(sec, full, L):
        return hmac.new(sec, struct.pack(">HB", L, len(full)) + full + b"\0\x01", HASH[hl]).digest()[:L]

    secrets = _secrets(77 + hl, 5, hl)
    for lab_key, lab_iv in ((k1, k20), (k20, k1)):
        fmt = hip.KdfFormat.custom(lab_key, lab_iv)
        assert fmt.check() == hip.OK
        with hip.SecretTable(hl, 5) as st, hip.KeyTable(16, 5) as kt:
            st.set(0, secrets).install(fmt, kt, [4, 3, 2, 1, 0], [0, 1, 2, 3, 4])
            pr = PROTOS["tls13"]
            nums = [3, 4, 5, 6, 7]
            recs = [pr.plain(i, nums[i]) for i in range(5)]
            got = pr.gpu(hip, kt, [0, 1, 2, 3, 4], None, nums, recs)
            for i in range(5):
                sec = secrets[4 - i]
                assert bytes(got[i]) == pr.protect((x(sec, lab_key, 16), x(sec, lab_iv, 12), None), nums[i], recs[i]), (lab_key, i)


def test_recorded_tls13_connections_from_their_traffic_secrets(hip):
    """OpenSSL's own traffic secrets (tests/golden/tls_records.json) installed on the device: its records decrypt with d_auth all 1 and re-encrypt byte for byte"""
    dirs = [d for d in T.directions() if d[2] == T.TLS13]
    assert dirs
    seen = set()
    for conn, who, ver, key, iv, recs in dirs:
        hl, kl = {"sha256": 32, "sha384": 48}[conn["hash"]], conn["key_len"]
        seen.add((hl, kl))
        with hip.SecretTable(hl, 1) as st, hip.KeyTable(kl, 1) as kt:
            st.set(0, bytes.fromhex(conn["dirs"][who]["traffic_secret"])).install(hip.KdfFormat.tls13(), kt, [0], [0])
            seqs, wire = [r[0] for r in recs], [r[1] for r in recs]
            back, auth = kt.crypt_records(hip.TlsFormat.tls13(), [0] * len(recs), seqs, wire, decrypt=True)
            assert auth == [1] * len(recs), (who, auth)
            for b, (_, w, pt) in zip(back, recs):
                assert bytes(b)[5:-16] == pt
            again, _ = kt.crypt_records(hip.TlsFormat.tls13(), [0] * len(recs), seqs, [bytes(b)[:-16] + bytes(16) for b in back])
            assert [bytes(a) for a in again] == wire
    assert len(seen) >= 1


# ---------------------------------------------------------------- update
@pytest.mark.parametrize("hl", [32, 48])
@pytest.mark.parametrize("name", ["tls13", "quic_v1", "dtls13", "quic_v2"])
def test_update_in_place_into_another_record_and_three_generations(hip, name, hl):
    pr = PROTOS[name]
    fmt = pr.fmt(hip)
    n = 70
    g0 = _secrets(500 + hl, n, hl)
    g1 = [pr.next(hl, s) for s in g0]
    g2 = [pr.next(hl, s) for s in g1]
    g3 = [pr.next(hl, s) for s in g2]
    with hip.SecretTable(hl, 2 * n) as st, hip.KeyTable(16, 4 * n) as kt:
        st.set(0, g0)
        # out of place: records n .. 2n - 1 become generation 1, the sources still install generation 0
        st.update(fmt, list(range(n)), list(range(n, 2 * n)))
        assert st.status() == (hip.OK, 0)
        _install(hip, pr, st, kt, list(range(2 * n)), list(range(2 * n)), list(range(2 * n, 4 * n)))
        _check(hip, pr, kt, hl, [((g0 + g1)[i], i, 2 * n + i) for i in range(2 * n)], "out of place")
        # in place, twice: records n .. become generations 2 and 3; each installed and checked
        for gen in (g2, g3):
            st.update(fmt, list(range(n, 2 * n)), list(range(n, 2 * n)))
            _install(hip, pr, st, kt, list(range(n, 2 * n)), list(range(n)), list(range(2 * n, 3 * n)))
            _check(hip, pr, kt, hl, [(gen[i], i, 2 * n + i) for i in range(n)], "in place")
        assert st.status() == (hip.OK, 0)


@pytest.mark.parametrize("name", ["quic_v1", "dtls13"])
def test_key_update_without_aux_slots_leaves_the_hp_slot_working(hip, name):
    """RFC 9001 6: the header-protection key does not change with a key update.  install with d_aux_slots = NULL (and with 0xFFFFFFFF entries) writes no aux slot"""
    pr, hl = PROTOS[name], 32
    fmt = pr.fmt(hip)
    g0 = _secrets(900, 3, hl)
    g1 = [pr.next(hl, s) for s in g0]
    with hip.SecretTable(hl, 3) as st, hip.KeyTable(32, 9) as kt:
        st.set(0, g0).install(fmt, kt, [0, 1, 2], [0, 1, 2], [6, 7, 8])
        st.update(fmt, [0, 1, 2], [0, 1, 2])
        st.install(fmt, kt, [0, 1, 2], [3, 4, 5])                               # the next phase's AEAD slots; no aux slots named
        nums = [10, 11, 12]
        recs = [pr.plain(i, nums[i]) for i in range(3)]
        got = pr.gpu(hip, kt, [3, 4, 5], [6, 7, 8], nums, recs)
        for i in range(3):
            key, iv, _ = pr.keys(hl, g1[i], 32)
            assert bytes(got[i]) == pr.protect((key, iv, pr.keys(hl, g0[i], 32)[2]), nums[i], recs[i]), i
        # the same with an array of 0xFFFFFFFF, but one entry that does name its aux slot
        st.install(fmt, kt, [0, 1, 2], [3, 4, 5], [NO_SLOT, 7, NO_SLOT])
        assert st.status() == (hip.OK, 0)
        got = pr.gpu(hip, kt, [3, 4, 5], [6, 7, 8], nums, recs)
        for i in range(3):
            key, iv, aux1 = pr.keys(hl, g1[i], 32)
            assert bytes(got[i]) == pr.protect((key, iv, aux1 if i == 1 else pr.keys(hl, g0[i], 32)[2]), nums[i], recs[i]), i


# ---------------------------------------------------------------- refusals
@pytest.mark.parametrize("kind", ["idx out of range", "record unset", "record cleared", "slot out of range", "aux slot out of range"])
def test_install_refusal_skips_the_entry_whole(hip, kind):
    pr, hl = PROTOS["quic_v1"], 32
    fmt = pr.fmt(hip)
    old = _secrets(31, 2, hl)                                                    # what the victim's slots hold before the call
    new = _secrets(32, 4, hl)
    with hip.SecretTable(hl, 8) as st, hip.KeyTable(16, 10) as kt:
        st.set(0, old).set(4, new[:3])                                           # records 0, 1 old; 4, 5, 6 new; 2, 3, 7 unset
        st.install(fmt, kt, [0, 1], [4, 5], [6, 7])                              # victim slot 4 / aux 6 hold old[0]'s keys; slot 5 / aux 7 old[1]'s
        idx, slots, aux = [4, 5, 6], [0, 4, 2], [1, 6, 3]
        if kind == "idx out of range":
            idx[1] = 8
        elif kind == "record unset":
            idx[1] = 7
        elif kind == "record cleared":
            st.clear(5)
        elif kind == "slot out of range":
            slots[1] = 10
        else:
            aux[1] = 10
        st.install(fmt, kt, idx, slots, aux)
        assert st.status() == (hip.EARG, 1) and st.status() == (hip.OK, 0)       # the lowest index; reading clears
        assert kt.status() == (hip.OK, 0)                                        # the key table's own status is not touched
        # the neighbours are installed; everything the refused entry names is as before: slot 4 with aux 6 still old[0]'s keys
        _check(hip, pr, kt, hl, [(new[0], 0, 1), (new[2], 2, 3), (old[0], 4, 6), (old[1], 5, 7)], kind)
        if kind != "record cleared":                                             # ... and its record still installs what it held
            st.install(fmt, kt, [5], [8], [9])
            _check(hip, pr, kt, hl, [(new[1], 8, 9)], kind)
        # two refused entries: the lowest is named
        st.install(fmt, kt, [4, 9, 6, 9], [0, 4, 2, 5], [1, 6, 3, 7])
        assert st.status() == (hip.EARG, 1)


@pytest.mark.parametrize("kind", ["from out of range", "to out of range", "from unset", "from cleared"])
def test_update_refusal_leaves_the_target_record_alone(hip, kind):
    pr, hl = PROTOS["tls13"], 48
    fmt = pr.fmt(hip)
    s = _secrets(41, 4, hl)
    with hip.SecretTable(hl, 6) as st, hip.KeyTable(32, 6) as kt:
        st.set(0, s)                                                             # records 0 .. 3 set; 4, 5 unset
        frm, to = [0, 1, 2], [0, 3, 2]                                           # entry 1: record 1 -> record 3
        if kind == "from out of range":
            frm[1] = 6
        elif kind == "to out of range":
            to[1] = 6
        elif kind == "from unset":
            frm[1] = 5
        else:
            st.clear(1)
        st.update(fmt, frm, to)
        assert st.status() == (hip.EARG, 1) and st.status() == (hip.OK, 0)
        st.install(fmt, kt, [0, 2, 3], [0, 2, 3])
        _check(hip, pr, kt, hl, [(pr.next(hl, s[0]), 0, None), (pr.next(hl, s[2]), 2, None), (s[3], 3, None)], kind)      # the neighbours stepped, record 3 as before
        if kind != "from cleared":
            st.install(fmt, kt, [1], [1])
            _check(hip, pr, kt, hl, [(s[1], 1, None)], kind)                     # ... and the source too


# ---------------------------------------------------------------- guards
@pytest.mark.parametrize("name,hl,key_len", [("tls13", 32, 16), ("quic_v1", 48, 32)])
def test_guard_slots_and_records_around_257_entries(hip, name, hl, key_len):
    pr = PROTOS[name]
    fmt = pr.fmt(hip)
    n = 257
    rng = random.Random("guards " + name)
    secrets = _secrets(61, 259, hl)
    with hip.SecretTable(hl, 259) as st, hip.KeyTable(key_len, 2 * 259) as kt:
        st.set(0, secrets[:258])                                                 # record 258 stays unset; record 0 is set and never named
        st.install(fmt, kt, [0], [0], [259] if pr.has_aux else None)             # slot 0 (aux 259) set with record 0's keys; slot 258 (aux 517) stays unset
        idx, slots = list(range(1, 258)), list(range(1, 258))
        rng.shuffle(idx)
        rng.shuffle(slots)
        aux = [259 + s for s in slots]
        _install(hip, pr, st, kt, idx, slots, aux)
        st.update(fmt, idx, idx)
        assert st.status() == (hip.OK, 0)
        _check(hip, pr, kt, hl, [(secrets[idx[i]], slots[i], aux[i]) for i in range(n)] + [(secrets[0], 0, 259)], "inside and the set guard")
        # the unset guard slot still refuses its packet: the record comes back as it went in
        rec = pr.plain(0, 9)
        out = pr.gpu(hip, kt, [258], [517], [9], [rec])
        assert bytes(out[0]) == rec and kt.status() == (hip.EARG, 0)
        # the records: 0 still holds its first generation, 258 is still unset, the inner ones stepped once
        _install(hip, pr, st, kt, [0, 258, idx[0]], [0, 258, 1], [259, 517, 260])
        assert st.status() == (hip.EARG, 1)
        _check(hip, pr, kt, hl, [(secrets[0], 0, 259), (pr.next(hl, secrets[idx[0]]), 1, 260)], "records")
        out = pr.gpu(hip, kt, [258], [517], [9], [rec])
        assert bytes(out[0]) == rec and kt.status() == (hip.EARG, 0)


# ---------------------------------------------------------------- capture
def test_captured_update_install_encrypt_replays_three_generations(hip):
    """update_dev in place, install_dev and records_crypt_dev (encrypt) captured on one created stream after one ordinary call of each; three replays give the
    fixture's records under generations 1, 2 and 3"""
    pr, hl, n = PROTOS["tls13"], 48, 300
    fmt, tf = pr.fmt(hip), hip.TlsFormat.tls13()
    g = [_secrets(71, n, hl)]
    for _ in range(3):
        g.append([pr.next(hl, s) for s in g[-1]])
    nums = list(range(100, 100 + n))
    recs = [pr.plain(i, nums[i]) for i in range(n)]
    off = [0]
    for r in recs:
        off.append(off[-1] + len(r))
    plain = b"".join(recs)
    perm = list(range(n))
    random.Random(5).shuffle(perm)
    st = G.stream_create()
    with hip.SecretTable(hl, n) as sec, hip.KeyTable(32, n) as kt:
        d_idx, d_slots, d_seq, d_off = _up(hip, _u32(perm)), _up(hip, _u32(perm)), _up(hip, _u64(nums)), _up(hip, _u64(off))
        d_rec_slots = _up(hip, _u32(list(range(n))))
        d_in, d_out = _up(hip, plain), _up(hip, bytes(len(plain)))

        def enqueue():
            sec.update_dev(fmt, n, d_idx.ptr, d_idx.ptr, stream=st)
            sec.install_dev(fmt, kt, n, d_idx.ptr, d_slots.ptr, stream=st)
            kt.records_crypt_dev(0, tf, n, d_rec_slots.ptr, d_seq.ptr, d_in.ptr, d_off.ptr, d_out.ptr, stream=st)

        try:
            sec.set(0, g[0], stream=st)
            enqueue()                                                           # the ordinary call of each
            G.synchronize(st)
            sec.set(0, g[0], stream=st)                                         # back to generation 0, outside the capture
            G.synchronize(st)
            with G.Graph(st, enqueue) as graph:
                for gen in (1, 2, 3):
                    graph.launch()
                    out = bytes(d_out.download(len(plain)))
                    for i in range(n):
                        want = pr.protect(pr.keys(hl, g[gen][i], 32), nums[i], recs[i])
                        assert out[off[i]:off[i + 1]] == want, (gen, i)
            assert sec.status() == (hip.OK, 0) and kt.status() == (hip.OK, 0)
        finally:
            for b in (d_idx, d_slots, d_seq, d_off, d_rec_slots, d_in, d_out):
                b.free()
    G.stream_destroy(st)


# ---------------------------------------------------------------- the rekey loop
def test_rekey_loop_with_send_counters(hip):
    """a counter's limit refuses the tail of a call; update, install into a fresh slot, reset the counter, assign and encrypt the refused tail: every record is the
    fixture's under the generation it was sent in"""
    pr, hl, n, limit = PROTOS["tls13"], 32, 40, 25
    fmt, tf = pr.fmt(hip), hip.TlsFormat.tls13()
    g0 = _secrets(81, 1, hl)[0]
    g1 = pr.next(hl, g0)
    with hip.SecretTable(hl, 1) as st, hip.KeyTable(16, 2) as kt, hip.TxCounters(1, n) as tc:
        st.set(0, g0).install(fmt, kt, [0], [0])
        tc.set(0, [0], [limit])
        _, nums, _, refused = tc.assign(hip.TxFormat.number_only(), [0] * n)
        assert refused == [False] * limit + [True] * (n - limit) and nums[:limit] == list(range(limit))
        assert tc.status() == (hip.EARG, limit)
        recs = [pr.plain(i, 0) for i in range(n)]
        sent = kt.crypt_records(tf, [0] * limit, nums[:limit], recs[:limit])[0]
        # the key update: the next secret, its keys into the unused slot, the counter from 0 again
        st.update(fmt, [0], [0]).install(fmt, kt, [0], [1])
        tc.set(0, [0], [limit])
        _, nums2, _, refused2 = tc.assign(hip.TxFormat.number_only(), [0] * (n - limit))
        assert refused2 == [False] * (n - limit) and nums2 == list(range(n - limit))
        sent += kt.crypt_records(tf, [1] * (n - limit), nums2, recs[limit:])[0]
        kt.clear(0)                                                             # the old slot is retired
        k0, k1 = pr.keys(hl, g0, 16), pr.keys(hl, g1, 16)
        for i in range(n):
            want = pr.protect(k0, nums[i], recs[i]) if i < limit else pr.protect(k1, nums2[i - limit], recs[i])
            assert bytes(sent[i]) == want, i
        assert st.status() == (hip.OK, 0) and kt.status() == (hip.OK, 0)


# ---------------------------------------------------------------- calls that need a table
def test_set_dev_clear_and_argument_errors_with_a_table(hip):
    pr, hl = PROTOS["dtls13"], 48
    fmt = pr.fmt(hip)
    s = _secrets(91, 3, hl)
    with hip.SecretTable(hl, 4) as st, hip.KeyTable(24, 8) as kt, hip.KeyTable(24, 1) as small:
        d_idx, d_sec = _up(hip, _u32([2, 9, 0])), _up(hip, b"\xEE" + b"".join(s))      # (an odd address: d_secrets has no alignment to keep)
        try:
            st.set_dev(3, d_idx.ptr, d_sec.ptr + 1)
            hip.dev_sync()
            assert st.status() == (hip.EARG, 1)                                  # record 9 does not exist
            st.install(fmt, kt, [2, 0], [0, 1], [4, 5])
            _check(hip, pr, kt, hl, [(s[0], 0, 4), (s[2], 1, 5)], "set_dev")
            st.clear(2)
            st.install(fmt, kt, [2, 0], [2, 3], [6, 7])
            assert st.status() == (hip.EARG, 0)
            _check(hip, pr, kt, hl, [(s[2], 3, 7)], "cleared")
            for call in (lambda: st.set(4, s[0]), lambda: st.set(3, s[0] + s[1]), lambda: st.clear(4), lambda: st.clear(0, 5), lambda: st.set(0, b"x" * 47)):
                with pytest.raises(hip.AesGcmError):
                    call()
            with pytest.raises(hip.AesGcmError):
                st.install(hip.KdfFormat.tls13(), kt, [0], [0], [1])             # aux slots with a format that has no label 2
            st.install(fmt, small, [0], [0], [1])                                # an aux slot outside a smaller table: refused on the device
            assert st.status() == (hip.EARG, 0)
        finally:
            d_idx.free()
            d_sec.free()
