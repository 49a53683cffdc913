"""GPU: TLS records in wire format through key tables (aesgcm_keytab_records_crypt_dev) -- TLS 1.3 (RFC 8446 5.2 / 5.3: nonce = write IV XOR the 64-bit sequence
number, AAD = the record header) and TLS 1.2 AES-GCM (RFC 5288 3 / RFC 5246 6.2.3.3: nonce = write IV | explicit nonce, AAD = seq | type, version | length).
1. the records of a real TLS stack (tests/golden/tls_records.json, keys derived in tests/tls_fixture.py) decrypt to their plaintext and are reproduced byte for byte;
2. random populations against libcrypto (oracle/evp_batch.c, evp_frames_crypt: nonce and AAD of every record built in tls_fixture.py from the RFCs' formulas), every
byte of the buffer compared, guard bytes included; 3. every kernel shape on lengths either side of its lane count; 4. where the sequence number goes; 5. the slot's
IV: its life cycle, the place it shares with the XPN state, stream ordering; 6. refusals, containment, tampering and aesgcm_wipe_failed_dev."""
import random
import struct

import pytest

import tls_fixture as T
from kt_common import CANARY, _collect, _layout, _u32, _u64, _up, evp  # noqa: F401
from kt_common import tls_ref_encrypt as _ref_encrypt
from util import splitmix_bytes

pytestmark = pytest.mark.gpu

SPECIAL = (16385, 0, 17, 1, 15, 16, 31, 32, 33, 255, 1400)
SEQS = (0, 2 ** 32 - 1, 2 ** 32, 2 ** 64 - 1)


def _fmt(hip, ver):
    return hip.TlsFormat.tls13() if ver == T.TLS13 else hip.TlsFormat.tls12()


def _make_records(rng, ver, n, seed, lens=None, max_payload=2048, aligned=False):
    """n plaintext records: random header (and explicit nonce), payload, the tag's bytes as placeholders.  Without lens: random lengths up to max_payload, the SPECIAL
    ones first as far as n goes.  aligned: every record a multiple of 16 bytes long"""
    h = T.HDR[ver]
    if lens is None:
        lens = [rng.randrange(0, max_payload + 1) for _ in range(n)]
        for i, x in enumerate(SPECIAL[:n]):
            lens[i] = x
        rng.shuffle(lens)
    if aligned:
        lens = [x + (-(h + x + 16)) % 16 for x in lens]
    blob = splitmix_bytes(seed, sum(lens) + n * h)
    recs, at = [], 0
    for x in lens:
        recs.append(blob[at:at + h + x] + b"\xAA" * 16)
        at += h + x
    return recs


def _make_seqs(rng, n):
    seqs = [rng.getrandbits(64) for _ in range(n)]
    if n >= 4:
        for i, p in enumerate(rng.sample(range(n), 4)):
            seqs[p] = SEQS[i]
    else:
        seqs[0] = SEQS[3 if n == 1 else 2]
    return seqs


def _run(hip, kt, decrypt, ver, slots, seqs, off, buf, inplace, out_fill=CANARY, sync=True):
    n = len(slots)
    d = {"slots": _up(hip, _u32(slots)), "in": _up(hip, buf), "off": _up(hip, _u64(off)), "seq": _up(hip, _u64(seqs))}
    d["out"] = d["in"] if inplace else _up(hip, bytes([out_fill]) * len(buf))
    d["auth"] = _up(hip, b"\x07" * 4 * n) if decrypt else None
    kt.records_crypt_dev(decrypt, _fmt(hip, ver), n, d["slots"].ptr, d["seq"].ptr, d["in"].ptr, d["off"].ptr, d["out"].ptr, d_auth=d["auth"].ptr if decrypt else None)
    d["nbytes"], d["n"] = len(buf), n
    return _collect(hip, d) if sync else d


def _table(hip, key_len, n_slots, seed):
    keys = splitmix_bytes(seed, key_len * n_slots)
    ib = splitmix_bytes(seed + 1, 12 * n_slots)
    ivs = [ib[12 * s:12 * s + 12] for s in range(n_slots)]
    kt = hip.KeyTable(key_len, n_slots)
    kt.set(0, keys)
    kt.set_tls_iv(0, ib)
    return kt, keys, ivs


def _both_ways(hip, evp, kt, keys, ivs, key_len, ver, slots, seqs, recs, lead, inplace):
    """encrypt against libcrypto, every byte of the buffer; then libcrypto's records back to the plaintext with every tag accepted (the tag's bytes stay)"""
    n = len(recs)
    off, buf = _layout(recs, lead)
    want = _ref_encrypt(evp, key_len, keys, ivs, ver, slots, seqs, recs)
    _, want_buf = _layout(want, lead)
    out, _, _ = _run(hip, kt, False, ver, slots, seqs, off, buf, inplace)
    if out != want_buf:                                                  # name the first record that differs
        for p in range(n):
            assert out[off[p]:off[p + 1]] == want[p], (p, len(recs[p]), seqs[p])
    assert out == want_buf
    back, auth, _ = _run(hip, kt, True, ver, slots, seqs, off, want_buf, inplace)
    _, plain_buf = _layout([r[:-16] + w[-16:] for r, w in zip(recs, want)], lead)
    assert back == plain_buf
    assert auth == [1] * n
    assert kt.status() == (hip.OK, 0)


# ---------------------------------------------------------------- 1. the records of a real TLS stack
@pytest.mark.parametrize("inplace", [True, False])
def test_records_of_a_real_tls_stack(hip, inplace):
    """no libcrypto here: the wire bytes are OpenSSL's own record layer's, the plaintext is seeded"""
    dirs = T.directions()
    for c in range(0, len(dirs), 2):                                     # a connection: its two directions are two slots of one table
        conn, _, ver, _, _, _ = dirs[c]
        with hip.KeyTable(conn["key_len"], 2) as kt:
            kt.set(0, dirs[c][3] + dirs[c + 1][3])
            kt.set_tls_iv(0, [dirs[c][4], dirs[c + 1][4]])
            slots, seqs, wire, plain = [], [], [], []
            for s in (0, 1):
                for seq, rec, pt in dirs[c + s][5]:
                    slots.append(s); seqs.append(seq); wire.append(rec); plain.append(pt)
            n, h = len(wire), T.HDR[ver]
            assert all(len(r) == h + len(pt) + 16 for r, pt in zip(wire, plain))
            off, wbuf = _layout(wire, 3)
            back, auth, _ = _run(hip, kt, True, ver, slots, seqs, off, wbuf, inplace)
            assert auth == [1] * n, conn["suite"]
            assert back == _layout([r[:h] + pt + r[-16:] for r, pt in zip(wire, plain)], 3)[1], conn["suite"]
            # the recorded header (and explicit nonce) with the plaintext in place, the tag's bytes placeholders: the recorded record, byte for byte
            _, pbuf = _layout([r[:h] + pt + b"\xAA" * 16 for r, pt in zip(wire, plain)], 3)
            out, _, _ = _run(hip, kt, False, ver, slots, seqs, off, pbuf, inplace)
            assert out == wbuf, conn["suite"]
            assert kt.status() == (hip.OK, 0)


# ---------------------------------------------------------------- 2. random populations against libcrypto, every byte compared
POPULATIONS = [(ver, key_len, n, n_slots) for ver in (T.TLS13, T.TLS12) for key_len in (16, 24, 32) for n, n_slots in ((1, 1), (7, 3), (4096, 64))]


@pytest.mark.parametrize("i, ver, key_len, n, n_slots", [(i,) + c for i, c in enumerate(POPULATIONS)])
def test_random_records_vs_libcrypto(hip, evp, i, ver, key_len, n, n_slots):
    aligned, inplace = i % 2 == 1, (i // 2) % 2 == 0                      # byte-packed and at 16-byte boundaries, in place and out of place, across the cases
    rng = random.Random("tls %d %d %d" % (ver, key_len, n))
    kt, keys, ivs = _table(hip, key_len, n_slots, 0x2F00 + 16 * ver + key_len + n)
    try:
        slots = [rng.randrange(n_slots) for _ in range(n)]
        slots[0], slots[-1] = 0, n_slots - 1
        recs = _make_records(rng, ver, n, 0x2F10 + n + key_len + ver, aligned=aligned)
        _both_ways(hip, evp, kt, keys, ivs, key_len, ver, slots, _make_seqs(rng, n), recs, 32 if aligned else 13, inplace)
    finally:
        kt.close()


# ---------------------------------------------------------------- 3. every kernel shape
@pytest.mark.parametrize("lanes", [8, 16, 64])
@pytest.mark.parametrize("ver, key_len", [(T.TLS13, 32), (T.TLS12, 32), (T.TLS13, 16), (T.TLS12, 24)])
def test_forced_shapes_vs_libcrypto(hip, evp, lanes, ver, key_len):
    """the debug build's batch_lanes knob; a record is one AAD block and its payload blocks, G = lanes of them per turn of the loop: payloads of G - 2, G - 1 and G
    blocks (and 2G - 1, 2G), one byte less and one more, lie either side of a whole number of turns"""
    with hip.debug_library() as dbg:
        dbg.force(batch_lanes=lanes)
        rng = random.Random("tls shape %d %d" % (lanes, ver))
        edge = [16 * m + d for m in (lanes - 2, lanes - 1, lanes, 2 * lanes - 1, 2 * lanes) for d in (-1, 0, 1)]
        n, n_slots = 150, 9
        lens = edge + [rng.randrange(0, 701) for _ in range(n - len(edge))]
        rng.shuffle(lens)
        kt, keys, ivs = _table(hip, key_len, n_slots, 0x2E00 + lanes + ver)
        try:
            slots = [rng.randrange(n_slots) for _ in range(n)]
            recs = _make_records(rng, ver, n, 0x2E10 + lanes, lens=lens)
            _both_ways(hip, evp, kt, keys, ivs, key_len, ver, slots, _make_seqs(rng, n), recs, 7, lanes == 16)
        finally:
            kt.close()


# ---------------------------------------------------------------- 4. where the number goes
@pytest.mark.parametrize("ver", [T.TLS13, T.TLS12])
def test_the_sequence_number_enters_nonce_or_aad(hip, evp, ver):
    rng = random.Random(40 + ver)
    key_len, n_slots, n = 32, 8, 200
    h = T.HDR[ver]
    kt, keys, ivs = _table(hip, key_len, n_slots, 0x2D00 + ver)
    try:
        slots = [rng.randrange(n_slots) for _ in range(n)]
        seqs = _make_seqs(rng, n)
        recs = _make_records(rng, ver, n, 0x2D10, lens=[rng.randrange(16, 300) for _ in range(n)])           # at least one block of payload each
        off, buf = _layout(recs, 3)
        want = _ref_encrypt(evp, key_len, keys, ivs, ver, slots, seqs, recs)
        a, _, _ = _run(hip, kt, False, ver, slots, seqs, off, buf, True)
        assert a == _layout(want, 3)[1]
        for bit in (0, 31, 32, 63):                                       # either half of the number
            flipped = [s ^ (1 << bit) for s in seqs]
            b, _, _ = _run(hip, kt, False, ver, slots, flipped, off, buf, True)
            for p in range(n):
                fa, fb = a[off[p]:off[p + 1]], b[off[p]:off[p + 1]]
                assert fa[:h] == fb[:h] == recs[p][:h]
                assert fa[-16:] != fb[-16:], (bit, p)
                if ver == T.TLS13:
                    assert fa[h:-16] != fb[h:-16], (bit, p)               # another nonce: another keystream
                else:
                    assert fa[h:-16] == fb[h:-16], (bit, p)               # the same nonce: the number is authenticated, nothing else
        # decrypt with one bit of the number wrong on chosen records: exactly those fail
        wrong = {0: 0, 1: 63, 77: 32, 150: 31, n - 1: 33}
        seqw = [s ^ (1 << wrong[p]) if p in wrong else s for p, s in enumerate(seqs)]
        back, auth, _ = _run(hip, kt, True, ver, slots, seqw, off, a, False, out_fill=0x3C)
        assert auth == [0 if p in wrong else 1 for p in range(n)]
        for p in range(n):
            if p not in wrong:
                assert back[off[p]:off[p + 1] - 16] == recs[p][:-16], p
        assert kt.status() == (hip.OK, 0)
    finally:
        kt.close()


@pytest.mark.parametrize("ver", [T.TLS13, T.TLS12])
def test_the_header_length_bytes(hip, evp, ver):
    """TLS 1.2's AAD takes the payload length from the offsets: a flipped header length byte changes nothing but itself.  TLS 1.3's AAD is the header: it fails"""
    rng = random.Random(42 + ver)
    key_len, n_slots, n = 16, 4, 64
    kt, keys, ivs = _table(hip, key_len, n_slots, 0x2C00 + ver)
    try:
        slots = [rng.randrange(n_slots) for _ in range(n)]
        seqs = _make_seqs(rng, n)
        recs = _make_records(rng, ver, n, 0x2C10, max_payload=200)
        want = _ref_encrypt(evp, key_len, keys, ivs, ver, slots, seqs, recs)
        off, wbuf = _layout(want, 5)
        hit = {p: 3 + (p & 1) for p in range(0, n, 3)}                    # the two length bytes of the header, in turn
        tam = bytearray(wbuf)
        for p, b in hit.items():
            tam[off[p] + b] ^= 0x40
        back, auth, _ = _run(hip, kt, True, ver, slots, seqs, off, bytes(tam), False, out_fill=0x3C)
        if ver == T.TLS12:
            assert auth == [1] * n
            plain = bytearray(_layout([r[:-16] + w[-16:] for r, w in zip(recs, want)], 5)[1])
            for p, b in hit.items():
                plain[off[p] + b] ^= 0x40
            assert back[5:-37] == bytes(plain[5:-37])
            # ... and encrypting under a flipped length byte gives the same payload and tag
            pt = bytearray(_layout(recs, 5)[1])
            for p, b in hit.items():
                pt[off[p] + b] ^= 0x40
            out, _, _ = _run(hip, kt, False, ver, slots, seqs, off, bytes(pt), True)
            assert out == bytes(tam)
        else:
            assert auth == [0 if p in hit else 1 for p in range(n)]
        assert kt.status() == (hip.OK, 0)
    finally:
        kt.close()


# ---------------------------------------------------------------- 5. the slot's IV
def test_tls_iv_life_cycle(hip, evp):
    """zero when fresh and after clear; survives set, set_dev and set_salt; shares its place with the XPN state: either setter overwrites the other"""
    rng = random.Random(50)
    key_len, n_slots, n = 24, 4, 48
    keys = splitmix_bytes(0x2B00, key_len * n_slots)
    ib = splitmix_bytes(0x2B01, 12 * n_slots)
    ivs = [ib[12 * s:12 * s + 12] for s in range(n_slots)]
    zero = [bytes(12)] * n_slots
    slots = [p % n_slots for p in range(n)]
    seqs = _make_seqs(rng, n)
    for ver in (T.TLS13, T.TLS12):
        recs = _make_records(rng, ver, n, 0x2B10, max_payload=120)
        off, buf = _layout(recs, 0)

        def ref(k, v):
            return _layout(_ref_encrypt(evp, key_len, k, v, ver, slots, seqs, recs), 0)[1]

        def got(kt):
            return _run(hip, kt, False, ver, slots, seqs, off, buf, True)[0]

        with hip.KeyTable(key_len, n_slots) as kt:
            kt.set(0, keys)
            kt.set_salt(0, splitmix_bytes(0x2B02, 8 * n_slots))             # (the classic salt is not the TLS IV)
            assert got(kt) == ref(keys, zero)
            kt.set_tls_iv(0, ivs)                                           # a list of entries
            assert got(kt) == ref(keys, ivs)
            new_keys = splitmix_bytes(0x2B20, key_len * n_slots)
            kt.set(0, new_keys)                                             # new keys by set and by set_dev, another salt: the IV stays
            d_slots, d_keys = _up(hip, _u32([2])), _up(hip, keys[:key_len])
            kt.set_dev(1, d_slots.ptr, d_keys.ptr)
            kt.set_salt(0, bytes(8 * n_slots))
            mixed = new_keys[:2 * key_len] + keys[:key_len] + new_keys[3 * key_len:]
            assert got(kt) == ref(mixed, ivs)
            kt.clear(1, 2)
            kt.set(1, mixed[key_len:3 * key_len])                           # slots 1 and 2 again: their IV is zero now
            part = [ivs[0], bytes(12), bytes(12), ivs[3]]
            assert got(kt) == ref(mixed, part)
            kt.set_tls_iv(2, ivs[2])                                        # one slot, as bytes
            part[2] = ivs[2]
            assert got(kt) == ref(mixed, part)
            # set_xpn writes the same 16 bytes: its salt is the IV now
            xs = splitmix_bytes(0x2B30, 12)
            kt.set_xpn(3, xs, b"\x01\x02\x03\x04")
            part[3] = xs
            assert got(kt) == ref(mixed, part)
            # ... and set_tls_iv overwrites the XPN state, SSCI included: an XPN frame under slot 3 sees the salt ivs[3] and the SSCI 0
            kt.set_tls_iv(3, ivs[3])
            part[3] = ivs[3]
            assert got(kt) == ref(mixed, part)
            xf = hip.WireFormatX.macsec_xpn()
            frame = splitmix_bytes(0x2B40, 28 + 50) + bytes(16)
            (enc,), _ = kt.crypt_frames(xf, [3], [frame], hi=[7])
            nonce = bytes(a ^ b for a, b in zip(ivs[3], bytes(4) + struct.pack(">I", 7) + frame[16:20]))
            from oracle import libcrypto_ref as R
            ct, tag = R.encrypt(mixed[3 * key_len:], nonce, frame[:28], frame[28:-16])
            assert enc == frame[:28] + bytes(ct) + bytes(tag)
            assert kt.status() == (hip.OK, 0)


def test_set_tls_iv_and_crypt_are_stream_ordered(hip, evp):
    key_len, n_slots, n, ver = 32, 8, 300, T.TLS13
    kt, keys, ivs = _table(hip, key_len, n_slots, 0x2A00)
    try:
        rng = random.Random(51)
        recs = _make_records(rng, ver, n, 0x2A10, max_payload=600)
        slots = [rng.randrange(n_slots) for _ in range(n)]
        seqs = _make_seqs(rng, n)
        off, buf = _layout(recs, 2)
        ivb = [bytes(x ^ 0x5A for x in v) for v in ivs]
        d1 = _run(hip, kt, False, ver, slots, seqs, off, buf, False, sync=False)
        kt.set_tls_iv(0, ivb)                                               # the null stream throughout, nothing waited for
        d2 = _run(hip, kt, False, ver, slots, seqs, off, buf, False, sync=False)
        kt.set_tls_iv(3, [ivs[3]])
        d3 = _run(hip, kt, False, ver, slots, seqs, off, buf, False, sync=False)
        r1, r2, r3 = _collect(hip, d1)[0], _collect(hip, d2)[0], _collect(hip, d3)[0]
        ivc = list(ivb)
        ivc[3] = ivs[3]
        for got, v in ((r1, ivs), (r2, ivb), (r3, ivc)):
            assert got == _layout(_ref_encrypt(evp, key_len, keys, v, ver, slots, seqs, recs), 2)[1]
        assert kt.status() == (hip.OK, 0)
    finally:
        kt.close()


# ---------------------------------------------------------------- 6. refusals and containment
@pytest.mark.parametrize("ver", [T.TLS13, T.TLS12])
@pytest.mark.parametrize("case", ["short", "long", "unset", "cleared", "slot_range", "falling"])
def test_refused_records(hip, evp, case, ver):
    rng = random.Random("%s %d" % (case, ver))
    key_len, n_slots, n = 24, 16, 60
    h = T.HDR[ver]
    kt, keys, ivs = _table(hip, key_len, n_slots, 0x2900)
    try:
        slots = [rng.randrange(1, n_slots) for _ in range(n)]
        seqs = _make_seqs(rng, n)
        recs = _make_records(rng, ver, n, 0x2910, max_payload=200)
        refused = set()
        if case == "short":
            recs[7] = recs[7][:h + 15]                                       # 20 bytes (1.3), 28 (1.2): one less than the shortest record
            recs[31] = b""
            recs[32] = recs[32][:1]
            assert len(recs[7]) == (20 if ver == T.TLS13 else 28)
            refused = {7, 31, 32}
        elif case == "long":
            recs[20] = splitmix_bytes(0x2920, 5 + 65536)                     # one byte more than the wire's length field can say
            recs[21] = splitmix_bytes(0x2921, 5 + 65535 - 16) + b"\xAA" * 16     # the longest record there is: taken
            refused = {20}
        elif case == "unset":
            kt.close()
            kt = hip.KeyTable(key_len, n_slots)
            kt.set(1, keys[key_len:])                                        # slot 0 never set
            kt.set_tls_iv(0, ivs)                                            # an IV alone does not make a slot usable
            slots[12] = slots[40] = 0
            refused = {12, 40}
        elif case == "cleared":
            kt.clear(5, 2)
            slots = [s if s not in (5, 6) else 7 for s in slots]
            slots[3], slots[4], slots[59] = 5, 6, 6
            refused = {3, 4, 59}
        elif case == "slot_range":
            slots[9], slots[10], slots[50] = n_slots, 0xFFFFFFFF, n_slots + 77
            refused = {9, 10, 50}
        off, buf = _layout(recs, 11)
        if case == "falling":
            # the last two entries: [A, A - 3) falls, [A - 3, A + 7) is too short -- both refused; the bytes they name belong to record n - 3 and to nobody
            off[n - 1] = off[n - 2] - 3
            off[n] = off[n - 1] + 10
            refused = {n - 2, n - 1}
        ok = [p for p in range(n) if p not in refused]
        ref = dict(zip(ok, _ref_encrypt(evp, key_len, keys, ivs, ver, [slots[p] for p in ok], [seqs[p] for p in ok], [recs[p] for p in ok])))
        for inplace, fill in ((True, None), (False, 0x3C)):
            want = bytearray(buf if inplace else bytes([fill]) * len(buf))
            for p in ok:
                want[off[p]:off[p + 1]] = ref[p]
            out, _, _ = _run(hip, kt, False, ver, slots, seqs, off, buf, inplace, out_fill=fill or 0)
            assert out == bytes(want), (case, inplace)
            assert kt.status() == (hip.EARG, min(refused)), case
            assert kt.status() == (hip.OK, 0)
            enc = bytearray(buf)
            for p in ok:
                enc[off[p]:off[p + 1]] = ref[p]
            back, auth, _ = _run(hip, kt, True, ver, slots, seqs, off, bytes(enc), inplace, out_fill=fill or 0)
            assert auth == [0 if p in refused else 1 for p in range(n)], case
            wantp = bytearray(enc if inplace else bytes([fill]) * len(buf))
            for p in ok:
                wantp[off[p]:off[p + 1]] = recs[p][:-16] + ref[p][-16:]
            assert back == bytes(wantp), (case, inplace)
            assert kt.status() == (hip.EARG, min(refused)), case
    finally:
        kt.close()


@pytest.mark.parametrize("ver", [T.TLS13, T.TLS12])
def test_containment_tampering_and_wipe(hip, evp, ver):
    """a padded layout -- guard bytes in front of, behind and between the records, which the offsets express as refused one-to-nineteen-byte records of their own --
    is touched nowhere but inside the accepted records; a flipped payload, tag or header bit fails that record alone; aesgcm_wipe_failed_dev zeroes exactly those"""
    rng = random.Random(61 + ver)
    key_len, n_slots, m = 32, 5, 40
    h = T.HDR[ver]
    kt, keys, ivs = _table(hip, key_len, n_slots, 0x2700 + ver)
    try:
        real = _make_records(rng, ver, m, 0x2710, lens=[rng.randrange(1, 400) for _ in range(m)])
        rslots = [rng.randrange(n_slots) for _ in range(m)]
        rseqs = _make_seqs(rng, m)
        want = _ref_encrypt(evp, key_len, keys, ivs, ver, rslots, rseqs, real)
        # records at even indices, gaps of 1 .. 19 guard bytes at odd ones (too short to be records: refused, untouched)
        gaps = [bytes([CANARY]) * rng.randrange(1, 20) for _ in range(m)]
        recs = [x for pair in zip(real, gaps) for x in pair]
        encs = [x for pair in zip(want, gaps) for x in pair]
        slots = [s for s in rslots for _ in (0, 1)]
        seqs = [s for s in rseqs for _ in (0, 1)]
        n = 2 * m
        off, buf = _layout(recs, 9)
        _, ebuf = _layout(encs, 9)
        for inplace in (True, False):
            out, _, _ = _run(hip, kt, False, ver, slots, seqs, off, buf, inplace)
            assert out == ebuf, inplace                                   # every guard byte is still CANARY (out of place: the fill)
            assert kt.status() == (hip.EARG, 1)
        tam = bytearray(ebuf)
        hits = {0: h, 4: -1, 10: 0, 20: 2, 2 * m - 2: -16, 30: h + 1}        # payload, the tag's last and first byte, header bytes (type, version)
        if ver == T.TLS12:
            hits[36] = 5                                                   # the explicit nonce
        for p, b in hits.items():
            tam[(off[p] if b >= 0 else off[p + 1]) + b] ^= 0x01
        back, auth, d = _run(hip, kt, True, ver, slots, seqs, off, bytes(tam), False, out_fill=0x3C)
        assert auth == [1 if p % 2 == 0 and p not in hits else 0 for p in range(n)]
        for p in range(0, n, 2):
            if p not in hits:
                assert back[off[p]:off[p + 1]] == recs[p][:-16] + encs[p][-16:], p
        for p in range(1, n, 2):
            assert back[off[p]:off[p + 1]] == b"\x3C" * len(recs[p]), p
        assert back[:9] == b"\x3C" * 9 and back[off[n]:] == b"\x3C" * 37
        hip.wipe_failed_dev(n, d["out"].ptr, d["auth"].ptr, d_data_off=d["off"].ptr)
        hip.dev_sync()
        wiped = bytes(d["out"].download(len(ebuf)))
        for p in range(n):
            if auth[p]:
                assert wiped[off[p]:off[p + 1]] == back[off[p]:off[p + 1]], p
            else:
                assert wiped[off[p]:off[p + 1]] == bytes(off[p + 1] - off[p]), p
        assert wiped[:9] == b"\x3C" * 9 and wiped[off[n]:] == b"\x3C" * 37
        assert kt.status() == (hip.EARG, 1)
    finally:
        kt.close()


def test_call_level_refusals_with_a_table_and_crypt_records(hip, evp):
    key_len, n_slots = 16, 3
    kt, keys, ivs = _table(hip, key_len, n_slots, 0x2600)
    try:
        d = _up(hip, bytes(256))
        for f in (hip.TlsFormat.tls13(), hip.TlsFormat.tls12()):
            with pytest.raises(hip.AesGcmError) as e:
                kt.records_crypt_dev(False, f, 1, d.ptr, None, d.ptr, d.ptr, d.ptr)                     # no d_seq
            assert e.value.code == hip.EARG
            with pytest.raises(hip.AesGcmError) as e:
                kt.records_crypt_dev(True, f, 1, d.ptr, d.ptr, d.ptr, d.ptr, d.ptr)                     # decrypt without d_auth
            assert e.value.code == hip.EARG
        with pytest.raises(hip.AesGcmError) as e:
            kt.records_crypt_dev(False, hip.TlsFormat(3, 0), 1, d.ptr, d.ptr, d.ptr, d.ptr, d.ptr)
        assert e.value.code == hip.EARG
        with pytest.raises(hip.AesGcmError) as e:
            kt.set_tls_iv(2, bytes(24))                                                              # past the last slot
        assert e.value.code == hip.EARG
        # the host convenience
        rng = random.Random(62)
        for ver in (T.TLS13, T.TLS12):
            recs = _make_records(rng, ver, 12, 0x2610, max_payload=90)
            slots = [p % n_slots for p in range(12)]
            seqs = _make_seqs(rng, 12)
            out, auth = kt.crypt_records(_fmt(hip, ver), slots, seqs, recs)
            assert auth is None and out == _ref_encrypt(evp, key_len, keys, ivs, ver, slots, seqs, recs)
            back, auth = kt.crypt_records(_fmt(hip, ver), slots, seqs, out, decrypt=True)
            assert auth == [1] * 12 and [b[:-16] for b in back] == [r[:-16] for r in recs]
        hip.dev_sync()
        assert kt.status() == (hip.OK, 0)
    finally:
        kt.close()
