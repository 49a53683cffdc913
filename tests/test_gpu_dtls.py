"""GPU: DTLS records in wire format through key tables (aesgcm_keytab_dtls_crypt_dev; DTLS 1.3: RFC 9147 -- AEAD with the unified header as AAD and the record sequence
number in the nonce, then record-number encryption; DTLS 1.2: RFC 6347 / RFC 5288 -- epoch and sequence number taken from the record) against tests/dtls_fixture.py,
which is written from the RFCs over libcrypto and does not know the library.  Every byte of a canaried arena is compared: lead and trail guard bytes, and out of place
the fill, with the output 5 bytes off the input.
1. both versions, three key sizes, both directions, in place and out of place: by the library's own choice of shape, with 8 / 16 / 64 lanes forced, and under the launch
ordered by length class; 2. the DTLS 1.3 grid: sample address mod 16 x sequence length x L bit x CID length, decoding that wraps up, wraps down and stays, d_seq_out
aliased to d_seq in one leg; 3. the DTLS 1.2 grid: every payload start mod 16 x lengths 0 .. 33; 4. forged tags, containment and aesgcm_wipe_failed_dev; 5. every refusal
kind, one record each among good ones; 6. the DTLS 1.2 records that OpenSSL sent (tests/golden/dtls12_records.json), decrypted and re-encrypted.  DTLS 1.3 has no such
witness: it is held to the RFC's formulas."""
import random
import struct

import pytest

import dtls_fixture as D
from kt_common import CANARY, TRAIL, _u32, _u64, _up
from util import splitmix_bytes

pytestmark = pytest.mark.gpu

V13, V12 = D.DTLS13, D.DTLS12
SHIFT = 5
FILL = 0x3C
SEQ_SENTINEL = 0x7777777777777777
POISON = 0xDEADDEADDEADDEAD
CIDS = (0, 1, 7, 20)


class Keys:
    """what the table's slots hold: n_aead AEAD slots (key and IV) followed by n_sn record-number slots (key only) -- the host's copy, made without a device"""

    def __init__(self, key_len, n_aead, n_sn, seed):
        self.key_len, self.n_aead, self.n_sn = key_len, n_aead, n_sn
        self.kb = splitmix_bytes(seed, key_len * (n_aead + n_sn))
        self.ib = splitmix_bytes(seed + 1, 12 * n_aead)
        self.keys = [self.kb[key_len * s:key_len * (s + 1)] for s in range(n_aead + n_sn)]
        self.ivs = [self.ib[12 * s:12 * s + 12] for s in range(n_aead)]

    def table(self, hip, extra=0):
        """a key table of the library in force holding them (extra: slots that are never set)"""
        kt = hip.KeyTable(self.key_len, self.n_aead + self.n_sn + extra)
        kt.set(0, self.kb)
        kt.set_tls_iv(0, self.ib)
        return kt


class Pop:
    """n plaintext records of one version and what the fixture makes of them.  1.3: unified header (CID bytes random, the truncated number written, the L bit's two bytes
    random: they are not interpreted) | payload | 0xAA where the tag goes; 1.2: hdr[13] | explicit nonce[8] | payload | 0xAA x 16"""

    def __init__(self, ver, keys, rng, lens, seed, cids=None, s16=None, wlen=None, seqs=None, exps=None):
        n = self.n = len(lens)
        self.ver, self.keys = ver, keys
        self.slots = [rng.randrange(keys.n_aead) for _ in range(n)]
        self.slots[0], self.slots[-1] = 0, keys.n_aead - 1
        blob = splitmix_bytes(seed, sum(lens) + 32 * n)
        self.pkts, at = [], 0
        if ver == V13:
            self.sns = [keys.n_aead + rng.randrange(keys.n_sn) for _ in range(n)]
            self.sns[0], self.sns[-1] = keys.n_aead + keys.n_sn - 1, keys.n_aead
            cids = list(cids) if cids is not None else [rng.choice(CIDS) for _ in range(n)]
            s16 = list(s16) if s16 is not None else [rng.randrange(2) for _ in range(n)]
            wlen = list(wlen) if wlen is not None else [rng.randrange(2) for _ in range(n)]
            self.seqs = list(seqs) if seqs is not None else [rng.getrandbits(rng.choice((8, 16, 48, 64))) for _ in range(n)]
            self.sn_offs = [1 + c for c in cids]
            for p, x in enumerate(lens):
                h = bytearray(D.header13(blob[at:at + cids[p]], self.seqs[p], s16[p], wlen[p], rng.randrange(4), 0))
                if wlen[p]:
                    h[-2:] = blob[at + 20:at + 22]
                self.pkts.append(bytes(h) + blob[at + 32:at + 32 + x] + b"\xAA" * 16)
                at += 32 + x
            # an expected number from which the record's own decodes: at most min(half a window - 1, 100) below it
            self.exps = list(exps) if exps is not None else [max(0, q - rng.randrange(0, (100 if b else 127) + 1)) for q, b in zip(self.seqs, s16)]
            self.hdrs = [D.hdr_len13(r, o) for r, o in zip(self.pkts, self.sn_offs)]
        else:
            for p, x in enumerate(lens):
                h = D.header12(20 + p % 6, rng.getrandbits(16), rng.getrandbits(48), x)
                self.pkts.append(h + blob[at:at + 8] + blob[at + 32:at + 32 + x] + b"\xAA" * 16)
                at += 32 + x
            self.hdrs = [21] * n
        self._wire = None

    def protect(self, p, rec=None):
        k, r = self.keys, self.pkts[p] if rec is None else rec
        if self.ver == V13:
            return D.protect13(k.keys[self.slots[p]], k.ivs[self.slots[p]], k.keys[self.sns[p]], self.seqs[p], self.sn_offs[p], r)
        return D.protect12(k.keys[self.slots[p]], k.ivs[self.slots[p]], r)

    def unprotect(self, p, rec, expected=None):
        """-> (bytes, seq or None, ok)"""
        k = self.keys
        if self.ver == V13:
            return D.unprotect13(k.keys[self.slots[p]], k.ivs[self.slots[p]], k.keys[self.sns[p]], self.exps[p] if expected is None else expected, self.sn_offs[p], rec)
        b, ok = D.unprotect12(k.keys[self.slots[p]], k.ivs[self.slots[p]], rec)
        return b, None, ok

    def wire(self):
        """the fixture's protected records (computed once, never changed)"""
        if self._wire is None:
            self._wire = [self.protect(p) for p in range(self.n)]
        return self._wire

    def clear(self):
        """what decrypting wire() leaves: header and plaintext, the tag's bytes as they came"""
        return [r[:-16] + w[-16:] for r, w in zip(self.pkts, self.wire())]


def _layout(pkts, lead):
    off = [lead]
    for r in pkts:
        off.append(off[-1] + len(r))
    return off, bytes([CANARY]) * lead + b"".join(pkts) + bytes([CANARY]) * (TRAIL + SHIFT)


def _run(hip, kt, pop, decrypt, off, buf, shift=None, slots=None, sns=None, seqs=None, sn_offs=None, alias=False):
    """one call.  shift None: in place; else out of place into a buffer of FILL, the output `shift` bytes off the input.  -> (the output buffer from the input's first
    byte's counterpart on, auth, seq_out, device buffers)"""
    n, v13 = len(off) - 1, pop.ver == V13
    fmt = hip.DtlsFormat.dtls13() if v13 else hip.DtlsFormat.dtls12()
    d = {"slots": _up(hip, _u32(pop.slots if slots is None else slots)), "in": _up(hip, buf), "off": _up(hip, _u64(off))}
    assert d["in"].ptr % 16 == 0
    d["out"] = d["in"] if shift is None else _up(hip, bytes([FILL]) * (len(buf) + 16))
    d["auth"] = _up(hip, b"\x07" * 4 * n) if decrypt else None
    kw = {}
    d["seq_out"] = None
    if v13:
        d["sn"], d["sn_off"] = _up(hip, _u32(pop.sns if sns is None else sns)), _up(hip, _u32(pop.sn_offs if sn_offs is None else sn_offs))
        d["seq"] = _up(hip, _u64(seqs if seqs is not None else pop.exps if decrypt else pop.seqs))
        if decrypt:
            d["seq_out"] = d["seq"] if alias else _up(hip, _u64([SEQ_SENTINEL] * n))
        kw = dict(d_sn_slots=d["sn"].ptr, d_seq=d["seq"].ptr, d_sn_off=d["sn_off"].ptr, d_seq_out=d["seq_out"].ptr if decrypt else None)
    d["out_ptr"] = d["out"].ptr + (shift or 0)
    kt.dtls_crypt_dev(decrypt, fmt, n, d["slots"].ptr, d["in"].ptr, d["off"].ptr, d["out_ptr"], d_auth=d["auth"].ptr if decrypt else None, **kw)
    hip.dev_sync()
    whole = bytes(d["out"].download(len(buf) + (16 if shift is not None else 0)))
    if shift is not None:
        assert whole[:shift] == bytes([FILL]) * shift and whole[shift + len(buf):] == bytes([FILL]) * (16 - shift), "bytes around the shifted output overwritten"
        assert bytes(d["in"].download(len(buf))) == buf, "the input of an out-of-place call changed"
        whole = whole[shift:shift + len(buf)]
    auth = list(struct.unpack("<%di" % n, bytes(d["auth"].download(4 * n)))) if decrypt else None
    seq_out = list(struct.unpack("<%dQ" % n, bytes(d["seq_out"].download(8 * n)))) if d["seq_out"] is not None else None
    return whole, auth, seq_out, d


def _want(buf, off, recs, shift):
    """the arena with recs[p] (None: untouched) in place of record p: in place over buf, out of place over FILL"""
    w = bytearray(buf if shift is None else bytes([FILL]) * len(buf))
    for p, r in enumerate(recs):
        if r is not None:
            assert len(r) == off[p + 1] - off[p]
            w[off[p]:off[p + 1]] = r
    return bytes(w)


def _first_difference(got, want, off):
    x = next((i for i in range(len(want)) if got[i] != want[i]), None)
    if x is None:
        return "lengths %d / %d" % (len(got), len(want))
    for p in range(len(off) - 1):
        if off[p] <= x < off[p + 1]:
            return "byte %d of record %d (%d bytes): %02x, wanted %02x" % (x - off[p], p, off[p + 1] - off[p], got[x], want[x])
    return "byte %d, outside the records: %02x, wanted %02x" % (x, got[x], want[x])


def _both_ways(hip, kt, pop, lead, shift, alias=False):
    """protect against the fixture, every byte of the arena; then the fixture's records back: header (1.3: unprotected), plaintext, the tag's bytes as they were, every tag
    accepted and every number decoded"""
    n = pop.n
    off, buf = _layout(pop.pkts, lead)
    _, wbuf = _layout(pop.wire(), lead)
    out, _, _, _ = _run(hip, kt, pop, False, off, buf, shift)
    want = _want(buf, off, pop.wire(), shift)
    assert out == want, _first_difference(out, want, off)
    back, auth, seq_out, _ = _run(hip, kt, pop, True, off, wbuf, shift, alias=alias)
    assert auth == [1] * n, [p for p in range(n) if auth[p] != 1][:8]
    if pop.ver == V13:
        assert seq_out == pop.seqs, [(p, seq_out[p], pop.seqs[p], pop.exps[p]) for p in range(n) if seq_out[p] != pop.seqs[p]][:4]
    wantp = _want(wbuf, off, pop.clear(), shift)
    assert back == wantp, _first_difference(back, wantp, off)
    assert kt.status() == (hip.OK, 0)


# ---------------------------------------------------------------- 1. populations: every instance of k_kt_dtls and k_kt_dtls_sn
_POPS = {}


def _population(ver, key_len):
    """about 300 records over 5 AEAD slots (1.3: and 3 sn slots): payload lengths 0 .. 48, and for G = 8, 16 and 64 lanes per record the lengths that make G - 1, G and
    G + 1 blocks of AAD and payload together, ending a byte into a block, on its last byte and a byte past it.  Built once per version and key size, never changed"""
    if (ver, key_len) not in _POPS:
        rng = random.Random("dtls pop %d %d" % (ver, key_len))
        keys = Keys(key_len, 5, 3 if ver == V13 else 0, 0xD700 + 16 * ver + key_len)
        lens = list(range(49))
        for G in (8, 16, 64):
            for total in (G - 1, G, G + 1):
                for n_aad in (1, 2):
                    for d in (-15, 0, 1):
                        lens.append(16 * (total - n_aad) + d)
        lens += [rng.randrange(0, 300) for _ in range(300 - len(lens))]
        rng.shuffle(lens)
        pop = Pop(ver, keys, rng, lens, 0xD710 + 16 * ver + key_len)
        if ver == V13:
            assert {(c, s, w) for c, s, w in zip([o - 1 for o in pop.sn_offs], [r[0] & 8 for r in pop.pkts], [r[0] & 4 for r in pop.pkts])} >= {(c, s, w) for c in CIDS for s in (0, 8) for w in (0, 4)}
        pop.wire()
        _POPS[ver, key_len] = pop
    return _POPS[ver, key_len]


SHAPES = ["own", "lanes8", "lanes16", "lanes64", "ordered8", "ordered16"]


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("key_len", [16, 24, 32])
@pytest.mark.parametrize("ver", [V13, V12])
def test_records_vs_fixture(hip, ver, key_len, shape):
    """encrypt and decrypt, in place and with the output 5 bytes off the input, by the library's own choice of shape, with the lanes per record forced (the debug
    library's batch_lanes), and under the launch ordered by falling length class (batch_order = 1, which the 8- and 16-lane shapes take)"""
    pop = _population(ver, key_len)

    def legs():
        with pop.keys.table(hip) as kt:
            _both_ways(hip, kt, pop, 3, None)
            _both_ways(hip, kt, pop, 3, SHIFT)
    if shape == "own":
        legs()
    else:
        with hip.debug_library() as dbg:
            if shape.startswith("ordered"):
                dbg.force(batch_lanes=int(shape[7:]), batch_order=1)
            else:
                dbg.force(batch_lanes=int(shape[5:]))
            legs()


# ---------------------------------------------------------------- 2. the DTLS 1.3 grid
def _fit(pos, front, residue):
    """the payload length 0 .. 15 of a filler record that starts at pos with `front` bytes in front of its payload, so that the record behind it starts at `residue` mod 16"""
    return (residue - (pos + front + 16)) % 16


@pytest.mark.parametrize("key_len", [16, 32])
def test_dtls13_grid(hip, key_len):
    """every sample address mod 16 x sequence length 1 | 2 x L bit x CID length 0, 1, 7, 20 -- a filler record in front of each cell puts it there; the expected numbers make
    the decode wrap upwards, wrap downwards and stay in turn; the second leg writes the decoded numbers over the expected ones"""
    rng = random.Random("dtls13 grid %d" % key_len)
    keys = Keys(key_len, 4, 2, 0xD800 + key_len)
    lead = 2
    lens, cids, s16, wlen, seqs, exps, cells = [], [], [], [], [], [], []
    pos = lead
    kinds = set()
    for res in range(16):
        for s in (0, 1):
            for w in (0, 1):
                for c in CIDS:
                    hdr = 1 + c + (2 if s else 1) + (2 if w else 0)
                    x = _fit(pos, 2, (res - hdr) % 16)                            # the filler: no CID, one sequence byte: a header of 2
                    lens.append(x); cids.append(0); s16.append(0); wlen.append(0); seqs.append(rng.getrandbits(40)); exps.append(max(0, seqs[-1] - 5))
                    pos += 2 + x + 16
                    assert (pos + hdr) % 16 == res
                    n = rng.randrange(0, 40)
                    win = 1 << (16 if s else 8)
                    base = rng.getrandbits(44) * win + 4 * win
                    kind = len(cells) % 3
                    q, e = ((base + 5, base + 9), (base + win + 1, base + win - 2), (base - 2, base + 1))[kind]
                    cand = (e & ~(win - 1)) | (q & (win - 1))
                    kinds.add((kind, (D.decode_seq(e, q & (win - 1), 8 * (2 if s else 1)) - cand) // win))
                    cells.append(len(lens))
                    lens.append(n); cids.append(c); s16.append(s); wlen.append(w); seqs.append(q); exps.append(e)
                    pos += hdr + n + 16
    assert kinds == {(0, 0), (1, 1), (2, -1)} and len(cells) == 256
    pop = Pop(V13, keys, rng, lens, 0xD810, cids=cids, s16=s16, wlen=wlen, seqs=seqs, exps=exps)
    off, _ = _layout(pop.pkts, lead)
    assert {((off[p] + pop.hdrs[p]) % 16, pop.pkts[p][0] & 8, pop.pkts[p][0] & 4, pop.sn_offs[p] - 1) for p in cells} == \
        {(r, s, w, c) for r in range(16) for s in (0, 8) for w in (0, 4) for c in CIDS}
    with keys.table(hip) as kt:
        _both_ways(hip, kt, pop, lead, None)
        _both_ways(hip, kt, pop, lead, SHIFT, alias=True)


# ---------------------------------------------------------------- 3. the DTLS 1.2 grid
@pytest.mark.parametrize("key_len", [16, 32])
def test_dtls12_grid(hip, key_len):
    """every payload start mod 16 x payload lengths 0 .. 33, a filler record in front of each cell"""
    rng = random.Random("dtls12 grid %d" % key_len)
    keys = Keys(key_len, 4, 0, 0xD900 + key_len)
    lead = 1
    lens, cells, pos = [], [], lead
    for res in range(16):
        for n in range(34):
            x = _fit(pos, 21, (res - 21) % 16)
            lens.append(x)
            pos += 37 + x
            assert (pos + 21) % 16 == res
            cells.append(len(lens))
            lens.append(n)
            pos += 37 + n
    pop = Pop(V12, keys, rng, lens, 0xD910)
    off, _ = _layout(pop.pkts, lead)
    assert {((off[p] + 21) % 16, len(pop.pkts[p]) - 37) for p in cells} == {(r, n) for r in range(16) for n in range(34)}
    with keys.table(hip) as kt:
        _both_ways(hip, kt, pop, lead, None)
        _both_ways(hip, kt, pop, lead, SHIFT)


# ---------------------------------------------------------------- 4. forged tags, containment, wipe
@pytest.mark.parametrize("shift", [None, SHIFT])
@pytest.mark.parametrize("ver", [V13, V12])
def test_forged_tags_containment_and_wipe(hip, ver, shift):
    """one flipped bit in a tag's first and last byte, in the payload, in the header (1.3: a CID byte and a sequence byte; 1.2: the epoch and the explicit nonce), and for
    1.3 an expected number two windows off: that record fails and no other, its neighbours' bytes are the fixture's, nothing outside the records is written, and
    aesgcm_wipe_failed_dev zeroes exactly the failed records"""
    rng = random.Random("dtls forge %d" % ver)
    n = 60
    keys = Keys(32, 5, 3 if ver == V13 else 0, 0xDA00 + ver)
    pop = Pop(ver, keys, rng, [rng.randrange(20, 300) for _ in range(n)], 0xDA10 + ver, cids=[7] * n if ver == V13 else None)
    wire = pop.wire()
    off, wbuf = _layout(wire, 9)
    tam = bytearray(wbuf)
    exps = list(pop.exps) if ver == V13 else None
    hits = {2: "tag_first", 7: "tag_last", 11: "payload", 19: "hdr_a", 23: "hdr_b", 31: "tag_first", 32: "tag_last", 59: "payload"}
    if ver == V13:
        hits[41] = "epoch"
    for p, what in hits.items():
        L, h = len(wire[p]), pop.hdrs[p]
        at = {"tag_first": L - 16, "tag_last": L - 1, "payload": h + 3, "hdr_a": 3, "hdr_b": pop.sn_offs[p] if ver == V13 else 15}.get(what)
        if at is not None:
            tam[off[p] + at] ^= 0x80 if what == "tag_last" else 1
        else:
            exps[p] = pop.seqs[p] + (2 << (16 if pop.pkts[p][0] & 8 else 8))
    tam = bytes(tam)
    ref = [pop.unprotect(p, tam[off[p]:off[p + 1]], exps[p] if exps else None) for p in range(n)]
    assert [int(r[2]) for r in ref] == [0 if p in hits else 1 for p in range(n)]
    with keys.table(hip) as kt:
        back, auth, seq_out, d = _run(hip, kt, pop, True, off, tam, shift, seqs=exps)
        assert auth == [0 if p in hits else 1 for p in range(n)]
        if ver == V13:
            assert seq_out == [r[1] for r in ref]
        good = [r[0] if p not in hits else None for p, r in enumerate(ref)]
        for p in range(n):
            if p not in hits:
                assert back[off[p]:off[p + 1]] == good[p] == pop.clear()[p], p
        outside = bytes([CANARY if shift is None else FILL])
        assert back[:9] == outside * 9 and back[off[n]:] == outside * (TRAIL + SHIFT)
        hip.wipe_failed_dev(n, d["out_ptr"], d["auth"].ptr, d_data_off=d["off"].ptr)
        hip.dev_sync()
        wiped = bytes(d["out"].download(len(tam) + (shift or 0)))[shift or 0:]
        for p in range(n):
            assert wiped[off[p]:off[p + 1]] == (bytes(off[p + 1] - off[p]) if p in hits else back[off[p]:off[p + 1]]), p
        assert wiped[:9] == outside * 9 and wiped[off[n]:] == outside * (TRAIL + SHIFT)
        assert kt.status() == (hip.OK, 0)


# ---------------------------------------------------------------- 5. refusals
REFUSALS = [(V13, c) for c in ("aead_range", "aead_unset", "sn_range", "sn_unset", "falling", "long", "sn_off_zero", "short17", "first_byte", "sample")] + \
           [(V12, c) for c in ("aead_range", "aead_unset", "falling", "short", "long")]


@pytest.mark.parametrize("ver, case", REFUSALS)
def test_refused_records(hip, ver, case):
    """each refusal alone among good records, both directions, in place and out of place: the refused record's bytes and its seq_out are untouched, its verdict is 0, its
    d_seq holds a poisoned value, the status word names the lowest refused index and clears on reading"""
    rng = random.Random("dtls refuse %d %s" % (ver, case))
    key_len, n = 32, 40
    v13 = ver == V13
    keys = Keys(key_len, 5, 3 if v13 else 0, 0xDB00 + ver)
    n_slots = keys.n_aead + keys.n_sn + 1                                     # the last slot is never set
    lens = [rng.randrange(0, 200) for _ in range(n)]
    cids = [rng.choice(CIDS) for _ in range(n)]
    s16 = [rng.randrange(2) for _ in range(n)]
    wlen = [rng.randrange(2) for _ in range(n)]
    refused = set()
    if case == "long":
        if v13:
            cids[11], s16[11], wlen[11], lens[11] = 7, 1, 1, 65536 - 16 - 12  # L = 65536: refused
            cids[12], s16[12], wlen[12], lens[12] = 7, 1, 1, 65535 - 16 - 12  # L = 65535: the longest record there is, taken
        else:
            lens[11], lens[12] = 65549 - 37, 65548 - 37                       # L - 13 = 65536: refused; 65535: taken
        refused = {11}
    elif case == "sample":
        cids[6], s16[6], wlen[6], lens[6] = 7, 1, 1, 0                        # hdr + 16 == L: taken
        cids[7], s16[7], wlen[7] = 1, 1, 1                                    # (cut short below)
        cids[30], s16[30], wlen[30] = 20, 0, 1
        refused = {7, 30}
    elif case == "short17":
        cids[8], s16[8], wlen[8], lens[8] = 0, 0, 0, 0                        # sn_off + 17 == L: taken
        cids[9], s16[9], wlen[9] = 7, 0, 0
        refused = {9}
    elif case == "short":
        lens[5] = 0                                                           # L = 37: taken
        refused = {6, 29}
    pop = Pop(ver, keys, rng, lens, 0xDB10 + ver, cids=cids, s16=s16, wlen=wlen)
    slots, pkts = list(pop.slots), list(pop.pkts)
    sns, sn_offs = (list(pop.sns), list(pop.sn_offs)) if v13 else (None, None)
    clear = []
    if case == "long":
        assert len(pkts[11]) == (65536 if v13 else 65549) and len(pkts[12]) == (65535 if v13 else 65548)
    elif case == "aead_range":
        slots[9], slots[10], slots[33] = n_slots, 0xFFFFFFFF, n_slots + 77
        refused = {9, 10, 33}
    elif case == "aead_unset":
        pop.slots = slots = [s if s != 2 else 3 for s in slots]
        slots = list(slots)
        slots[3], slots[21] = 2, n_slots - 1                                  # cleared below, and never set
        refused, clear = {3, 21}, [2]
    elif case == "sn_range":
        sns[5], sns[6], sns[39] = n_slots, 0xFFFFFFFF, 0x80000000
        refused = {5, 6, 39}
    elif case == "sn_unset":
        pop.sns = sns = [s if s != 6 else 7 for s in sns]
        sns = list(sns)
        sns[4], sns[22] = 6, n_slots - 1
        refused, clear = {4, 22}, [6]
    elif case == "sn_off_zero":
        sn_offs[13] = 0
        refused = {13}
    elif case == "first_byte":
        for p, b0 in ((14, 0x00), (15, 0x40), (16, 0xA0), (17, 0x30 ^ 0x20 ^ 0x80)):
            pkts[p] = bytes([(pkts[p][0] & 0x1F) | b0]) + pkts[p][1:]
        refused = {14, 15, 16, 17}
    elif case == "sample":
        for p in (7, 30):                                                     # hdr + 16 == L + 1, and sn_off + 17 <= L
            pkts[p] = pkts[p][:pop.hdrs[p] + 15]
            assert sn_offs[p] + 17 <= len(pkts[p])
    elif case == "short17":
        pkts[9] = pkts[9][:sn_offs[9] + 16]                                   # sn_off + 17 == L + 1
        assert len(pkts[8]) == sn_offs[8] + 17
    elif case == "short":
        for p in (6, 29):
            pkts[p] = pkts[p][:36]
        assert len(pkts[5]) == 37
    off, buf = _layout(pkts, 11)
    if case == "falling":
        # the last two entries: [A, A - 3) falls; [A - 3, A - 3 + w) names bytes of record n - 3 and guard bytes and is too short for what its arguments say
        w = 43 if v13 else 36
        off[n - 1] = off[n - 2] - 3
        off[n] = off[n - 1] + w
        if v13:
            sn_offs[n - 1] = 39
        refused = {n - 2, n - 1}
        buf = buf + bytes([CANARY]) * 64
    ok = [p for p in range(n) if p not in refused]
    wire = {p: pop.protect(p, pkts[p]) for p in ok}
    seqs = [POISON if p in refused else pop.seqs[p] for p in range(n)] if v13 else None
    exps = [POISON if p in refused else pop.exps[p] for p in range(n)] if v13 else None
    with keys.table(hip, extra=1) as kt:
        for s in clear:
            kt.clear(s)
        for shift in (None, SHIFT):
            out, _, _, _ = _run(hip, kt, pop, False, off, buf, shift, slots=slots, sns=sns, seqs=seqs, sn_offs=sn_offs)
            want = _want(buf, off, [wire.get(p) for p in range(n)], shift)
            assert out == want, (case, shift, _first_difference(out, want, off))
            assert kt.status() == (hip.EARG, min(refused)), case
            assert kt.status() == (hip.OK, 0)
            enc = _want(buf, off, [wire.get(p) for p in range(n)], None)
            back, auth, seq_out, _ = _run(hip, kt, pop, True, off, enc, shift, slots=slots, sns=sns, seqs=exps, sn_offs=sn_offs)
            assert auth == [0 if p in refused else 1 for p in range(n)], case
            if v13:
                assert seq_out == [SEQ_SENTINEL if p in refused else pop.seqs[p] for p in range(n)], case
            wantp = _want(enc, off, [pkts[p][:-16] + wire[p][-16:] if p in wire else None for p in range(n)], shift)
            assert back == wantp, (case, shift, _first_difference(back, wantp, off))
            assert kt.status() == (hip.EARG, min(refused)), case


# ---------------------------------------------------------------- 6. the recorded OpenSSL records
@pytest.mark.parametrize("shift", [None, SHIFT])
def test_recorded_openssl_records(hip, shift):
    """every record of a connection in one call, a slot per direction: decrypted to what was written, and re-encrypted to the bytes OpenSSL sent"""
    dirs = D.directions()
    for key_len in (16, 32):
        mine = [d for d in dirs if d[0]["key_len"] == key_len]
        assert len(mine) == 2
        wire = [w for _, _, _, _, recs in mine for w, _ in recs]
        plain = [w[:21] + pt + w[-16:] for _, _, _, _, recs in mine for w, pt in recs]
        slots = [s for s, d in enumerate(mine) for _ in d[4]]

        class P:
            ver, n = V12, len(wire)
        P.slots = slots
        with hip.KeyTable(key_len, 2) as kt:
            kt.set(0, b"".join(d[2] for d in mine))
            kt.set_tls_iv(0, b"".join(d[3] for d in mine))
            off, wbuf = _layout(wire, 7)
            back, auth, _, _ = _run(hip, kt, P, True, off, wbuf, shift)
            assert auth == [1] * P.n
            want = _want(wbuf, off, plain, shift)
            assert back == want, _first_difference(back, want, off)
            _, pbuf = _layout([p[:-16] + b"\xAA" * 16 for p in plain], 7)
            out, _, _, _ = _run(hip, kt, P, False, off, pbuf, shift)
            want = _want(pbuf, off, wire, shift)
            assert out == want, _first_difference(out, want, off)
            assert kt.status() == (hip.OK, 0)


# ---------------------------------------------------------------- the host convenience
def test_crypt_dtls_host_convenience(hip):
    rng = random.Random("dtls host")
    for ver in (V13, V12):
        keys = Keys(16, 3, 2 if ver == V13 else 0, 0xDC00 + ver)
        pop = Pop(ver, keys, rng, [0, 1, 17, 100, 1400], 0xDC10 + ver)
        fmt = hip.DtlsFormat.dtls13() if ver == V13 else hip.DtlsFormat.dtls12()
        with keys.table(hip) as kt:
            kw = dict(sn_slots=pop.sns, sn_offs=pop.sn_offs) if ver == V13 else {}
            outs, auth, so = kt.crypt_dtls(fmt, pop.slots, pop.pkts, seqs=pop.seqs if ver == V13 else None, **kw)
            assert outs == pop.wire() and auth is None and so is None
            back, auth, so = kt.crypt_dtls(fmt, pop.slots, pop.wire(), decrypt=True, seqs=pop.exps if ver == V13 else None, **kw)
            assert back == pop.clear() and auth == [1] * pop.n and so == (pop.seqs if ver == V13 else None)
            assert kt.status() == (hip.OK, 0)
