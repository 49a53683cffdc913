"""GPU: QUIC packets in wire format through key tables (aesgcm_keytab_quic_crypt_dev, RFC 9001 section 5: AEAD with the header as AAD and the packet number in the nonce,
then header protection) against tests/quic_fixture.py, which is written from the RFCs with hashlib, hmac and libcrypto.  Every byte of the buffer is compared: lead and
trail guard bytes, and out of place the fill.
1. the client Initial of RFC 9001 Appendix A (its keys and header; a seeded payload); 2. random populations; 3. the shortest packets: the sample is the tag, and the sample
ends at the packet's end; 4. every kernel shape on block counts either side of its lane count; 5. packet-number decoding at the far sides of a truncation window and beside
2^62, d_pn_out aliased to d_pn; 6. refusals, each alone among good packets; 7. tampering, containment and aesgcm_wipe_failed_dev; 8. stream ordering."""
import random
import struct

import pytest

import quic_fixture as Q
from kt_common import CANARY, TRAIL, _layout, _u32, _u64, _up
from util import splitmix_bytes

pytestmark = pytest.mark.gpu

SPECIAL = (0, 1, 3, 15, 16, 17, 31, 32, 33, 255, 1200, 1452)
PNS = (0, 2 ** 32 - 1, 2 ** 32, 2 ** 62 - 1)
PN_SENTINEL = 0x7777777777777777


class Table:
    """a key table of n_aead AEAD slots (key and IV) followed by n_hp header-protection slots (key only), and the host's copy of what is in them"""

    def __init__(self, hip, key_len, n_aead, n_hp, seed, extra=0, stream=None):
        self.key_len, self.n_aead, self.n_hp = key_len, n_aead, n_hp
        kb = splitmix_bytes(seed, key_len * (n_aead + n_hp))
        ib = splitmix_bytes(seed + 1, 12 * n_aead)
        self.keys = [kb[key_len * s:key_len * (s + 1)] for s in range(n_aead + n_hp)]
        self.ivs = [ib[12 * s:12 * s + 12] for s in range(n_aead)]
        self.kt = hip.KeyTable(key_len, n_aead + n_hp + extra)                # (extra: slots that are never set)
        self.kt.set(0, kb, stream=stream)
        self.kt.set_tls_iv(0, ib, stream=stream)

    def close(self):
        self.kt.close()


class Pop:
    """n unprotected packets: first byte (long or short form, random other bits, pn_len - 1 in its low bits), random header bytes up to pn_off, the truncated packet
    number, a random payload, and 0xAA where the tag goes"""

    def __init__(self, rng, tab, n, seed, lens=None, pn_offs=None, pn_lens=None, pns=None, max_payload=2048):
        if lens is None:
            lens = [rng.randrange(0, max_payload + 1) for _ in range(n)]
            for i, x in enumerate(SPECIAL[:n]):
                lens[i] = x
            rng.shuffle(lens)
        self.n = n
        self.slots = [rng.randrange(tab.n_aead) for _ in range(n)]
        self.hps = [tab.n_aead + rng.randrange(tab.n_hp) for _ in range(n)]
        self.slots[0], self.slots[-1] = 0, tab.n_aead - 1
        self.hps[0], self.hps[-1] = tab.n_aead + tab.n_hp - 1, tab.n_aead
        self.pn_offs = list(pn_offs) if pn_offs is not None else [rng.randrange(1, 61) for _ in range(n)]
        # the sample must lie inside the packet: pn_len + payload >= 4
        self.pn_lens = list(pn_lens) if pn_lens is not None else [rng.randrange(max(1, 4 - x), 5) if x < 4 else 1 + (i + rng.randrange(2)) % 4 for i, x in enumerate(lens)]
        if pns is None:
            pns = [rng.getrandbits(rng.choice((8, 16, 31, 33, 62))) for _ in range(n)]
            if n >= 4:
                for i, p in enumerate(rng.sample(range(n), 4)):
                    pns[p] = PNS[i]
        self.pns = list(pns)
        blob = splitmix_bytes(seed, sum(lens) + sum(self.pn_offs))
        self.pkts, at = [], 0
        for p, x in enumerate(lens):
            po, pl = self.pn_offs[p], self.pn_lens[p]
            hdr = bytearray(blob[at:at + po])
            hdr[0] = (hdr[0] & 0x7C) | (pl - 1) | (0x80 if p % 3 == 1 else 0)      # long and short forms mixed; the other bits random
            trunc = (self.pns[p] & ((1 << (8 * pl)) - 1)).to_bytes(pl, "big")
            self.pkts.append(bytes(hdr) + trunc + blob[at + po:at + po + x] + b"\xAA" * 16)
            at += po + x
        self._wire = None
        self.tab = tab

    def wire(self):
        """the fixture's protected packets (computed once)"""
        if self._wire is None:
            t = self.tab
            self._wire = [Q.protect(t.keys[self.slots[p]], t.ivs[self.slots[p]], t.keys[self.hps[p]], self.pns[p], self.pn_offs[p], self.pkts[p]) for p in range(self.n)]
        return self._wire

    def expected_pns(self, rng):
        """an expected number per packet from which A.3 decodes the packet's own: at most min(half a window - 1, 100) below it"""
        return [max(0, pn - rng.randrange(0, min((1 << (8 * pl - 1)) - 1, 100) + 1)) for pn, pl in zip(self.pns, self.pn_lens)]


def _run(hip, kt, decrypt, slots, hps, pns, pn_offs, off, buf, inplace, out_fill=CANARY, alias_pn=False, stream=None, sync=True):
    n = len(slots)
    d = {"slots": _up(hip, _u32(slots)), "hps": _up(hip, _u32(hps)), "pn": _up(hip, _u64(pns)), "pn_off": _up(hip, _u32(pn_offs)), "in": _up(hip, buf), "off": _up(hip, _u64(off))}
    d["out"] = d["in"] if inplace else _up(hip, bytes([out_fill]) * len(buf))
    d["auth"] = _up(hip, b"\x07" * 4 * n) if decrypt else None
    d["pn_out"] = (d["pn"] if alias_pn else _up(hip, _u64([PN_SENTINEL] * n))) if decrypt else None
    kt.quic_crypt_dev(decrypt, n, d["slots"].ptr, d["hps"].ptr, d["pn"].ptr, d["pn_off"].ptr, d["in"].ptr, d["off"].ptr, d["out"].ptr,
                      d_pn_out=d["pn_out"].ptr if decrypt else None, d_auth=d["auth"].ptr if decrypt else None, stream=stream)
    d["nbytes"], d["n"] = len(buf), n
    return _collect(hip, d) if sync else d


def _collect(hip, d):
    hip.dev_sync()
    n = d["n"]
    out = bytes(d["out"].download(d["nbytes"]))
    auth = list(struct.unpack("<%di" % n, bytes(d["auth"].download(4 * n)))) if d["auth"] is not None else None
    pn_out = list(struct.unpack("<%dQ" % n, bytes(d["pn_out"].download(8 * n)))) if d["pn_out"] is not None else None
    return out, auth, pn_out, d


def _first_difference(got, want, off, n):
    for p in range(n):
        if got[off[p]:off[p + 1]] != want[off[p]:off[p + 1]]:
            return "packet %d of %d bytes" % (p, off[p + 1] - off[p])
    return "outside the packets"


def _both_ways(hip, pop, lead, inplace, rng, fill=0x3C):
    """protect against the fixture, every byte of the buffer; then the fixture's packets back: the unprotected header, the plaintext, the tag's bytes as they were, every
    tag accepted and every number decoded"""
    kt, n = pop.tab.kt, pop.n
    off, buf = _layout(pop.pkts, lead)
    _, wbuf = _layout(pop.wire(), lead)
    want = wbuf if inplace else bytes([fill]) * lead + wbuf[lead:len(wbuf) - TRAIL] + bytes([fill]) * TRAIL
    out, _, _, _ = _run(hip, kt, False, pop.slots, pop.hps, pop.pns, pop.pn_offs, off, buf, inplace, out_fill=fill)
    assert out == want, _first_difference(out, want, off, n)
    _, pbuf = _layout([r[:-16] + w[-16:] for r, w in zip(pop.pkts, pop.wire())], lead)
    wantp = pbuf if inplace else bytes([fill]) * lead + pbuf[lead:len(pbuf) - TRAIL] + bytes([fill]) * TRAIL
    back, auth, pn_out, _ = _run(hip, kt, True, pop.slots, pop.hps, pop.expected_pns(rng), pop.pn_offs, off, wbuf, inplace, out_fill=fill)
    assert auth == [1] * n, [p for p in range(n) if auth[p] != 1][:8]
    assert pn_out == pop.pns
    assert back == wantp, _first_difference(back, wantp, off, n)
    assert kt.status() == (hip.OK, 0)


# ---------------------------------------------------------------- 1. RFC 9001 Appendix A
@pytest.mark.parametrize("inplace", [True, False])
def test_rfc9001_client_initial(hip, inplace):
    """the Appendix A client Initial: its DCID's keys, its header, packet number 2, a seeded payload of the RFC's 1162 bytes"""
    key, iv, hp = Q.initial_keys(bytes.fromhex("8394c8f03e515708"), "client")
    assert key.hex() == "1f369613dd76d5467730efcbe3b1a22d"
    header = bytes.fromhex("c300000001088394c8f03e5157080000449e00000002")
    payload = splitmix_bytes(0x9001, 1162)
    plain = header + payload + b"\xAA" * 16
    assert len(plain) == 1200
    wire = Q.protect(key, iv, hp, 2, 18, plain)
    assert wire[1:18] == header[1:18] and wire[0] & 0xF0 == 0xC0 and len(wire) == 1200
    with hip.KeyTable(16, 2) as kt:
        kt.set(0, key + hp)
        kt.set_tls_iv(0, iv)
        off, buf = _layout([plain], 5)
        out, _, _, _ = _run(hip, kt, False, [0], [1], [2], [18], off, buf, inplace)
        assert out == _layout([wire], 5)[1]
        back, auth, pn_out, _ = _run(hip, kt, True, [0], [1], [0], [18], off, out, inplace)
        assert auth == [1] and pn_out == [2]
        assert back == _layout([header + payload + wire[-16:]], 5)[1]
        # the host convenience, both ways
        (w2,), a2, p2 = kt.crypt_quic([0], [1], [2], [18], [plain])
        assert w2 == wire and a2 is None and p2 is None
        (b2,), a2, p2 = kt.crypt_quic([0], [1], [1], [18], [wire], decrypt=True)
        assert b2[:-16] == plain[:-16] and a2 == [1] and p2 == [2]
        assert kt.status() == (hip.OK, 0)


# ---------------------------------------------------------------- 2. random populations against the fixture
_POPS = {}


def _population(hip, key_len):
    """300 packets over 7 AEAD slots and 3 hp slots, and the fixture's protected form of them: built once per key size, shared by its six cases, never changed"""
    if key_len not in _POPS:
        rng = random.Random("quic pop %d" % key_len)
        tab = Table(hip, key_len, 7, 3, 0x9100 + key_len)
        pn_offs = [1, 60] + [rng.randrange(1, 61) for _ in range(298)]
        pop = Pop(rng, tab, 300, 0x9110 + key_len, pn_offs=pn_offs)
        assert set(pop.pn_lens) == {1, 2, 3, 4} and {r[0] >> 7 for r in pop.pkts} == {0, 1} and set(PNS) <= set(pop.pns)
        assert set(SPECIAL) <= {len(r) - 16 - po - pl for r, po, pl in zip(pop.pkts, pop.pn_offs, pop.pn_lens)}
        pop.wire()
        _POPS[key_len] = pop
    return _POPS[key_len]


@pytest.mark.parametrize("lead", [0, 1, 13])
@pytest.mark.parametrize("inplace", [True, False])
@pytest.mark.parametrize("key_len", [16, 32])
def test_random_packets_vs_fixture(hip, key_len, inplace, lead):
    pop = _population(hip, key_len)
    _both_ways(hip, pop, lead, inplace, random.Random("quic exp %d %d" % (key_len, lead)))


# ---------------------------------------------------------------- 3. the shortest packets
@pytest.mark.parametrize("key_len", [16, 32])
def test_shortest_packets(hip, key_len):
    """pn_off 1, pn_len 1, payload 3: 21 bytes, the sample IS the tag.  And for every pn_len a packet whose sample ends at its end: pn_off + 20 == L"""
    rng = random.Random("quic short %d" % key_len)
    tab = Table(hip, key_len, 3, 2, 0x9200 + key_len)
    try:
        pn_offs = [1, 1, 1, 1, 1, 7, 7, 7, 7, 33, 60, 60]
        pn_lens = [1, 1, 2, 3, 4, 1, 2, 3, 4, 4, 1, 4]
        lens = [3] + [4 - pl for pl in pn_lens[1:]]
        pop = Pop(rng, tab, len(lens), 0x9210, lens=lens, pn_offs=pn_offs, pn_lens=pn_lens)
        assert len(pop.pkts[0]) == 21 and all(po + 20 == len(r) for po, r in zip(pop.pn_offs, pop.pkts))
        for inplace in (True, False):
            _both_ways(hip, pop, 3, inplace, rng)
    finally:
        tab.close()


# ---------------------------------------------------------------- 4. every kernel shape
@pytest.mark.parametrize("lanes", [8, 16, 64])
@pytest.mark.parametrize("key_len", [16, 32])
def test_forced_shapes_vs_fixture(hip, lanes, key_len):
    """the debug build's batch_lanes knob; a packet is its header's blocks and its payload's, G = lanes of them per turn of the loop: G - 1, G and G + 1 blocks (and
    2G - 1, 2G, 2G + 1), the header one, two or four of them, the payload ending on a block's last byte, a byte short of it and a byte into its last block"""
    with hip.debug_library() as dbg:
        dbg.force(batch_lanes=lanes)
        rng = random.Random("quic shape %d %d" % (lanes, key_len))
        pn_offs, pn_lens, lens = [], [], []
        for total in (lanes - 1, lanes, lanes + 1, 2 * lanes - 1, 2 * lanes, 2 * lanes + 1):
            for hb in (1, 2, 4):
                for d in (0, -1, -15):
                    pl = rng.randrange(1, 5)
                    hdr = 16 * hb - rng.randrange(0, 8)                      # header bytes: hb blocks
                    pn_offs.append(hdr - pl); pn_lens.append(pl); lens.append(16 * (total - hb) + d)
        n = 150
        fill = n - len(lens)
        assert fill > 0
        pn_offs += [rng.randrange(1, 61) for _ in range(fill)]
        pn_lens += [rng.randrange(1, 5) for _ in range(fill)]
        lens += [rng.randrange(3, 701) for _ in range(fill)]
        order = list(range(n))
        rng.shuffle(order)
        tab = Table(hip, key_len, 9, 3, 0x9300 + lanes + key_len)
        try:
            pop = Pop(rng, tab, n, 0x9310 + lanes, lens=[lens[i] for i in order], pn_offs=[pn_offs[i] for i in order], pn_lens=[pn_lens[i] for i in order])
            _both_ways(hip, pop, 7, lanes == 16, rng)
        finally:
            tab.close()


# ---------------------------------------------------------------- 5. decoding the packet number
def test_packet_number_decoding(hip):
    """expected numbers at the far sides of the truncation window (half a window above, less one; half a window below), one step beyond either side (where A.3
    decodes another number and the tag fails), and beside 2^62; d_pn_out is d_pn.  The fixture says what each must give"""
    rng = random.Random("quic decode")
    key_len = 16
    tab = Table(hip, key_len, 4, 2, 0x9400)
    try:
        pns, exps, pn_lens = [], [], []
        for pl in (1, 2, 3, 4):
            win = 1 << (8 * pl)
            hwin = win >> 1
            for pn in (rng.getrandbits(40) + win, 3 * win + 5, (1 << 62) - 1, (1 << 62) - win + 3, (1 << 62) - win - 2, hwin - 1, 0):
                for e in (pn, pn + hwin - 1, pn - hwin + 1, pn - hwin, pn + hwin, pn - hwin - 1, pn + win, pn + 1):
                    if 0 <= e < 1 << 63:
                        pns.append(pn); exps.append(e); pn_lens.append(pl)
        n = len(pns)
        pop = Pop(rng, tab, n, 0x9410, lens=[rng.randrange(3, 80) for _ in range(n)], pn_lens=pn_lens, pns=pns)
        wire = pop.wire()
        off, wbuf = _layout(wire, 2)
        ref = [Q.unprotect(tab.keys[pop.slots[p]], tab.ivs[pop.slots[p]], tab.keys[pop.hps[p]], exps[p], pop.pn_offs[p], wire[p]) for p in range(n)]
        good = [p for p in range(n) if ref[p][2]]
        assert len(good) >= n // 2 and len(good) < n                          # both kinds are there
        assert all(ref[p][1] == pns[p] for p in good)
        assert any(ref[p][1] == (1 << 62) - 1 for p in good)
        back, auth, pn_out, _ = _run(hip, tab.kt, True, pop.slots, pop.hps, exps, pop.pn_offs, off, wbuf, False, out_fill=0x3C, alias_pn=True)
        assert pn_out == [r[1] for r in ref]
        assert auth == [int(r[2]) for r in ref]
        for p in good:
            assert back[off[p]:off[p + 1]] == ref[p][0], p
        for p in range(n):                                                  # the unprotected header is there whether the tag held or not
            h = pop.pn_offs[p] + pn_lens[p]
            assert back[off[p]:off[p] + h] == pop.pkts[p][:h], p
        assert tab.kt.status() == (hip.OK, 0)
    finally:
        tab.close()


# ---------------------------------------------------------------- 6. refusals
REFUSALS = ["aead_range", "aead_unset", "hp_range", "hp_unset", "falling", "long", "pn_off_zero", "sample", "pn_2p62"]


@pytest.mark.parametrize("case", REFUSALS)
def test_refused_packets(hip, case):
    rng = random.Random("quic refuse " + case)
    key_len, n = 32, 40
    tab = Table(hip, key_len, 5, 3, 0x9500, extra=1)                          # slot 8 is never set
    kt, n_slots = tab.kt, 9
    try:
        lens = [rng.randrange(3, 200) for _ in range(n)]
        pn_offs = [rng.randrange(1, 40) for _ in range(n)]
        pn_lens = [rng.randrange(1, 5) for _ in range(n)]
        refused, enc_only = set(), False
        if case == "long":
            pn_offs[11], pn_lens[11], lens[11] = 30, 2, 65536 - 16 - 32       # L = 65536: refused
            pn_offs[12], pn_lens[12], lens[12] = 30, 2, 65535 - 16 - 32       # L = 65535: the longest packet there is, taken
            refused = {11}
        elif case == "sample":
            pn_offs[6], pn_lens[6], lens[6] = 9, 4, 0                         # pn_off + 20 == L: taken
            refused = {7, 30}                                                 # (cut short below)
        pop = Pop(rng, tab, n, 0x9510, lens=lens, pn_offs=pn_offs, pn_lens=pn_lens)
        slots, hps, pns, pn_offs = list(pop.slots), list(pop.hps), list(pop.pns), list(pop.pn_offs)
        if case == "long":
            assert len(pop.pkts[11]) == 65536 and len(pop.pkts[12]) == 65535
        if case == "aead_range":
            slots[9], slots[10], slots[33] = n_slots, 0xFFFFFFFF, n_slots + 77
            refused = {9, 10, 33}
        elif case == "aead_unset":
            kt.clear(2)
            slots = [s if s != 2 else 3 for s in slots]
            pop.slots = list(slots)
            slots[3], slots[21] = 2, 8                                        # cleared, and never set
            refused = {3, 21}
        elif case == "hp_range":
            hps[5], hps[6], hps[39] = n_slots, 0xFFFFFFFF, 0x80000000
            refused = {5, 6, 39}
        elif case == "hp_unset":
            kt.clear(6)
            hps = [s if s != 6 else 7 for s in hps]
            pop.hps = list(hps)
            hps[4], hps[22] = 6, 8
            refused = {4, 22}
        elif case == "pn_off_zero":
            pn_offs[13] = 0
            refused = {13}
        elif case == "pn_2p62":
            pns[17], pns[18], pns[19] = 1 << 62, (1 << 64) - 1, (1 << 62) - 1
            pop.pns[19] = (1 << 62) - 1
            tr = pop.pkts[19]
            h = pop.pn_offs[19]
            pop.pkts[19] = tr[:h] + ((1 << 62) - 1 & ((1 << (8 * pop.pn_lens[19])) - 1)).to_bytes(pop.pn_lens[19], "big") + tr[h + pop.pn_lens[19]:]
            refused, enc_only = {17, 18}, True
        pkts = list(pop.pkts)
        if case == "sample":
            for p in (7, 30):                                               # pn_off + 20 == L + 1: the sample's last byte is the next packet's
                pkts[p] = pkts[p][:pn_offs[p] + 19]
        off, buf = _layout(pkts, 11)
        if case == "falling":
            # the last two entries: [A, A - 3) falls, [A - 3, A + 40) names bytes of packet n - 3 and guard bytes under a header that does not fit them: at pn_off 39
            off[n - 1] = off[n - 2] - 3
            off[n] = off[n - 1] + 43
            pn_offs[n - 1] = 39
            refused = {n - 2, n - 1}
            buf = buf + bytes([CANARY]) * 64
        ok = [p for p in range(n) if p not in refused]
        wire = {p: Q.protect(tab.keys[pop.slots[p]], tab.ivs[pop.slots[p]], tab.keys[pop.hps[p]], pop.pns[p], pop.pn_offs[p], pkts[p]) for p in ok}
        for inplace, fill in ((True, None), (False, 0x3C)):
            want = bytearray(buf if inplace else bytes([fill]) * len(buf))
            for p in ok:
                want[off[p]:off[p + 1]] = wire[p]
            out, _, _, _ = _run(hip, kt, False, slots, hps, pns, pn_offs, off, buf, inplace, out_fill=fill or 0)
            assert out == bytes(want), (case, inplace, _first_difference(out, bytes(want), off, n))
            assert kt.status() == (hip.EARG, min(refused)), case
            assert kt.status() == (hip.OK, 0)
            if enc_only:
                continue
            enc = bytearray(buf)
            for p in ok:
                enc[off[p]:off[p + 1]] = wire[p]
            back, auth, pn_out, _ = _run(hip, kt, True, slots, hps, pns, pn_offs, off, bytes(enc), inplace, out_fill=fill or 0)
            assert auth == [0 if p in refused else 1 for p in range(n)], case
            assert pn_out == [PN_SENTINEL if p in refused else pns[p] for p in range(n)], case
            wantp = bytearray(enc if inplace else bytes([fill]) * len(buf))
            for p in ok:
                wantp[off[p]:off[p + 1]] = pkts[p][:-16] + wire[p][-16:]
            assert back == bytes(wantp), (case, inplace, _first_difference(back, bytes(wantp), off, n))
            assert kt.status() == (hip.EARG, min(refused)), case
    finally:
        tab.close()


# ---------------------------------------------------------------- 7. tampering, containment, wipe
@pytest.mark.parametrize("inplace", [True, False])
def test_tampering_containment_and_wipe(hip, inplace):
    """one flipped bit in the sample, the packet-number field, the first byte (a masked bit, the pn_len bits, an unmasked bit), the payload, the tag; the wrong hp slot;
    an expected number of another epoch: that packet fails and no other, no byte outside the failed packets differs from the fixture's, and the wipe zeroes exactly them"""
    rng = random.Random("quic tamper")
    key_len, n = 32, 60
    tab = Table(hip, key_len, 5, 3, 0x9600)
    try:
        pop = Pop(rng, tab, n, 0x9610, lens=[rng.randrange(20, 400) for _ in range(n)])
        wire = pop.wire()
        off, wbuf = _layout(wire, 9)
        exps = pop.expected_pns(rng)
        hps = list(pop.hps)
        tam = bytearray(wbuf)
        hits = {2: ("sample", 0x01), 5: ("sample_end", 0x80), 9: ("pn", 0x01), 13: ("first", 0x04), 17: ("first", 0x01), 21: ("first", 0x40), 25: ("payload", 0x10),
                29: ("tag", 0x01), 33: ("tag_first", 0x80), 37: ("hp_slot", 0), 41: ("epoch", 0), 59: ("pn_last", 0x80)}
        for p, (what, bit) in hits.items():
            po, L = pop.pn_offs[p], len(wire[p])
            at = {"sample": po + 4, "sample_end": po + 19, "pn": po, "pn_last": po + pop.pn_lens[p] - 1, "first": 0, "payload": po + pop.pn_lens[p] + 7, "tag": L - 1,
                  "tag_first": L - 16}.get(what)
            if at is not None:
                tam[off[p] + at] ^= bit
            elif what == "hp_slot":
                hps[p] = tab.n_aead + (hps[p] - tab.n_aead + 1) % tab.n_hp
            else:
                exps[p] = pop.pns[p] + (2 << (8 * pop.pn_lens[p]))               # two windows on: A.3 decodes a number of that epoch
        fill = 0x3C
        back, auth, pn_out, d = _run(hip, tab.kt, True, pop.slots, hps, exps, pop.pn_offs, off, bytes(tam), inplace, out_fill=fill)
        assert auth == [0 if p in hits else 1 for p in range(n)]
        outside = bytes([CANARY if inplace else fill])
        for p in range(n):
            if p not in hits:
                assert back[off[p]:off[p + 1]] == pop.pkts[p][:-16] + wire[p][-16:], p
                assert pn_out[p] == pop.pns[p], p
        assert back[:9] == outside * 9 and back[off[n]:] == outside * TRAIL
        hip.wipe_failed_dev(n, d["out"].ptr, d["auth"].ptr, d_data_off=d["off"].ptr)
        hip.dev_sync()
        wiped = bytes(d["out"].download(len(wbuf)))
        for p in range(n):
            assert wiped[off[p]:off[p + 1]] == (bytes(off[p + 1] - off[p]) if p in hits else back[off[p]:off[p + 1]]), p
        assert wiped[:9] == outside * 9 and wiped[off[n]:] == outside * TRAIL
        assert tab.kt.status() == (hip.OK, 0)
    finally:
        tab.close()


# ---------------------------------------------------------------- 8. stream ordering
def test_set_and_two_calls_on_one_stream(hip):
    """keys, IVs, protect and unprotect on one non-default stream, in place on the same buffers, with no host synchronisation between them"""
    rng = random.Random("quic stream")
    key_len, n = 16, 300
    other = hip.Context(bytes(16))
    st = other.stream()
    tab = Table(hip, key_len, 6, 2, 0x9700, stream=st)
    try:
        pop = Pop(rng, tab, n, 0x9710, max_payload=600)
        off, buf = _layout(pop.pkts, 2)
        exps = pop.expected_pns(rng)
        d_exp = _up(hip, _u64(exps))
        d = _run(hip, tab.kt, False, pop.slots, pop.hps, pop.pns, pop.pn_offs, off, buf, True, stream=st, sync=False)
        d["auth"], d["pn_out"] = _up(hip, b"\x07" * 4 * n), _up(hip, _u64([PN_SENTINEL] * n))
        tab.kt.quic_crypt_dev(True, n, d["slots"].ptr, d["hps"].ptr, d_exp.ptr, d["pn_off"].ptr, d["in"].ptr, d["off"].ptr, d["in"].ptr,
                              d_pn_out=d["pn_out"].ptr, d_auth=d["auth"].ptr, stream=st)
        back, auth, pn_out, _ = _collect(hip, d)
        assert auth == [1] * n and pn_out == pop.pns
        assert back == _layout([r[:-16] + w[-16:] for r, w in zip(pop.pkts, pop.wire())], 2)[1]
        assert tab.kt.status() == (hip.OK, 0)
    finally:
        tab.close()
        other.close()
