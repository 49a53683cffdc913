"""GPU: SRTP and SRTCP packets in wire format through key tables (aesgcm_keytab_srtp_crypt_dev; RFC 7714 AES-GCM over RFC 3711's packets: the RTP header's length parsed
on the device, a tag that is not the packet's last bytes, SRTCP's AAD in two pieces) against tests/srtp_fixture.py, which is written from the RFCs over libcrypto and does
not know the library.  Every byte of a canaried arena is compared: lead and trail guard bytes, and out of place the fill, with the output 5 bytes off the input.
1. both kinds, three key sizes, MKIs of 0 and 4 bytes, both directions, in place and out of place: by the library's own choice of shape, with 8 / 16 / 64 lanes forced, and
under the launch ordered by length class; 2. the RTP grid: every payload start mod 16 x header kind x payload lengths 0 .. 33; 3. the SRTCP grid: E set, every payload
start mod 16 x lengths 0 .. 33; E clear, every packet start mod 16 x every residue of the AAD's packet bytes mod 16 (where W meets them, and splits over two blocks) x bodies
of less than a block, one block and several; 4. forged bits, containment and aesgcm_wipe_failed_dev; 5. every refusal kind, one packet each among good ones, with the
neighbour that just fits; 6. RFC 7714's test vectors (tests/golden/srtp_rfc7714.json) and the host convenience.  SRTCP with E clear has no published vector: it is held to
the RFC's formulas."""
import random
import struct

import pytest

import srtp_fixture as S
from kt_common import CANARY, TRAIL, _u32, _u64, _up
from util import splitmix_bytes

pytestmark = pytest.mark.gpu

RTP, RTCP = S.RTP, S.RTCP
SHIFT = 5
FILL = 0x3C
POISON = 0xDEADDEAD
# RTP header kinds (CSRC count, extension words or None): CC 0, 1, 15; X clear; X set with an extension of 0, 1 and 5 words
HEADERS = ((0, None), (1, None), (15, None), (0, 0), (1, 1), (15, 5))


def _hdr_len(cc, ext):
    return 12 + 4 * cc + (0 if ext is None else 4 + 4 * ext)


class Keys:
    """what the table's slots hold: n slots of session key and 12-byte session salt -- the host's copy, made without a device"""

    def __init__(self, key_len, n, seed):
        self.key_len, self.n = key_len, n
        self.kb = splitmix_bytes(seed, key_len * n)
        self.sb = splitmix_bytes(seed + 1, 12 * n)
        self.keys = [self.kb[key_len * s:key_len * (s + 1)] for s in range(n)]
        self.salts = [self.sb[12 * s:12 * s + 12] for s in range(n)]

    def table(self, hip, extra=0):
        """a key table of the library in force holding them (extra: slots that are never set)"""
        kt = hip.KeyTable(self.key_len, self.n + extra)
        kt.set(0, self.kb)
        kt.set_tls_iv(0, self.sb)
        return kt


class Pop:
    """n plaintext packets of one kind and what the fixture makes of them.  specs[p]: RTP (cc, ext, payload bytes); RTCP (E, bytes behind the 8-byte header).  Every packet:
    headers random but for what is parsed, 0xAA where the tag goes, SRTCP's W = E | a random index, mki_len random MKI bytes"""

    def __init__(self, kind, keys, rng, specs, seed, mki_len=0):
        n = self.n = len(specs)
        self.kind, self.keys, self.mki_len, self.specs = kind, keys, mki_len, list(specs)
        self.slots = [rng.randrange(keys.n) for _ in range(n)]
        self.slots[0], self.slots[-1] = 0, keys.n - 1
        self.rocs = [rng.getrandbits(rng.choice((1, 16, 32))) for _ in range(n)]
        blob = splitmix_bytes(seed, sum(s[-1] for s in specs) + 256 * n)
        self.pkts, at = [], 0
        for p, s in enumerate(specs):
            fill = blob[at:at + 256]
            if kind == RTP:
                cc, ext, x = s
                h = S.rtp_header(cc, ext, rng.getrandbits(16), rng.getrandbits(32), rng.getrandbits(32), fill, pt=rng.randrange(128), marker=rng.randrange(2),
                                 padding=rng.randrange(2))
                assert len(h) == _hdr_len(cc, ext)
                tail = b""
            else:
                e, x = s
                h = bytes([0x80 | rng.randrange(32), 200 + rng.randrange(5)]) + fill[0:2] + fill[4:8]          # the length field is not interpreted
                tail = ((e << 31) | rng.getrandbits(rng.choice((1, 12, 31)))).to_bytes(4, "big")
            self.pkts.append(h + blob[at + 256:at + 256 + x] + b"\xAA" * 16 + tail + fill[200:200 + mki_len])
            at += 256 + x
        self.hdrs = [S.rtp_hdr_len(r) if kind == RTP else 8 for r in self.pkts]
        self.tags = [len(r) - mki_len - (16 if kind == RTP else 20) for r in self.pkts]                          # where each tag starts
        self._wire = None

    def protect(self, p, pkt=None):
        k, s = self.keys, self.slots[p]
        return S.protect(self.kind, k.keys[s], k.salts[s], self.rocs[p], self.pkts[p] if pkt is None else pkt, self.mki_len)

    def unprotect(self, p, pkt, roc=None):
        k, s = self.keys, self.slots[p]
        return S.unprotect(self.kind, k.keys[s], k.salts[s], self.rocs[p] if roc is None else roc, pkt, self.mki_len)

    def wire(self):
        """the fixture's protected packets (computed once, never changed)"""
        if self._wire is None:
            self._wire = [self.protect(p) for p in range(self.n)]
        return self._wire

    def clear(self):
        """what decrypting wire() leaves: headers and plaintext, then the tag's bytes as they came, W and the MKI"""
        return [r[:t] + w[t:] for r, w, t in zip(self.pkts, self.wire(), self.tags)]


def _layout(pkts, lead):
    off = [lead]
    for r in pkts:
        off.append(off[-1] + len(r))
    return off, bytes([CANARY]) * lead + b"".join(pkts) + bytes([CANARY]) * (TRAIL + SHIFT)


def _run(hip, kt, pop, decrypt, off, buf, shift=None, slots=None, rocs=None):
    """one call.  shift None: in place; else out of place into a buffer of FILL, the output `shift` bytes off the input.  -> (the output buffer from the input's first
    byte's counterpart on, auth, device buffers)"""
    n, rtp = len(off) - 1, pop.kind == RTP
    fmt = hip.SrtpFormat.rtp(pop.mki_len) if rtp else hip.SrtpFormat.rtcp(pop.mki_len)
    d = {"slots": _up(hip, _u32(pop.slots if slots is None else slots)), "in": _up(hip, buf), "off": _up(hip, _u64(off))}
    assert d["in"].ptr % 16 == 0
    d["out"] = d["in"] if shift is None else _up(hip, bytes([FILL]) * (len(buf) + 16))
    d["auth"] = _up(hip, b"\x07" * 4 * n) if decrypt else None
    d["roc"] = _up(hip, _u32(pop.rocs if rocs is None else rocs)) if rtp else None
    d["out_ptr"] = d["out"].ptr + (shift or 0)
    kt.srtp_crypt_dev(decrypt, fmt, n, d["slots"].ptr, d["in"].ptr, d["off"].ptr, d["out_ptr"], d_roc=d["roc"].ptr if rtp else None,
                      d_auth=d["auth"].ptr if decrypt else None)
    hip.dev_sync()
    whole = bytes(d["out"].download(len(buf) + (16 if shift is not None else 0)))
    if shift is not None:
        assert whole[:shift] == bytes([FILL]) * shift and whole[shift + len(buf):] == bytes([FILL]) * (16 - shift), "bytes around the shifted output overwritten"
        assert bytes(d["in"].download(len(buf))) == buf, "the input of an out-of-place call changed"
        whole = whole[shift:shift + len(buf)]
    auth = list(struct.unpack("<%di" % n, bytes(d["auth"].download(4 * n)))) if decrypt else None
    return whole, auth, d


def _want(buf, off, pkts, shift):
    """the arena with pkts[p] (None: untouched) in place of packet p: in place over buf, out of place over FILL"""
    w = bytearray(buf if shift is None else bytes([FILL]) * len(buf))
    for p, r in enumerate(pkts):
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
            return "byte %d of packet %d (%d bytes): %02x, wanted %02x" % (x - off[p], p, off[p + 1] - off[p], got[x], want[x])
    return "byte %d, outside the packets: %02x, wanted %02x" % (x, got[x], want[x])


def _both_ways(hip, kt, pop, lead, shift):
    """protect against the fixture, every byte of the arena; then the fixture's packets back: headers, plaintext, the tag's bytes as they were, W and MKI, every tag
    accepted"""
    n = pop.n
    off, buf = _layout(pop.pkts, lead)
    _, wbuf = _layout(pop.wire(), lead)
    out, _, _ = _run(hip, kt, pop, False, off, buf, shift)
    want = _want(buf, off, pop.wire(), shift)
    assert out == want, _first_difference(out, want, off)
    back, auth, _ = _run(hip, kt, pop, True, off, wbuf, shift)
    assert auth == [1] * n, [(p, pop.specs[p]) for p in range(n) if auth[p] != 1][:8]
    wantp = _want(wbuf, off, pop.clear(), shift)
    assert back == wantp, _first_difference(back, wantp, off)
    assert kt.status() == (hip.OK, 0)


# ---------------------------------------------------------------- 1. populations: every instance of k_kt_srtp
_POPS = {}


def _population(kind, key_len, mki_len):
    """about 300 packets over 5 slots: payload lengths 0 .. 48, and for G = 8, 16 and 64 lanes per packet the lengths that make G - 1, G and G + 1 blocks of AAD and
    payload together, ending a byte into a block, on its last byte and a byte past it.  RTP: every header kind; SRTCP: E mixed, and with E clear it is the AAD that has
    those lengths.  Built once per kind, key size and MKI length, never changed"""
    if (kind, key_len, mki_len) not in _POPS:
        rng = random.Random("srtp pop %d %d %d" % (kind, key_len, mki_len))
        keys = Keys(key_len, 5, 0x5700 + 16 * kind + key_len)
        specs = []
        for x in range(49):
            specs.append(HEADERS[x % len(HEADERS)] + (x,) if kind == RTP else (x % 2, x))
        i = 0
        for G in (8, 16, 64):
            for total in (G - 1, G, G + 1):
                for d in (-15, 0, 1):
                    for rep in (0, 1):
                        i += 1
                        if kind == RTP:
                            cc, ext = HEADERS[i % len(HEADERS)]
                            specs.append((cc, ext, 16 * (total - (_hdr_len(cc, ext) + 15) // 16) + d))
                        elif rep:
                            specs.append((1, 16 * (total - 1) + d))              # E set: one AAD block
                        else:
                            specs.append((0, 16 * total + d - 4 - 8))            # E clear: 8 + x + 4 bytes of AAD, no payload
        while len(specs) < 300:
            specs.append(rng.choice(HEADERS) + (rng.randrange(300),) if kind == RTP else (rng.randrange(2), rng.randrange(300)))
        assert all(s[-1] >= 0 for s in specs)
        rng.shuffle(specs)
        pop = Pop(kind, keys, rng, specs, 0x5710 + 16 * kind + key_len, mki_len)
        if kind == RTP:
            assert {s[:2] for s in specs} == set(HEADERS)
        pop.wire()
        _POPS[kind, key_len, mki_len] = pop
    return _POPS[kind, key_len, mki_len]


SHAPES = ["own", "lanes8", "lanes16", "lanes64", "ordered8", "ordered16"]


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("key_len", [16, 24, 32])
@pytest.mark.parametrize("kind", [RTP, RTCP])
def test_packets_vs_fixture(hip, kind, key_len, shape):
    """encrypt and decrypt, in place and with the output 5 bytes off the input, without an MKI and with one of 4 bytes, by the library's own choice of shape, with the
    lanes per packet forced (the debug library's batch_lanes), and under the launch ordered by falling length class (batch_order = 1, which the 8- and 16-lane shapes take)"""
    def legs():
        for mki_len in (0, 4):
            pop = _population(kind, key_len, mki_len)
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


# ---------------------------------------------------------------- 2. the RTP grid
def _fit(pos, fixed, residue):
    """the payload length 0 .. 15 of a filler packet that starts at pos and has `fixed` bytes beside its payload, so that the packet behind it starts at `residue` mod 16"""
    return (residue - (pos + fixed)) % 16


@pytest.mark.parametrize("key_len", [16, 32])
def test_rtp_grid(hip, key_len):
    """every payload start mod 16 x header kind x payload lengths 0 .. 33 -- a filler packet in front of each cell puts it there"""
    rng = random.Random("srtp grid %d" % key_len)
    keys = Keys(key_len, 4, 0x5800 + key_len)
    lead, mki_len = 1, 4 if key_len == 32 else 0
    specs, cells, pos = [], [], lead
    for res in range(16):
        for cc, ext in HEADERS:
            hdr = _hdr_len(cc, ext)
            for n in range(34):
                x = _fit(pos, 28 + mki_len, (res - hdr) % 16)                 # the filler: a bare header of 12
                specs.append((0, None, x))
                pos += 28 + mki_len + x
                assert (pos + hdr) % 16 == res
                cells.append(len(specs))
                specs.append((cc, ext, n))
                pos += hdr + n + 16 + mki_len
    pop = Pop(RTP, keys, rng, specs, 0x5810, mki_len)
    off, _ = _layout(pop.pkts, lead)
    assert {((off[p] + pop.hdrs[p]) % 16, pop.specs[p][:2], pop.specs[p][2]) for p in cells} == {(r, h, n) for r in range(16) for h in HEADERS for n in range(34)}
    with keys.table(hip) as kt:
        _both_ways(hip, kt, pop, lead, None)
        _both_ways(hip, kt, pop, lead, SHIFT)


# ---------------------------------------------------------------- 3. the SRTCP grid
@pytest.mark.parametrize("mki_len", [0, 3])
def test_rtcp_grid(hip, mki_len):
    """E set: every payload start mod 16 x payload lengths 0 .. 33.  E clear: every packet start mod 16 x every residue mod 16 of the AAD's packet bytes -- the byte of the
    last AAD block at which W begins; from residue 13 on W splits over two blocks -- x bodies of less than a block (8 .. 15), one block and four.  A filler packet in front
    of each cell puts it at its address"""
    rng = random.Random("srtcp grid %d" % mki_len)
    keys = Keys(32 if mki_len else 16, 4, 0x5900 + mki_len)
    lead = 2
    fixed = 28 + mki_len                                                      # what a packet has beside the bytes behind its header
    bodies = sorted(set(range(8, 16)) | {16 + r for r in range(16)} | {64 + r for r in range(16)})
    specs, cells, pos = [], [], lead
    for res in range(16):
        for e, xs in ((1, range(34)), (0, [b - 8 for b in bodies])):
            for x in xs:
                f = _fit(pos, fixed, res if e == 0 else (res - 8) % 16)
                specs.append((1, f))
                pos += fixed + f
                assert (pos + (8 if e else 0)) % 16 == res
                cells.append(len(specs))
                specs.append((e, x))
                pos += fixed + x
    pop = Pop(RTCP, keys, rng, specs, 0x5910, mki_len)
    off, _ = _layout(pop.pkts, lead)
    assert {((off[p] + 8) % 16, pop.specs[p][1]) for p in cells if pop.specs[p][0]} == {(r, n) for r in range(16) for n in range(34)}
    assert {(off[p] % 16, pop.tags[p]) for p in cells if not pop.specs[p][0]} == {(r, b) for r in range(16) for b in bodies}
    assert {b % 16 for b in bodies} == set(range(16)) and all(pop.pkts[p][pop.tags[p] + 16] >> 7 == pop.specs[p][0] for p in range(pop.n))
    with keys.table(hip) as kt:
        _both_ways(hip, kt, pop, lead, None)
        _both_ways(hip, kt, pop, lead, SHIFT)


# ---------------------------------------------------------------- 4. forged bits, containment, wipe
@pytest.mark.parametrize("shift", [None, SHIFT])
@pytest.mark.parametrize("kind", [RTP, RTCP])
def test_forged_bits_containment_and_wipe(hip, kind, shift):
    """one flipped bit in the header, the SSRC, a CSRC, the extension, the payload, the tag's first and last byte, W's index and its E bit (packets with E set and with E
    clear), and for SRTP a wrong rollover counter: that packet fails and no other, its neighbours' bytes are the fixture's, nothing outside the packets is written, and
    aesgcm_wipe_failed_dev zeroes exactly the failed packets.  A flipped MKI bit fails nothing and passes through"""
    rng = random.Random("srtp forge %d" % kind)
    n, mki_len = 60, 4
    keys = Keys(32, 5, 0x5A00 + kind)
    if kind == RTP:
        specs = [(1, 1, rng.randrange(20, 300)) for _ in range(n)]            # a header of 24: 12, a CSRC, an extension of one word
        hits = {2: "tag_first", 7: "tag_last", 11: "payload", 13: "marker", 19: "seq", 23: "ssrc", 29: "csrc", 31: "ext_profile", 32: "ext_word", 41: "roc", 59: "payload"}
    else:
        specs = [(p % 2, rng.randrange(20, 300)) for p in range(n)]
        hits = {2: "tag_first", 7: "tag_last", 11: "payload", 12: "payload", 13: "hdr", 18: "hdr", 22: "ssrc", 23: "ssrc", 30: "index", 31: "index", 40: "e_bit", 41: "e_bit",
                59: "tag_first"}
    pop = Pop(kind, keys, rng, specs, 0x5A10 + kind, mki_len)
    wire = pop.wire()
    off, wbuf = _layout(wire, 9)
    tam = bytearray(wbuf)
    rocs = list(pop.rocs)
    for p, what in hits.items():
        t = pop.tags[p]
        at = {"tag_first": t, "tag_last": t + 15, "payload": pop.hdrs[p] + 3, "marker": 1, "seq": 3, "ssrc": 9 if kind == RTP else 5, "csrc": 13, "ext_profile": 16,
              "ext_word": 21, "hdr": 1, "index": t + 19, "e_bit": t + 16}.get(what)
        if at is not None:
            tam[off[p] + at] ^= 0x80 if what in ("tag_last", "marker", "e_bit") else 1
        else:
            rocs[p] ^= 1
    mki_hits = {4, 5, 44}
    for p in mki_hits:
        tam[off[p + 1] - 1 - (p % 3)] ^= 0x10
    tam = bytes(tam)
    ref = [pop.unprotect(p, tam[off[p]:off[p + 1]], rocs[p]) for p in range(n)]
    assert [int(r[1]) for r in ref] == [0 if p in hits else 1 for p in range(n)]
    with keys.table(hip) as kt:
        back, auth, d = _run(hip, kt, pop, True, off, tam, shift, rocs=rocs)
        assert auth == [0 if p in hits else 1 for p in range(n)]
        for p in range(n):
            if p not in hits:
                assert back[off[p]:off[p + 1]] == ref[p][0], p
                assert (ref[p][0] == pop.clear()[p]) == (p not in mki_hits), p
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
REFUSALS = [(RTP, c) for c in ("slot_range", "slot_unset", "falling", "long", "short", "version", "csrc", "ext_fixed", "ext_len")] + \
           [(RTCP, c) for c in ("slot_range", "slot_unset", "falling", "long", "short", "version")]


@pytest.mark.parametrize("kind, case", REFUSALS)
def test_refused_packets(hip, kind, case):
    """each refusal alone among good packets, both directions, in place and out of place: the refused packet's bytes are untouched, its verdict is 0, its d_roc holds a
    poisoned value, the status word names the lowest refused index and clears on reading.  Beside each refused packet stands the one that just fits, and is taken"""
    rng = random.Random("srtp refuse %d %s" % (kind, case))
    key_len, n, mki_len = 32, 40, 4
    rtp = kind == RTP
    keys = Keys(key_len, 5, 0x5B00 + kind)
    n_slots = keys.n + 1                                                      # the last slot is never set
    floor = (12 if rtp else 8) + (16 if rtp else 20) + mki_len                # the shortest packet there is
    specs = [rng.choice(HEADERS) + (rng.randrange(200),) if rtp else (rng.randrange(2), rng.randrange(200)) for _ in range(n)]
    cut = {}                                                                  # refused packets made by hand: index -> bytes
    if case == "long":
        specs[11] = (0, None, 65536 - floor) if rtp else (1, 65536 - floor)  # L = 65536: refused
        specs[12] = (0, None, 65535 - floor) if rtp else (0, 65535 - floor)  # L = 65535: the longest packet there is, taken
        refused = {11}
    elif case == "short":
        specs[5] = (0, None, 0) if rtp else (1, 0)                            # L = floor: taken
        specs[28] = (0, None, 0) if rtp else (0, 0)
        cut = {6: floor - 1, 29: 0, 30: 1}
        refused = set(cut)
    elif case == "version":
        refused = {14, 15, 16}
    elif case == "csrc":
        specs[8] = (15, None, 0)                                              # 72 + 16 + mki_len == L: taken
        cut = {9: bytes([0x8F]) + splitmix_bytes(9, 72 + 16 + mki_len - 2), 20: bytes([0xA3]) + splitmix_bytes(20, floor - 1)}      # CC = 15 and CC = 3, a byte short / 12 short
        refused = set(cut)
    elif case == "ext_fixed":
        specs[8] = (0, 0, 0)                                                  # 12 + 4 + 16 + mki_len == L: taken
        cut = {9: bytes([0x90]) + splitmix_bytes(9, 12 + 4 + 16 + mki_len - 2), 21: bytes([0x90]) + splitmix_bytes(21, floor - 1)}  # a byte short, and no byte of the extension
        refused = set(cut)
    elif case == "ext_len":
        specs[8] = (1, 5, 0)                                                  # 16 + 4 + 20 + 16 + mki_len == L: taken
        a = bytearray(bytes([0x91]) + splitmix_bytes(9, 16 + 4 + 20 + 16 + mki_len - 2))
        a[18:20] = b"\x00\x05"                                                # the extension's five words end a byte behind the room there is
        b = bytearray(bytes([0x90]) + splitmix_bytes(22, 299))
        b[14:16] = b"\xFF\xFF"                                                # ... and 65535 words
        cut = {9: bytes(a), 22: bytes(b)}
        refused = set(cut)
    pop = Pop(kind, keys, rng, specs, 0x5B10 + kind, mki_len)
    slots, pkts = list(pop.slots), list(pop.pkts)
    clear = []
    for p, c in cut.items():
        pkts[p] = c if isinstance(c, bytes) else pkts[p][:c]
    if case == "long":
        assert len(pkts[11]) == 65536 and len(pkts[12]) == 65535
    elif case == "short":
        assert len(pkts[5]) == len(pkts[28]) == floor
    elif case == "slot_range":
        slots[9], slots[10], slots[33] = n_slots, 0xFFFFFFFF, n_slots + 77
        refused = {9, 10, 33}
    elif case == "slot_unset":
        pop.slots = slots = [s if s != 2 else 3 for s in slots]
        slots = list(slots)
        slots[3], slots[21] = 2, n_slots - 1                                  # cleared below, and never set
        refused, clear = {3, 21}, [2]
    elif case == "version":
        for p, b0 in ((14, 0x00), (15, 0x40), (16, 0xC0)):
            pkts[p] = bytes([(pkts[p][0] & 0x3F) | b0]) + pkts[p][1:]
    off, buf = _layout(pkts, 11)
    if case == "falling":
        # the last two entries: [A, A - 3) falls; [A - 3, A - 3 + 20) names bytes of packet n - 3 and is too short for any packet
        off[n - 1] = off[n - 2] - 3
        off[n] = off[n - 1] + 20
        refused = {n - 2, n - 1}
        buf = buf + bytes([CANARY]) * 64
    ok = [p for p in range(n) if p not in refused]
    wire = {p: pop.protect(p, pkts[p]) for p in ok}
    rocs = [POISON if p in refused else pop.rocs[p] for p in range(n)]
    with keys.table(hip, extra=1) as kt:
        for s in clear:
            kt.clear(s)
        for shift in (None, SHIFT):
            out, _, _ = _run(hip, kt, pop, False, off, buf, shift, slots=slots, rocs=rocs)
            want = _want(buf, off, [wire.get(p) for p in range(n)], shift)
            assert out == want, (case, shift, _first_difference(out, want, off))
            assert kt.status() == (hip.EARG, min(refused)), case
            assert kt.status() == (hip.OK, 0)
            enc = _want(buf, off, [wire.get(p) for p in range(n)], None)
            back, auth, _ = _run(hip, kt, pop, True, off, enc, shift, slots=slots, rocs=rocs)
            assert auth == [0 if p in refused else 1 for p in range(n)], case
            wantp = _want(enc, off, [pkts[p][:pop.tags[p]] + wire[p][pop.tags[p]:] if p in wire else None for p in range(n)], shift)
            assert back == wantp, (case, shift, _first_difference(back, wantp, off))
            assert kt.status() == (hip.EARG, min(refused)), case


# ---------------------------------------------------------------- 6. RFC 7714's vectors, and the host convenience
@pytest.mark.parametrize("shift", [None, SHIFT])
def test_rfc7714_vectors(hip, shift):
    """each published vector encrypted to the RFC's bytes and decrypted back, alone in its call, at an odd address"""
    for name, kind, key, salt, roc, plain, _, wire in S.vectors():
        class P:
            n, mki_len, slots, rocs = 1, 0, [1], [roc]
        P.kind = kind
        with hip.KeyTable(len(key), 2) as kt:
            kt.set(1, key)
            kt.set_tls_iv(1, salt)
            off, pbuf = _layout([plain], 7)
            out, _, _ = _run(hip, kt, P, False, off, pbuf, shift)
            want = _want(pbuf, off, [wire], shift)
            assert out == want, (name, _first_difference(out, want, off))
            _, wbuf = _layout([wire], 7)
            back, auth, _ = _run(hip, kt, P, True, off, wbuf, shift)
            t = len(wire) - (16 if kind == RTP else 20)
            wantp = _want(wbuf, off, [plain[:t] + wire[t:]], shift)
            assert auth == [1] and back == wantp, (name, _first_difference(back, wantp, off))
            assert kt.status() == (hip.OK, 0)


def test_crypt_srtp_host_convenience(hip):
    rng = random.Random("srtp host")
    for kind, mki_len in ((RTP, 0), (RTP, 4), (RTCP, 0), (RTCP, 4)):
        keys = Keys(16, 3, 0x5C00 + kind)
        specs = [(0, None, 0), (1, 1, 1), (15, 5, 17), (0, 0, 100), (15, None, 1400)] if kind == RTP else [(1, 0), (0, 0), (1, 17), (0, 101), (1, 1400)]
        pop = Pop(kind, keys, rng, specs, 0x5C10 + kind, mki_len)
        fmt = hip.SrtpFormat.rtp(mki_len) if kind == RTP else hip.SrtpFormat.rtcp(mki_len)
        with keys.table(hip) as kt:
            kw = dict(rocs=pop.rocs) if kind == RTP else {}
            outs, auth = kt.crypt_srtp(fmt, pop.slots, pop.pkts, **kw)
            assert outs == pop.wire() and auth is None
            back, auth = kt.crypt_srtp(fmt, pop.slots, pop.wire(), decrypt=True, **kw)
            assert back == pop.clear() and auth == [1] * pop.n
            assert kt.status() == (hip.OK, 0)
