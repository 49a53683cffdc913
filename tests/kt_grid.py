"""The alignment grid of the key-table family: wire frames (MACsec, ESP), their 64-bit-number forms (XPN, ESN), TLS records, QUIC packets, DTLS records and SRTP /
SRTCP packets.  One deterministic generator (numpy only, no GPU) for tests/test_gpu_kt_grid.py and for the CPU check of the generator itself (tests/test_kt_grid_cpu.py).

All of these run the text of aesgcm_batch3_body.inc under WIRE / WIREX: a nonce loaded from the middle of a header, an ICV of 8, 12 or 16 bytes whose dword accesses
must end at the frame's end (SRTP / SRTCP: at the tag's end, in front of a trailer), wire_copy_front's overlapping last piece, AAD blocks built in registers, a header
length per packet (QUIC, DTLS 1.3, RTP), k_kt_quic_hp's and k_kt_dtls_sn's sample at any address, SRTCP's AAD in two pieces.  What such code gets wrong is one
(address & 15, length & 15) pair, a turn of the lane group's loop, or a store that spills into the neighbour.  So a grid is one byte-packed buffer of frames
front | payload | ICV | trailer with its offset array, made of CELLS that must all occur, placed by pkt_grid.pack (the packet kernels' own loop):

  residue by length   every (payload start mod 16, payload length) for lengths 0 .. 272 and the mode's slot edges; every (payload start mod 128, length) for
                      pkt_grid.compact_lengths() and the slot edges.  The auth-only formats (macsec_auth, srtcp_clear) have no payload: there the start is the
                      frame's and the length is what its body has behind the header (the body, header included, is the AAD; SRTCP's W joins it).
  slot edges          a frame is na AAD blocks and its payload blocks, G of them per turn of its lane group: payload lengths 16 (m - na) + d for
                      m in G - 1, G, G + 1, 2 G - 1, 2 G, 2 G + 1, d in -1, 0, 1 and G in 8, 16, 64 -- one grid per mode for all three lane counts.  Where na is the
                      packet's own (QUIC: 1 .. 4 blocks of header; DTLS 1.3: 1 .. 2; RTP: 1, 2, 5, 6) every (na, G, m, d) occurs on a packet with that na, and the
                      residue cells are those of the lengths 0 .. 272 and of compact_lengths().
  ICV placement       every ICV start mod 16 (follows from the above; asserted)
  QUIC header         pn_len cycles 1 .. 4, pn_off through a permutation of 1 .. 51 (period 51), long and short first bytes with period 5: every combination occurs;
                      every (sample address (start + pn_off + 4) mod 16, pn_len, form) of the 16 x 4 x 2 occurs; pn_len + payload >= 4 (the sample lies in the packet)
  DTLS 1.3 header     0 0 1 C S L E E | CID | 1 or 2 sequence bytes | 2 length bytes under L (random: not interpreted).  The CID length cycles through 0, 1, 7, 20
                      (period 4), S with period 3, L with period 5: every (payload start mod 16 -- the sample's address --, CID, S, L) of the 16 x 4 x 2 x 2 occurs
  DTLS 1.2            hdr[13] | explicit nonce[8] | payload | tag: version fe fd and the length field written, the rest seeded; epoch | sequence number (bytes 3 .. 10)
                      all zero on one pinned record and all ones on another
  RTP header          the six kinds of HEADERS (CSRC count, extension words): 12, 16, 72, 16 with X, 24 and 96 bytes, period 6: every (payload start mod 16, kind)
                      occurs; version 2, CC, X and the extension's length field say what the kind says, every other bit is seeded; srtp_mki: 4 bytes of MKI end it
  SRTCP               hdr[8] | payload | tag | W (srtcp: E set on every packet, trailer 4) or hdr[8] | body | tag | W | mki[3] (srtcp_clear: E clear, trailer 7, auth
                      only: AAD = hdr | body | W, na = (8 + x + 4 + 15) // 16).  The seam: where W meets the packet's bytes in the AAD's last block or two, (8 + x) mod 16:
                      every (packet start mod 16, seam) occurs on AADs of 1 block (x = 0 .. 4: seams 8 .. 12, all there are), of 2 blocks and of 9 or more
  numbers             hi / seq / pn / roc from a seeded stream; 0, 2^32 - 1, 2^32 and the format's last (QUIC 2^62 - 1, DTLS 1.3 2^64 - 1) pinned on the packets PINNED
                      names (hi and roc are 32 bits wide: 0 and 2^32 - 1).  RTP's SEQ is 0 and 0xFFFF, SRTCP's index 0 and 2^31 - 1 on the first two of them
  slots               packet i takes AEAD slot i mod 11 (QUIC, DTLS 1.3: the second slot 11 + i mod 5): neighbours never share a key

Fillers are ordinary frames, checked like the rest.  Every arena has pkt_grid.GUARD canary bytes in front and behind.  The generator asserts that every required cell
occurred (Grid.check): a grid that lost a part fails."""
import numpy as np

import pkt_grid as PG

LANES = (8, 16, 64)
N_AEAD, N_HP = 11, 5
PLACEHOLDER = 0xAA                                     # where the ICV goes in a plaintext frame
PINNED = {"zero": 0, "u32_max": 1, "two_32": 2, "two_62_less_1": 3, "two_64_less_1": 3}        # packet indices
PN_OFFS = tuple((20 * k) % 51 + 1 for k in range(51))                    # a permutation of 1 .. 51: period 51, coprime to 4, 16 and 5
LONG_FORM = (False, True, False, False, True)                            # period 5
CIDS = (0, 1, 7, 20)                                                     # DTLS 1.3 connection ID lengths: period 4
S16 = (False, True, True)                                                # ... a sequence field of 16 bits: period 3
WITH_LEN = (False, True, False, False, True)                             # ... the L bit: period 5
HEADERS = ((0, None), (1, None), (15, None), (0, 0), (1, 1), (15, 5))    # RTP header kinds (CSRC count, extension words or None), as tests/test_gpu_srtp.py's

#        family, bytes in front of the payload, ICV, AAD blocks (None: the frame's own), auth-only, the number that is not on the wire
MODES = {
    "macsec": ("wire", 28, 16, 2, False, None),
    "esp16": ("wire", 16, 16, 1, False, None),
    "macsec_auth": ("wire", 20, 16, None, True, None),
    "esp12": ("wire", 16, 12, 1, False, None),
    "esp8": ("wire", 16, 8, 1, False, None),
    "xpn": ("wirex", 28, 16, 2, False, "hi"),
    "esn16": ("wirex", 16, 16, 1, False, "hi"),
    "tls13": ("tls", 5, 16, 1, False, "seq"),
    "tls12": ("tls", 13, 16, 1, False, "seq"),
    "quic": ("quic", None, 16, None, False, "pn"),
    "dtls12": ("dtls", 21, 16, 1, False, None),
    "dtls13": ("dtls", None, 16, None, False, "seq"),
    "srtp": ("srtp", None, 16, None, False, "roc"),
    "srtp_mki": ("srtp", None, 16, None, False, "roc"),
    "srtcp": ("srtp", 8, 16, 1, False, None),
    "srtcp_clear": ("srtp", 8, 16, None, True, None),
}
TRAILS = {"srtp_mki": 4, "srtcp": 4, "srtcp_clear": 7}                   # bytes behind the tag: SRTCP's W and the MKI
# the order that seeds are counted in: the first ten modes sorted, as they were when they were all there was, then the later ones -- a new mode moves no old arena
SEED_ORDER = sorted(list(MODES)[:10]) + list(MODES)[10:]
_M = (lambda G: (G - 1, G, G + 1, 2 * G - 1, 2 * G, 2 * G + 1))


def splitmix(seed, n):
    """n 64-bit words of splitmix64 from `seed`"""
    z = np.uint64(seed) + np.arange(1, n + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def slot_edges(na, less=0):
    """payload lengths either side of a whole number of turns: 16 (m - na) + d - less, where not negative"""
    return sorted({16 * (m - na) + d - less for G in LANES for m in _M(G) for d in (-1, 0, 1) if 16 * (m - na) + d - less >= 0})


def rtp_hdr_len(kind):
    cc, ext = kind
    return 12 + 4 * cc + (0 if ext is None else 4 + 4 * ext)


class Grid:
    """n frames of one mode.  off has n + 1 entries, offsets from the arena's first byte (off[0] = GUARD); the arena is off[n] + GUARD bytes: canary, the plaintext
    frames (seeded front, payload and trailer, PLACEHOLDER where the ICV goes), canary.  lens: what the cells count (payload bytes; auth-only: body bytes behind the
    header); fronts: the bytes in front of that; trail: the bytes behind the ICV, which starts at flen - trail - tag_len."""

    def __init__(self, mode):
        self.mode = mode
        self.family, hdr, self.tag_len, na, self.auth_only, self.number = MODES[mode]
        quic, d13, rtp = self.family == "quic", mode == "dtls13", mode in ("srtp", "srtp_mki")
        self.rtcp = mode in ("srtcp", "srtcp_clear")
        tr = TRAILS.get(mode, 0)
        self.aad_extra = 4 if mode == "srtcp_clear" else 0                # what the auth-only AAD has besides the frame's bytes in front of the ICV: SRTCP's W
        self.lc = PG.compact_lengths()
        self.nas = (1, 2, 3, 4) if quic else (1, 2) if d13 else (1, 2, 5, 6) if rtp else None        # the AAD blocks of a mode whose packets have their own
        if self.nas:
            self.full = list(range(273))
            allowed = None
            if quic:
                self.pn_lens = lambda i: 1 + i % 4
                self.pn_offs = lambda i: PN_OFFS[i % 51]
                front = lambda i: self.pn_offs(i) + self.pn_lens(i)
                allowed = lambda i, L: self.pn_lens(i) + L >= 4
            elif d13:
                front = lambda i: 1 + CIDS[i % 4] + (2 if S16[i % 3] else 1) + (2 if WITH_LEN[i % 5] else 0)
            else:
                front = lambda i: rtp_hdr_len(HEADERS[i % 6])
            na_of = lambda i: (front(i) + 15) // 16
            want = {(a, L) for a in self.nas for L in slot_edges(a)}
            self.edge_cells = sorted(want)

            def prefer(i):
                c = [L for (a, L) in want if a == na_of(i) and (allowed is None or allowed(i, L))]
                if not c:
                    return None
                want.discard((na_of(i), max(c)))
                return max(c)
            lens = PG.pack(self.full, self.lc, front=front, span=lambda i, L: front(i) + L + 16 + tr, allowed=allowed, prefer=prefer)
            assert not want
        else:
            edges = slot_edges(0, less=hdr + self.aad_extra) if self.auth_only else slot_edges(na)
            self.full = sorted(set(range(273)) | set(edges))
            self.lc = sorted(set(self.lc) | set(edges))
            self.edge_cells = edges
            cell_front = 0 if self.auth_only else hdr                     # where the counted start lies in the frame
            front = lambda i: hdr
            lens = PG.pack(self.full, self.lc, front=lambda i: cell_front, span=lambda i, L: hdr + L + self.tag_len + tr)
        n = self.n = len(lens)
        self.lens = lens
        self.fronts = [front(i) for i in range(n)]
        self.trail = [tr] * n
        flen = [f + L + self.tag_len + tr for f, L in zip(self.fronts, lens)]
        self.off = np.concatenate(([PG.GUARD], PG.GUARD + np.cumsum(flen))).astype(np.uint64)
        self.size = int(self.off[-1]) + PG.GUARD
        self.at = [int(x) for x in self.off[:-1]]
        self.flen = flen
        self.slots = [i % N_AEAD for i in range(n)]
        self.hps = [N_AEAD + i % N_HP for i in range(n)] if quic or d13 else None       # QUIC's header-protection slot, DTLS 1.3's record-number slot
        seed = 0x6B740000 + 97 * SEED_ORDER.index(mode)
        # ---- the numbers that are not on the wire
        self.nums = None
        if self.number:
            w = splitmix(seed + 1, n)
            if self.number == "hi":
                nums = [int(x) & 0xFFFFFFFF for x in w]
                nums[PINNED["zero"]], nums[PINNED["u32_max"]] = 0, 2 ** 32 - 1
            elif self.number == "roc":
                nums = [int(x) >> (64 - (1, 16, 32)[i % 3]) for i, x in enumerate(w)]
                nums[PINNED["zero"]], nums[PINNED["u32_max"]] = 0, 2 ** 32 - 1
            else:
                bits = (8, 16, 31, 33, 62) if quic else (8, 16, 31, 33, 48, 64) if d13 else (64,)
                nums = [int(x) >> (64 - bits[i % len(bits)]) for i, x in enumerate(w)]
                nums[PINNED["zero"]], nums[PINNED["u32_max"]], nums[PINNED["two_32"]] = 0, 2 ** 32 - 1, 2 ** 32
                if quic:
                    nums[PINNED["two_62_less_1"]] = 2 ** 62 - 1
                if d13:
                    nums[PINNED["two_64_less_1"]] = 2 ** 64 - 1
            self.nums = nums
        if self.rtcp:                                                     # W's 31-bit index: on the wire, behind the tag
            self.index = [int(x) >> 33 for x in splitmix(seed + 1, n)]
            self.index[PINNED["zero"]], self.index[PINNED["u32_max"]] = 0, 2 ** 31 - 1
        # ---- the arena
        a = np.full(self.size, PG.CANARY_IN, dtype=np.uint8)
        r = splitmix(seed + 2, (self.size + 7) // 8).view(np.uint8)
        put = lambda at, v, k: a.__setitem__(slice(at, at + k), np.frombuffer(int(v).to_bytes(k, "big"), dtype=np.uint8))
        for i in range(n):
            s, e = self.at[i], self.at[i] + flen[i]
            a[s:e] = r[s:e]
            a[e - tr - self.tag_len:e - tr] = PLACEHOLDER
            if quic:
                po, pl = self.pn_offs(i), self.pn_lens(i)
                a[s] = (int(a[s]) & 0x7C) | (pl - 1) | (0x80 if LONG_FORM[i % 5] else 0)
                put(s + po, self.nums[i] & ((1 << (8 * pl)) - 1), pl)
            elif d13:
                c, s16, wl = CIDS[i % 4], S16[i % 3], WITH_LEN[i % 5]
                a[s] = 0x20 | (0x10 if c else 0) | (0x08 if s16 else 0) | (0x04 if wl else 0) | (int(a[s]) & 3)
                put(s + 1 + c, self.nums[i] & (0xFFFF if s16 else 0xFF), 2 if s16 else 1)
            elif mode == "dtls12":
                a[s + 1], a[s + 2] = 0xFE, 0xFD
                put(s + 11, (lens[i] + 24) & 0xFFFF, 2)
                if i in (PINNED["zero"], PINNED["u32_max"]):
                    a[s + 3:s + 11] = 0 if i == PINNED["zero"] else 0xFF
            elif rtp:
                cc, ext = HEADERS[i % 6]
                a[s] = 0x80 | (int(a[s]) & 0x20) | (0x10 if ext is not None else 0) | cc
                if ext is not None:
                    put(s + 12 + 4 * cc + 2, ext, 2)
                if i in (PINNED["zero"], PINNED["u32_max"]):
                    put(s + 2, 0 if i == PINNED["zero"] else 0xFFFF, 2)
            elif self.rtcp:
                a[s] = 0x80 | (int(a[s]) & 0x3F)
                put(e - tr, (0 if self.auth_only else 1 << 31) | self.index[i], 4)
        a.setflags(write=False)
        self.arena = a
        if quic:
            self.pn_off = [self.pn_offs(i) for i in range(n)]
            self.pn_len = [self.pn_lens(i) for i in range(n)]
            self.long = [LONG_FORM[i % 5] for i in range(n)]
            d = splitmix(seed + 3, n)
            # the number a receiver expects: at most min(half a window - 1, 100) below the packet's own, so that RFC 9000 A.3 decodes it
            self.expected_pns = [max(0, pn - int(x) % (min((1 << (8 * pl - 1)) - 1, 100) + 1)) for pn, pl, x in zip(self.nums, self.pn_len, d)]
        if d13:
            self.cid = [CIDS[i % 4] for i in range(n)]
            self.sn_off = [1 + c for c in self.cid]
            self.s16 = [S16[i % 3] for i in range(n)]
            self.with_len = [WITH_LEN[i % 5] for i in range(n)]
            d = splitmix(seed + 3, n)
            # as QUIC's: half a window - 1 is 127 or 32767, so at most 100 below
            self.expected_seqs = [max(0, q - int(x) % (min((1 << (15 if s else 7)) - 1, 100) + 1)) for q, s, x in zip(self.nums, self.s16, d)]
        if rtp:
            self.kind = [HEADERS[i % 6] for i in range(n)]
        self.forged = PG.forged(n)
        self.check()

    def na(self, i):
        """AAD blocks of frame i"""
        if self.nas:
            return (self.fronts[i] + 15) // 16
        if self.auth_only:
            return (self.fronts[i] + self.lens[i] + self.aad_extra + 15) // 16
        return MODES[self.mode][3]

    def start(self, i):
        """the arena offset whose residue the cells count: the payload's first byte (auth-only: the frame's)"""
        return self.at[i] + (0 if self.auth_only else self.fronts[i])

    def tag_at(self, i):
        """where frame i's ICV starts, from the frame's first byte"""
        return self.flen[i] - self.trail[i] - self.tag_len

    def part(self, i, off):
        """the part of frame i that its byte `off` lies in: front, payload (auth-only: the body behind the header), tag or trailer"""
        assert 0 <= off < self.flen[i], (i, off)
        t = self.tag_at(i)
        return "front" if off < min(self.fronts[i], t) else "payload" if off < t else "tag" if off < t + self.tag_len else "trailer"

    def where(self, x, shift=0):
        """the arena byte x of an arena laid out like this grid's `shift` bytes on -> (frame, byte within it, part); a byte of the guards in front of or behind
        the frames -> (the next frame behind it, None, "guard")"""
        j, off = PG.owner([a + shift for a in self.at], self.flen, x)
        return (j, None, "guard") if off is None else (j, off, self.part(j, off))

    def check(self):
        """completeness: every required cell occurred"""
        n = self.n
        seen16 = {(self.start(i) % 16, self.lens[i]) for i in range(n)}
        seen128 = {(self.start(i) % 128, self.lens[i]) for i in range(n)}
        miss16 = [(r, L) for L in self.full for r in range(16) if (r, L) not in seen16]
        miss128 = [(r, L) for L in self.lc for r in range(128) if (r, L) not in seen128]
        assert not miss16 and not miss128, (self.mode, "grid incomplete", miss16[:5], miss128[:5])
        assert set(range(273)) <= set(self.full) and set(PG.compact_lengths()) <= set(self.lc)
        assert int(self.off[0]) == PG.GUARD and all(self.at[i] + self.flen[i] == int(self.off[i + 1]) for i in range(n))
        assert set(self.trail) == {TRAILS.get(self.mode, 0)}
        # slot edges: n_seq = AAD blocks + payload blocks at G - 1, G, G + 1, 2 G - 1, 2 G, 2 G + 1, the last block a byte short, whole, a byte over
        nct = lambda i: 0 if self.auth_only else (self.lens[i] + 15) // 16
        body = lambda i: self.fronts[i] + self.lens[i] + self.aad_extra if self.auth_only else self.lens[i]
        seen = {(self.na(i) + nct(i), body(i) % 16) for i in range(n)}
        if self.nas:
            seen = {(self.na(i), self.na(i) + nct(i), body(i) % 16) for i in range(n)}
            assert {self.na(i) for i in range(n)} == set(self.nas)
        for G in LANES:
            for m in _M(G):
                for nas in (self.nas or (None,)):
                    key = (lambda *k: k if nas is None else (nas,) + k)
                    # 16 x + 15 and 16 x fill x + 1 resp. x blocks, 16 x + 1 one more: a byte short of, at, and a byte over m slots
                    assert key(m, 15) in seen and key(m, 0) in seen and key(m + 1, 1) in seen, (self.mode, "slot edge missing", G, m, nas)
        icv = {(self.at[i] + self.tag_at(i)) % 16 for i in range(n)}
        assert icv == set(range(16)), (self.mode, "ICV residues", sorted(icv))
        assert all(self.slots[i] != self.slots[i + 1] for i in range(n - 1)) and set(self.slots) == set(range(N_AEAD))
        first = lambda i: int(self.arena[self.at[i]])
        if self.nums is not None:
            lim = 2 ** 32 if self.number in ("hi", "roc") else 2 ** 62 if self.family == "quic" else 2 ** 64
            assert all(0 <= x < lim for x in self.nums) and self.nums[PINNED["zero"]] == 0 and self.nums[PINNED["u32_max"]] == 2 ** 32 - 1
            assert self.number in ("hi", "roc") or self.nums[PINNED["two_32"]] == 2 ** 32
        if self.hps is not None:
            assert all(self.hps[i] != self.hps[i + 1] for i in range(n - 1)) and set(self.hps) == set(range(N_AEAD, N_AEAD + N_HP))
        if self.family == "quic":
            assert self.nums[PINNED["two_62_less_1"]] == 2 ** 62 - 1
            assert set(self.pn_off) == set(range(1, 52)) and max(self.pn_off) >= 50 and {self.na(i) for i in range(n)} == {1, 2, 3, 4}
            assert {(po, pl, lg) for po, pl, lg in zip(self.pn_off, self.pn_len, self.long)} == {(po, pl, lg) for po in range(1, 52) for pl in (1, 2, 3, 4) for lg in (False, True)}
            assert all(pl + L >= 4 for pl, L in zip(self.pn_len, self.lens))
            samp = {((self.at[i] + self.pn_off[i] + 4) % 16, self.pn_len[i], self.long[i]) for i in range(n)}
            miss = [(r, pl, lg) for r in range(16) for pl in (1, 2, 3, 4) for lg in (False, True) if (r, pl, lg) not in samp]
            assert not miss, ("sample cells missing", miss[:8])
            assert all((first(i) & 3) + 1 == self.pn_len[i] and bool(first(i) & 0x80) == self.long[i] for i in range(n))
        if self.mode == "dtls13":
            assert self.nums[PINNED["two_64_less_1"]] == 2 ** 64 - 1 and {x.bit_length() > 48 for x in self.nums} == {False, True}
            assert all(0 <= q - e <= 100 for q, e in zip(self.nums, self.expected_seqs)) and len({q - e for q, e in zip(self.nums, self.expected_seqs)}) > 50
            assert all(self.fronts[i] == self.sn_off[i] + (2 if self.s16[i] else 1) + (2 if self.with_len[i] else 0) for i in range(n))
            assert min(self.fronts) == 2 and max(self.fronts) == 25
            assert all(first(i) >> 5 == 1 and bool(first(i) & 0x10) == (self.cid[i] > 0) and bool(first(i) & 8) == self.s16[i] and bool(first(i) & 4) == self.with_len[i]
                       for i in range(n))
            hk = {(self.start(i) % 16, self.cid[i], self.s16[i], self.with_len[i]) for i in range(n)}
            miss = [(r, c, s, w) for r in range(16) for c in CIDS for s in (False, True) for w in (False, True) if (r, c, s, w) not in hk]
            assert not miss, ("header cells missing", miss[:8])
        if self.mode == "dtls12":
            z, f = self.at[PINNED["zero"]], self.at[PINNED["u32_max"]]
            assert not self.arena[z + 3:z + 11].any() and (self.arena[f + 3:f + 11] == 0xFF).all()
        if self.mode in ("srtp", "srtp_mki"):
            assert all(self.fronts[i] == rtp_hdr_len(self.kind[i]) for i in range(n)) and [rtp_hdr_len(k) for k in HEADERS] == [12, 16, 72, 16, 24, 96]
            hk = {(self.start(i) % 16, self.kind[i]) for i in range(n)}
            miss = [(r, k) for r in range(16) for k in HEADERS if (r, k) not in hk]
            assert not miss, ("header cells missing", miss[:8])
            for i in range(n):                                            # the header says what the kind says
                cc, ext = self.kind[i]
                b = self.arena[self.at[i]:self.at[i] + self.fronts[i]]
                assert b[0] >> 6 == 2 and b[0] & 15 == cc and bool(b[0] & 0x10) == (ext is not None)
                assert ext is None or (int(b[12 + 4 * cc + 2]) << 8 | int(b[12 + 4 * cc + 3])) == ext
            seq = lambda i: int(self.arena[self.at[i] + 2]) << 8 | int(self.arena[self.at[i] + 3])
            assert seq(PINNED["zero"]) == 0 and seq(PINNED["u32_max"]) == 0xFFFF
            assert {x.bit_length() > 16 for x in self.nums} == {False, True} and 1 in self.nums
        if self.rtcp:
            w = lambda i: int.from_bytes(self.arena[self.at[i] + self.tag_at(i) + 16:self.at[i] + self.tag_at(i) + 20].tobytes(), "big")
            assert all(first(i) >> 6 == 2 and w(i) >> 31 == (0 if self.auth_only else 1) and w(i) & 0x7FFFFFFF == self.index[i] for i in range(n))
            assert self.index[PINNED["zero"]] == 0 and self.index[PINNED["u32_max"]] == 2 ** 31 - 1 and all(0 <= x < 2 ** 31 for x in self.index)
        if self.mode == "srtcp_clear":
            # the seam between the packet's bytes and W in the AAD: every (packet start, seam) on AADs of one block (x = 0 .. 4: no other seam fits), two, and nine or more
            for blocks, seams in ((lambda b: b == 1, range(8, 13)), (lambda b: b == 2, range(16)), (lambda b: b >= 9, range(16))):
                have = {(self.at[i] % 16, (8 + self.lens[i]) % 16) for i in range(n) if blocks(self.na(i))}
                miss = [(r, s) for r in range(16) for s in seams if (r, s) not in have]
                assert not miss, ("seam cells missing", miss[:8])

    def frames(self, arena=None):
        """the frames of an arena laid out like this grid's (default: its own plaintext), as bytes"""
        b = (self.arena if arena is None else arena).tobytes()
        return [b[self.at[i]:self.at[i] + self.flen[i]] for i in range(self.n)]

    def cell(self, i):
        """what frame i is; icv_res is its tag's start mod 16"""
        c = dict(frame=i, start_res=self.start(i) % 16, start_res128=self.start(i) % 128, length=self.lens[i], tag_len=self.tag_len, na=self.na(i), slot=self.slots[i],
                 icv_res=(self.at[i] + self.tag_at(i)) % 16)
        if self.nums is not None:
            c[self.number] = self.nums[i]
        if self.family == "quic":
            c.update(pn_off=self.pn_off[i], pn_len=self.pn_len[i], long=self.long[i], sample_res=(self.at[i] + self.pn_off[i] + 4) % 16)
        if self.family in ("dtls", "srtp"):
            c.update(front=self.fronts[i], trail=self.trail[i])
        if self.mode == "dtls13":
            c.update(cid=self.cid[i], s16=self.s16[i], with_len=self.with_len[i], expected=self.expected_seqs[i], sn_slot=self.hps[i])
        if self.mode in ("srtp", "srtp_mki"):
            c.update(kind=self.kind[i], rtp_seq=int(self.arena[self.at[i] + 2]) << 8 | int(self.arena[self.at[i] + 3]))
        if self.rtcp:
            c.update(index=self.index[i], seam=(8 + self.lens[i]) % 16 if self.auth_only else None)
        return c


_GRIDS = {}


def grid(mode):
    """the mode's grid, built once"""
    if mode not in _GRIDS:
        _GRIDS[mode] = Grid(mode)
    return _GRIDS[mode]


def length_classes(g):
    """the classes order_launch sorts by (aesgcm_pkt.h, pkt_len_class: 64 bytes of frame each, 256 classes)"""
    return sorted({min(L >> 6, 255) for L in g.flen})
