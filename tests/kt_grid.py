"""The alignment grid of the key-table family: wire frames (MACsec, ESP), their 64-bit-number forms (XPN, ESN), TLS records and QUIC packets.  One deterministic
generator (numpy only, no GPU) for tests/test_gpu_kt_grid.py and for the CPU check of the generator itself (tests/test_kt_grid_cpu.py).

All of these run the text of aesgcm_batch3_body.inc under WIRE / WIREX: a nonce loaded from the middle of a header, an ICV of 8, 12 or 16 bytes whose dword accesses
must end at the frame's end, wire_copy_front's overlapping last piece, AAD blocks built in registers, QUIC's header length per packet and k_kt_quic_hp's sample at any
address.  What such code gets wrong is one (address & 15, length & 15) pair, a turn of the lane group's loop, or a store that spills into the neighbour.  So a grid is
one byte-packed buffer of frames front | payload | ICV with its offset array, made of CELLS that must all occur, placed by pkt_grid.pack (the packet kernels' own loop):

  residue by length   every (payload start mod 16, payload length) for lengths 0 .. 272 and the mode's slot edges; every (payload start mod 128, length) for
                      pkt_grid.compact_lengths() and the slot edges.  The auth-only format has no payload: there the start is the frame's and the length is what
                      its body has behind the header (the body, header included, is the AAD).
  slot edges          a frame is na AAD blocks and its payload blocks, G of them per turn of its lane group: payload lengths 16 (m - na) + d for
                      m in G - 1, G, G + 1, 2 G - 1, 2 G, 2 G + 1, d in -1, 0, 1 and G in 8, 16, 64 -- one grid per mode for all three lane counts.  QUIC's na is the
                      packet's own (1 .. 4 blocks of header): every (na, G, m, d) occurs on a packet with that na; the residue cells of QUIC are those of the lengths
                      0 .. 272 and of compact_lengths().
  ICV placement       every ICV start mod 16 (follows from the above; asserted)
  QUIC header         pn_len cycles 1 .. 4, pn_off through a permutation of 1 .. 51 (period 51), long and short first bytes with period 5: every combination occurs;
                      every (sample address (start + pn_off + 4) mod 16, pn_len, form) of the 16 x 4 x 2 occurs; pn_len + payload >= 4 (the sample lies in the packet)
  numbers             hi / seq / pn from a seeded stream; 0, 2^32 - 1, 2^32 and (QUIC) 2^62 - 1 pinned on the packets PINNED names (hi is 32 bits wide: 0 and 2^32 - 1)
  slots               packet i takes AEAD slot i mod 11 (QUIC: header-protection slot 11 + i mod 5): neighbours never share a key

Fillers are ordinary frames, checked like the rest.  Every arena has pkt_grid.GUARD canary bytes in front and behind.  The generator asserts that every required cell
occurred (Grid.check): a grid that lost a part fails."""
import numpy as np

import pkt_grid as PG

LANES = (8, 16, 64)
N_AEAD, N_HP = 11, 5
PLACEHOLDER = 0xAA                                     # where the ICV goes in a plaintext frame
PINNED = {"zero": 0, "u32_max": 1, "two_32": 2, "two_62_less_1": 3}        # packet indices
PN_OFFS = tuple((20 * k) % 51 + 1 for k in range(51))                    # a permutation of 1 .. 51: period 51, coprime to 4, 16 and 5
LONG_FORM = (False, True, False, False, True)                            # period 5

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
}
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


class Grid:
    """n frames of one mode.  off has n + 1 entries, offsets from the arena's first byte (off[0] = GUARD); the arena is off[n] + GUARD bytes: canary, the plaintext
    frames (seeded front and payload, PLACEHOLDER where the ICV goes), canary.  lens: what the cells count (payload bytes; auth-only: body bytes behind the header);
    fronts: the bytes in front of that."""

    def __init__(self, mode):
        self.mode = mode
        self.family, hdr, self.tag_len, na, self.auth_only, self.number = MODES[mode]
        quic = self.family == "quic"
        self.lc = PG.compact_lengths()
        if quic:
            self.full = list(range(273))
            self.pn_lens = lambda i: 1 + i % 4
            self.pn_offs = lambda i: PN_OFFS[i % 51]
            front = lambda i: self.pn_offs(i) + self.pn_lens(i)
            na_of = lambda i: (front(i) + 15) // 16
            allowed = lambda i, L: self.pn_lens(i) + L >= 4
            want = {(a, L) for a in (1, 2, 3, 4) for L in slot_edges(a)}
            self.edge_cells = sorted(want)

            def prefer(i):
                c = [L for (a, L) in want if a == na_of(i) and allowed(i, L)]
                if not c:
                    return None
                want.discard((na_of(i), max(c)))
                return max(c)
            lens = PG.pack(self.full, self.lc, front=front, span=lambda i, L: front(i) + L + 16, allowed=allowed, prefer=prefer)
            assert not want
        else:
            edges = slot_edges(0, less=hdr) if self.auth_only else slot_edges(na)
            self.full = sorted(set(range(273)) | set(edges))
            self.lc = sorted(set(self.lc) | set(edges))
            self.edge_cells = edges
            cell_front = 0 if self.auth_only else hdr                     # where the counted start lies in the frame
            front = lambda i: hdr
            lens = PG.pack(self.full, self.lc, front=lambda i: cell_front, span=lambda i, L: hdr + L + self.tag_len)
        n = self.n = len(lens)
        self.lens = lens
        self.fronts = [front(i) for i in range(n)]
        flen = [f + L + self.tag_len for f, L in zip(self.fronts, lens)]
        self.off = np.concatenate(([PG.GUARD], PG.GUARD + np.cumsum(flen))).astype(np.uint64)
        self.size = int(self.off[-1]) + PG.GUARD
        self.at = [int(x) for x in self.off[:-1]]
        self.flen = flen
        self.slots = [i % N_AEAD for i in range(n)]
        self.hps = [N_AEAD + i % N_HP for i in range(n)] if quic else None
        seed = 0x6B740000 + 97 * sorted(MODES).index(mode)
        # ---- the numbers that are not on the wire
        self.nums = None
        if self.number:
            w = splitmix(seed + 1, n)
            if self.number == "hi":
                nums = [int(x) & 0xFFFFFFFF for x in w]
                nums[PINNED["zero"]], nums[PINNED["u32_max"]] = 0, 2 ** 32 - 1
            else:
                bits = (8, 16, 31, 33, 62) if quic else (64,)
                nums = [int(x) >> (64 - bits[i % len(bits)]) for i, x in enumerate(w)]
                nums[PINNED["zero"]], nums[PINNED["u32_max"]], nums[PINNED["two_32"]] = 0, 2 ** 32 - 1, 2 ** 32
                if quic:
                    nums[PINNED["two_62_less_1"]] = 2 ** 62 - 1
            self.nums = nums
        # ---- the arena
        a = np.full(self.size, PG.CANARY_IN, dtype=np.uint8)
        r = splitmix(seed + 2, (self.size + 7) // 8).view(np.uint8)
        for i in range(n):
            s, e = self.at[i], self.at[i] + flen[i]
            a[s:e - self.tag_len] = r[s:e - self.tag_len]
            a[e - self.tag_len:e] = PLACEHOLDER
            if quic:
                po, pl = self.pn_offs(i), self.pn_lens(i)
                a[s] = (int(a[s]) & 0x7C) | (pl - 1) | (0x80 if LONG_FORM[i % 5] else 0)
                a[s + po:s + po + pl] = np.frombuffer((self.nums[i] & ((1 << (8 * pl)) - 1)).to_bytes(pl, "big"), dtype=np.uint8)
        a.setflags(write=False)
        self.arena = a
        if quic:
            self.pn_off = [self.pn_offs(i) for i in range(n)]
            self.pn_len = [self.pn_lens(i) for i in range(n)]
            self.long = [LONG_FORM[i % 5] for i in range(n)]
            d = splitmix(seed + 3, n)
            # the number a receiver expects: at most min(half a window - 1, 100) below the packet's own, so that RFC 9000 A.3 decodes it
            self.expected_pns = [max(0, pn - int(x) % (min((1 << (8 * pl - 1)) - 1, 100) + 1)) for pn, pl, x in zip(self.nums, self.pn_len, d)]
        self.forged = PG.forged(n)
        self.check()

    def na(self, i):
        """AAD blocks of frame i"""
        if self.family == "quic":
            return (self.fronts[i] + 15) // 16
        if self.auth_only:
            return (self.fronts[i] + self.lens[i] + 15) // 16
        return MODES[self.mode][3]

    def start(self, i):
        """the arena offset whose residue the cells count: the payload's first byte (auth-only: the frame's)"""
        return self.at[i] + (0 if self.auth_only else self.fronts[i])

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
        # slot edges: n_seq = AAD blocks + payload blocks at G - 1, G, G + 1, 2 G - 1, 2 G, 2 G + 1, the last block a byte short, whole, a byte over
        nct = lambda i: 0 if self.auth_only else (self.lens[i] + 15) // 16
        body = lambda i: self.fronts[i] + self.lens[i] if self.auth_only else self.lens[i]
        seen = {(self.na(i) + nct(i), body(i) % 16) for i in range(n)}
        if self.family == "quic":
            seen = {(self.na(i), self.na(i) + nct(i), body(i) % 16) for i in range(n)}
        for G in LANES:
            for m in _M(G):
                for nas in ((1, 2, 3, 4) if self.family == "quic" else (None,)):
                    key = (lambda *k: k if nas is None else (nas,) + k)
                    # 16 x + 15 and 16 x fill x + 1 resp. x blocks, 16 x + 1 one more: a byte short of, at, and a byte over m slots
                    assert key(m, 15) in seen and key(m, 0) in seen and key(m + 1, 1) in seen, (self.mode, "slot edge missing", G, m, nas)
        icv = {(int(self.off[i + 1]) - self.tag_len) % 16 for i in range(n)}
        assert icv == set(range(16)), (self.mode, "ICV residues", sorted(icv))
        assert all(self.slots[i] != self.slots[i + 1] for i in range(n - 1)) and set(self.slots) == set(range(N_AEAD))
        if self.nums is not None:
            lim = 2 ** 32 if self.number == "hi" else 2 ** 62 if self.family == "quic" else 2 ** 64
            assert all(0 <= x < lim for x in self.nums) and self.nums[PINNED["zero"]] == 0 and self.nums[PINNED["u32_max"]] == 2 ** 32 - 1
            assert self.number == "hi" or self.nums[PINNED["two_32"]] == 2 ** 32
        if self.family == "quic":
            assert self.nums[PINNED["two_62_less_1"]] == 2 ** 62 - 1
            assert all(self.hps[i] != self.hps[i + 1] for i in range(n - 1)) and set(self.hps) == set(range(N_AEAD, N_AEAD + N_HP))
            assert set(self.pn_off) == set(range(1, 52)) and max(self.pn_off) >= 50 and {self.na(i) for i in range(n)} == {1, 2, 3, 4}
            assert {(po, pl, lg) for po, pl, lg in zip(self.pn_off, self.pn_len, self.long)} == {(po, pl, lg) for po in range(1, 52) for pl in (1, 2, 3, 4) for lg in (False, True)}
            assert all(pl + L >= 4 for pl, L in zip(self.pn_len, self.lens))
            samp = {((self.at[i] + self.pn_off[i] + 4) % 16, self.pn_len[i], self.long[i]) for i in range(n)}
            miss = [(r, pl, lg) for r in range(16) for pl in (1, 2, 3, 4) for lg in (False, True) if (r, pl, lg) not in samp]
            assert not miss, ("sample cells missing", miss[:8])
            assert all((int(self.arena[self.at[i]]) & 3) + 1 == self.pn_len[i] and bool(int(self.arena[self.at[i]]) & 0x80) == self.long[i] for i in range(n))

    def frames(self, arena=None):
        """the frames of an arena laid out like this grid's (default: its own plaintext), as bytes"""
        b = (self.arena if arena is None else arena).tobytes()
        return [b[self.at[i]:self.at[i] + self.flen[i]] for i in range(self.n)]

    def cell(self, i):
        c = dict(frame=i, start_res=self.start(i) % 16, start_res128=self.start(i) % 128, length=self.lens[i], tag_len=self.tag_len, na=self.na(i), slot=self.slots[i],
                 icv_res=(int(self.off[i + 1]) - self.tag_len) % 16)
        if self.nums is not None:
            c[self.number] = self.nums[i]
        if self.family == "quic":
            c.update(pn_off=self.pn_off[i], pn_len=self.pn_len[i], long=self.long[i], sample_res=(self.at[i] + self.pn_off[i] + 4) % 16)
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
