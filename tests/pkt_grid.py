"""The alignment grid of the packet kernels: one deterministic generator for the GPU tests (tests/test_gpu_pkt_grid.py) and for the CPU check of the
generator itself (tests/test_pkt_grid_cpu.py); tests/host_emul/emul.cpp restates the same rules in C++ for the lane code run on the host.

What the lane code can get wrong is a shift or a store for ONE (address & 15, length & 15) pair, a loop boundary that meets a 128-byte line, or a store that spills
into the neighbouring packet.  So the grid is made of CELLS that must all occur, and every arena is compared whole:

  packed form      one byte-packed buffer and an offset array: every (start mod 16, length) for all lengths, every (start mod 128, length) for the compact
                   set L_c; filler packets of 0 .. 127 bytes steer the starts and are ordinary packets, checked like the rest
  scattered form   arrays of addresses and lengths: every (input residue, output residue) of 16 x 16 for every length of L_c, 1 .. 19 guard bytes between
                   neighbours in both arenas; the in-place variant has every (residue, length) for all lengths
  AAD              lengths cycle with period 13 (coprime to the residues' 16 and 128 and to the forged tags' 7), byte-packed or at cycling residues behind guards

Every arena has GUARD bytes of canary in front and behind.  The generator asserts that every required cell occurred: a grid that lost a part fails."""
import numpy as np

GUARD = 256                       # bytes of canary in front of and behind every arena (also the margin that keeps a kernel that is off by a line inside the allocation)
CANARY_IN, CANARY_OUT = 0xC3, 0x5E
AAD_CYCLE = (0, 1, 12, 15, 16, 17, 20, 28, 31, 32, 33, 40, 20)          # the twelve lengths and one repeat: period 13
GROUPS = (4, 8, 16, 64)
FORGE_EVERY = 7


def group_edges(G):
    """16 m + d around the turns of a group of G lanes: m blocks fill G - 1, G, G + 1, 2 G - 1, 2 G, 2 G + 1 slots"""
    return sorted({16 * m + d for m in (G - 1, G, G + 1, 2 * G - 1, 2 * G, 2 * G + 1) for d in (-1, 0, 1)})


def all_lengths():
    """every length 0 .. 272 (two lines and a block) and the group edges of every lane group"""
    s = set(range(273))
    for G in GROUPS:
        s.update(group_edges(G))
    return sorted(s)


def compact_lengths(G=0):
    """L_c: the edges of the lane's loops (block, 64-byte group, 128-byte line, ragged end) and the group edges of the shape under test (G lanes, 0 = none)"""
    s = {0, 1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 79, 80, 81, 111, 112, 113, 127, 128, 129, 143, 144, 145, 191, 192, 193, 255, 256, 257, 271, 272}
    if G:
        s.update(group_edges(G))
    return sorted(s)


def forged(n):
    """about one tag in seven, packets 0 and n - 1 among them"""
    return sorted(set(range(0, n, FORGE_EVERY)) | {n - 1})


def pack(full, lc, front=None, span=None, allowed=None, prefer=None):
    """The placement loop: byte-packed packets such that every (start mod 16, L) for L in `full` and every (start mod 128, L) for L in `lc` occurs -> the lengths
    in order.  Packet i of length L at `pos` occupies span(i, L) bytes and the start that counts is pos + front(i) (defaults: the packet is its L bytes and starts
    at pos -- the packet kernels' grid; tests/kt_grid.py places frames header | payload | ICV by their payload).  allowed(i, L): whether packet i may have length L;
    prefer(i): a length that packet i takes in front of every other choice, or None."""
    front = front or (lambda i: 0)
    span = span or (lambda i, L: L)
    allowed = allowed or (lambda i, L: True)
    need16 = {r: set(full) for r in range(16)}
    need128 = {r: set(lc) for r in range(128)}
    left = 16 * len(full) + 128 * len(lc)
    lens, pos = [], 0
    order16 = {r: sorted(need16[r], reverse=True) for r in range(16)}          # deterministic: longest first, so that the fillers (short) find their own cells taken late
    order128 = {r: sorted(need128[r], reverse=True) for r in range(128)}

    def put(L):
        nonlocal pos, left
        r = (pos + front(len(lens))) % 128
        if L in need128[r]:
            need128[r].discard(L); left -= 1
        if L in need16[r % 16]:
            need16[r % 16].discard(L); left -= 1
        pos += span(len(lens), L)
        lens.append(L)

    def pick(r, i):
        while order128[r] and order128[r][0] not in need128[r]:
            order128[r].pop(0)
        for L in order128[r]:
            if L in need128[r] and allowed(i, L):
                return L
        q = order16[r % 16]
        while q and q[0] not in need16[r % 16]:
            q.pop(0)
        for L in q:
            if L in need16[r % 16] and allowed(i, L):
                return L
        return None

    while left:
        i = len(lens)
        L = prefer(i) if prefer else None
        if L is None:
            L = pick((pos + front(i)) % 128, i)
        if L is None:                                                          # nothing left at this start: a filler to the nearest start that still needs a packet
            f = next((f for f in range(1, 128) if allowed(i, f) and pick((pos + span(i, f) + front(i + 1)) % 128, i + 1) is not None), None)
            put(f if f is not None else next(f for f in range(1, 128) if allowed(i, f)))       # (no start that the next packet may take: any filler, the one after it steers)
            continue
        put(L)
    return lens


class Packed:
    """n byte-packed packets: doff / aoff have n + 1 entries, offsets from the arena's first byte (doff[0] = aoff[0] = GUARD); the arenas are doff[n] + GUARD
    and aoff[n] + GUARD bytes.  With the arena on a 128-byte boundary a packet's residues are doff[i] % 16 and % 128."""

    def __init__(self, G=0):
        full, lc = all_lengths(), compact_lengths(G)
        lens = pack(full, lc)
        self.G, self.n, self.lens = G, len(lens), lens
        self.aads = [AAD_CYCLE[i % len(AAD_CYCLE)] for i in range(self.n)]
        self.doff = np.concatenate(([GUARD], GUARD + np.cumsum(lens))).astype(np.uint64)
        self.aoff = np.concatenate(([GUARD], GUARD + np.cumsum(self.aads))).astype(np.uint64)
        self.size, self.aad_size = int(self.doff[-1]) + GUARD, int(self.aoff[-1]) + GUARD
        self.check(full, lc)

    def check(self, full, lc):
        """completeness: every required cell occurred, fillers are 0 .. 127 bytes or required lengths, AAD starts vary"""
        seen16 = {(int(o) % 16, L) for o, L in zip(self.doff[:-1], self.lens)}
        seen128 = {(int(o) % 128, L) for o, L in zip(self.doff[:-1], self.lens)}
        miss16 = [(r, L) for L in full for r in range(16) if (r, L) not in seen16]
        miss128 = [(r, L) for L in lc for r in range(128) if (r, L) not in seen128]
        assert not miss16 and not miss128, ("packed grid incomplete", miss16[:5], miss128[:5])
        assert set(range(273)) <= set(full) and all(set(group_edges(g)) <= set(full) for g in GROUPS) and 34 <= len(lc) <= 60 and set(lc) <= set(full)
        assert self.n == len(self.lens) == len(self.aads) and int(self.doff[0]) == GUARD and int(self.doff[-1]) == GUARD + sum(self.lens)
        assert {int(o) % 16 for o in self.aoff[:-1]} == set(range(16)) and set(self.aads) == set(AAD_CYCLE)

    def cell(self, i):
        return dict(pkt=i, in_res=int(self.doff[i]) % 16, in_res128=int(self.doff[i]) % 128, length=self.lens[i], aad=self.aads[i], aad_res=int(self.aoff[i]) % 16)


def _place(pos, res, i):
    """the next address behind `pos` with residue `res` that leaves 1 .. 19 guard bytes"""
    g = (res - (pos + 1)) % 16 + 1
    if g <= 3 and i % 2:
        g += 16
    return pos + g


class Scattered:
    """messages wherever they live: pos_in / pos_out / pos_aad are offsets from the first byte of three arenas (size_in, size_out, size_aad; GUARD bytes in front
    and behind), 1 .. 19 guard bytes between neighbours.  inplace: one arena (pos_out is pos_in), every residue for all lengths; else every (input residue, output
    residue) pair for every length of L_c."""

    AADS = AAD_CYCLE

    def lengths(self):
        """the lengths whose every cell must occur (tests/rows_grid.py lays its own lengths and AAD cycle out by the same rules)"""
        return all_lengths() if self.inplace else compact_lengths(self.G)

    def __init__(self, G=0, inplace=False):
        self.G, self.inplace = G, inplace
        self.lay(self.order())
        self.check()

    def order(self):
        """the cells (input residue, output residue, length), neighbours of unlike length and residue: a stride coprime to the count walks the cells"""
        cells = [(a, a, L) for L in self.lengths() for a in range(16)] if self.inplace else [(a, b, L) for L in self.lengths() for a in range(16) for b in range(16)]
        n = len(cells)
        step = next(s for s in range(n // 3 | 1, n, 2) if np.gcd(s, n) == 1)
        return [cells[(k * step) % n] for k in range(n)]

    def lay(self, order, aads=None):
        """place the messages of `order` in the three arenas; aads: their AAD lengths (default: the cycle)"""
        n = len(order)
        self.n, self.lens = n, [c[2] for c in order]
        self.aads = list(aads) if aads is not None else [self.AADS[i % len(self.AADS)] for i in range(n)]
        self.pos_in, self.pos_out, self.pos_aad = [], [], []
        a = b = c = GUARD - 1
        for i, (ra, rb, L) in enumerate(order):
            a = _place(a, ra, i); self.pos_in.append(a); a += L
            b = _place(b, rb, i + 1); self.pos_out.append(b); b += L
            c = _place(c, (5 * i + 3) % 16, i); self.pos_aad.append(c); c += self.aads[i]
        if self.inplace:
            self.pos_out = self.pos_in
        self.size_in, self.size_out, self.size_aad = a + 1 + GUARD, (a if self.inplace else b) + 1 + GUARD, c + 1 + GUARD

    def check(self):
        lens = self.lengths()
        seen = {(p % 16, q % 16, L) for p, q, L in zip(self.pos_in, self.pos_out, self.lens)}
        want = {(a, a, L) for L in lens for a in range(16)} if self.inplace else {(a, b, L) for L in lens for a in range(16) for b in range(16)}
        assert want <= seen and len(self.lens) == self.n == len(want), ("scattered grid incomplete", sorted(want - seen)[:5])
        for pos, ln in ((self.pos_in, self.lens), (self.pos_out, self.lens), (self.pos_aad, self.aads)):
            assert pos[0] >= GUARD
            gaps = [pos[i + 1] - (pos[i] + ln[i]) for i in range(self.n - 1)]
            assert min(gaps) >= 1 and max(gaps) <= 19, (min(gaps), max(gaps))
        assert {p % 16 for p in self.pos_aad} == set(range(16))

    def cell(self, i):
        return dict(msg=i, in_res=self.pos_in[i] % 16, out_res=self.pos_out[i] % 16, length=self.lens[i], aad=self.aads[i], aad_res=self.pos_aad[i] % 16)


def first_difference(got, want):
    """index of the first byte at which two equally long byte arrays differ, or None"""
    g, w = np.frombuffer(got, dtype=np.uint8), np.frombuffer(want, dtype=np.uint8)
    assert g.size == w.size, (g.size, w.size)
    d = np.flatnonzero(g != w)
    return int(d[0]) if d.size else None


def owner(starts, lens, at):
    """which packet the arena byte `at` belongs to: (index, byte within it); for a guard byte (index of the next packet behind it, None)"""
    starts = np.asarray(starts, dtype=np.int64)
    ends = starts + np.asarray(lens, dtype=np.int64)                   # nondecreasing in both forms
    j = int(np.searchsorted(ends, at, side="right"))
    if j < len(lens) and starts[j] <= at:
        return j, at - int(starts[j])
    return j, None
