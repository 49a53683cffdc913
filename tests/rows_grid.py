"""The alignment grid at ROW scale: one deterministic generator for the GPU tests of the row kernels and of routed calls (tests/test_gpu_rows_grid.py) and for the CPU
check of the generator itself (tests/test_rows_grid_cpu.py); tests/host_emul/emul.cpp (test_rows_grid) restates the same rules in C++ for the lane code run on the host.

tests/pkt_grid.py ends where the row code (k_rows / k_rows_close, csrc/aesgcm_rows.h) begins to do work of its own: a message of 1024 R + t bytes is R whole rows of 64
blocks (a RUN of rows is one piece of body_rows_lane, with lane constants for four row phases), a tail of up to 64 blocks (up to SMALL_TAIL = 16 of them a lane each of
the closing launch; more: one right-aligned row of the row launch) and an AAD (up to SMALL_AAD = 64 blocks on the closing launch's axis; more: rows of its own).  So the
cells here are made of those numbers, placed and checked by pkt_grid's own machinery (pack, _place, the canaries, forged, first_difference, owner):

  packed form      every (start mod 16, length) for `full_lengths` (R in 0 1 2 3 4 5 9 x tails either side of every boundary; below 257 bytes only with rows in front: the
                   rest is pkt_grid's already), every (start mod 128, length) for the dozen `lc_lengths`; fillers of 0 .. 127 bytes steer the starts
  scattered form   every (input residue, output residue) of 16 x 16 for the six SC_LENGTHS, 1 .. 19 guard bytes between neighbours in all three arenas; the in-place
                   variant has every (residue, length) of `full_lengths`
  AAD              period 13 (coprime to 16, 128 and the forged tags' 7), either side of SMALL_AAD; lengths 1024 and 1025 occur at EVERY AAD residue mod 16
  route grid       a ROUTED call sends messages of data + AAD below a mark to the packet kernels (the caller's stream) and the others by rows (the context's side
                   stream): two kernels write neighbouring messages of one byte-packed buffer at the same time.  Messages of mark - 1, mark and mark + 1 bytes, short and
                   long alternating, so that each of the three sizes lies in front of and behind a boundary between the two kernels at every residue of that boundary, and
                   all 32 (boundary residue, short-then-long / long-then-short) cells occur; messages of no bytes and of a quarter of the mark in between

The arenas hold a few thousand messages and about 10 MB (packed: R = 9 at every start mod 16 is a quarter of that; it is what may be cut from `full_lengths` -- never
from `lc_lengths` -- should the cases built on this grid take too long).  Every generator asserts that every required cell occurred: a grid that lost a part fails."""
import numpy as np

import pkt_grid as PG

# csrc/aesgcm_rows.h (tests/test_rows_grid_cpu.py reads them there too)
ROW = 1024                        # rows_geom: R = len >> 10, a row is 64 blocks
SMALL_TAIL = 16                   # ROWS_SMALL_TAIL: blocks of a tail up to which it lies on the smalls axis
SMALL_AAD = 64                    # ROWS_SMALL_AAD: blocks of an AAD up to which it lies on the smalls axis

FULL_R = (0, 1, 2, 3, 4, 5, 9)
FULL_T = (0, 1, 15, 16, 17, 255, 256, 257, 272, 511, 512, 1007, 1008, 1009, 1023)
AAD_CYCLE = (0, 1, 13, 16, 20, 1007, 1008, 1009, 1023, 1024, 1025, 1040, 2048 + 7)          # thirteen lengths: period 13
SC_LENGTHS = (700, 1024, 1025, 2048 + 257, 3 * 1024 + 1023, 4096 + 16)


def full_lengths():
    """1024 R + t either side of every boundary of the tail (block, SMALL_TAIL, half a row, the last block); R = 0 only from 257 bytes"""
    return sorted({ROW * R + t for R in FULL_R for t in FULL_T if R or t >= 257})


def lc_lengths():
    """placed at every start mod 128: a lone row, a row and a byte, a row and a tail of 16 / of 17 blocks, two rows + 1023, four rows, five rows + 17, a tail only, nine rows + 257"""
    return sorted({ROW, ROW + 1, ROW + 16 * SMALL_TAIL, ROW + 16 * SMALL_TAIL + 1, 2 * ROW + 1023, 4 * ROW, 5 * ROW + 17, 1023, 9 * ROW + 257})


def geometry(length, aad):
    """what the row code makes of a message: whole rows, blocks of its tail, blocks of its AAD"""
    return dict(R=length // ROW, tail_blocks=(length % ROW + 15) // 16, aad_blocks=(aad + 15) // 16)


def _aad_cells(aads, starts):
    """the AAD residues mod 16 at which the lengths either side of SMALL_AAD occur"""
    return {al: {int(s) % 16 for s, a in zip(starts, aads) if a == al} for al in (16 * SMALL_AAD, 16 * SMALL_AAD + 1)}


class Packed:
    """n byte-packed messages, as pkt_grid.Packed: doff / aoff have n + 1 entries, offsets from the arena's first byte (doff[0] = aoff[0] = GUARD)"""

    def __init__(self):
        full, lc = full_lengths(), lc_lengths()
        lens = PG.pack(full, lc)
        self.G, self.n, self.lens = 0, len(lens), lens
        self.aads = [AAD_CYCLE[i % len(AAD_CYCLE)] for i in range(self.n)]
        self.doff = np.concatenate(([PG.GUARD], PG.GUARD + np.cumsum(lens))).astype(np.uint64)
        self.aoff = np.concatenate(([PG.GUARD], PG.GUARD + np.cumsum(self.aads))).astype(np.uint64)
        self.size, self.aad_size = int(self.doff[-1]) + PG.GUARD, int(self.aoff[-1]) + PG.GUARD
        self.check(full, lc)

    def check(self, full, lc):
        seen16 = {(int(o) % 16, L) for o, L in zip(self.doff[:-1], self.lens)}
        seen128 = {(int(o) % 128, L) for o, L in zip(self.doff[:-1], self.lens)}
        miss16 = [(r, L) for L in full for r in range(16) if (r, L) not in seen16]
        miss128 = [(r, L) for L in lc for r in range(128) if (r, L) not in seen128]
        assert not miss16 and not miss128, ("packed row grid incomplete", miss16[:5], miss128[:5])
        assert {ROW * R + t for R in FULL_R if R for t in FULL_T} <= set(full) and min(full) == 257 and len(FULL_T) == 15
        assert {ROW, ROW + 1, ROW + 256, ROW + 257, 2 * ROW + 1023, 4 * ROW, 5 * ROW + 17, 1023, 9 * ROW + 257} == set(lc)
        assert all(L < 128 or L in full or L in lc for L in self.lens), "a filler is an ordinary message of 0 .. 127 bytes"
        assert self.n == len(self.lens) == len(self.aads) and int(self.doff[0]) == PG.GUARD and int(self.doff[-1]) == PG.GUARD + sum(self.lens)
        assert len(AAD_CYCLE) == 13 and set(self.aads) == set(AAD_CYCLE)
        assert all(v == set(range(16)) for v in _aad_cells(self.aads, self.aoff[:-1]).values()), "AADs of 64 and of 65 blocks at every residue"
        assert self.n <= 6000 and self.size <= 12 << 20, (self.n, self.size)

    def cell(self, i):
        return dict(pkt=i, in_res=int(self.doff[i]) % 16, in_res128=int(self.doff[i]) % 128, length=self.lens[i], aad=self.aads[i], aad_res=int(self.aoff[i]) % 16,
                    **geometry(self.lens[i], self.aads[i]))


class Scattered(PG.Scattered):
    """messages wherever they live, laid out by pkt_grid.Scattered's rules: every (input residue, output residue) pair for SC_LENGTHS, or in place every residue for
    every length of `full_lengths`; the AADs at cycling residues behind guards"""
    AADS = AAD_CYCLE

    def __init__(self, inplace=False):
        super().__init__(0, inplace)

    def lengths(self):
        return full_lengths() if self.inplace else list(SC_LENGTHS)

    def check(self):
        super().check()
        assert all(v == set(range(16)) for v in _aad_cells(self.aads, self.pos_aad).values()), "AADs of 64 and of 65 blocks at every residue"
        assert self.n == (16 if self.inplace else 256) * len(self.lengths()) and self.size_in <= 12 << 20

    def cell(self, i):
        return dict(super().cell(i), **geometry(self.lens[i], self.aads[i]))


# ---------------------------------------------------------------------------------------------- the route grid
class Route:
    """Byte-packed messages around the mark of a routed call.  A message is SHORT (the packet kernels') when data + AAD < mark (csrc/aesgcm_rows.h rows_route_size,
    rows_is_small), else LONG (by rows).  Messages that have bytes alternate strictly short, long, short, ...: every boundary of the buffer lies between the two
    kernels.  The sizes mark - 1 (short), mark and mark + 1 (long) each occur with the boundary in front of them ("s": at the message's start) and behind them ("e": at
    its end) at every residue of that boundary mod 16 -- the data lengths follow from the AAD lengths chosen: data = size - AAD --, fillers of either kind steer.
    Messages of no bytes (they take no place: their neighbours still meet) and of a quarter of the mark sit in between."""

    def __init__(self, mark):
        assert mark % 64 == 0 and mark >= 1024
        self.mark, self.G = mark, 0
        A = [a for a in AAD_CYCLE if a <= mark - 1 - 16 * SMALL_TAIL - 1]               # (the data keeps a long tail at least: 17 blocks or more)
        sizes = ((mark - 1,), (mark, mark + 1))
        need = {(s, r, side) for s in (mark - 1, mark, mark + 1) for r in range(16) for side in "se"}
        lens, aads = [], []
        pos = k = 0                                                            # k: messages with bytes so far; message k is short when k is even

        def put(L, a):
            nonlocal pos, k
            lens.append(L); aads.append(a)
            pos += L
            k += 1 if L else 0

        def best(kind, r, k):
            b = None
            for s in sizes[kind]:
                for j in range(len(A)):
                    a = A[(k + j) % len(A)]
                    gain = ((s, r, "s") in need) + ((s, (r + s - a) % 16, "e") in need)
                    if gain > (b[0] if b else 0):
                        b = (gain, s, a)
            return b

        put(37, 13)                                                            # in front of everything: a short filler, so that the first cell has a neighbour
        while need:
            kind, r = k % 2, pos % 16
            assert len(lens) < 4000, "the route grid does not close"
            if kind == 0 and k % 8 == 4:
                put(mark // 4 - A[k % 5], A[k % 5])                             # a quarter of the mark
                continue
            b = best(kind, r, k)
            if b:
                _gain, s, a = b
                need.discard((s, r, "s")); need.discard((s, (r + s - a) % 16, "e"))
                put(s - a, a)
                if kind == 0 and k % 8 == 1:
                    put(0, (0, 1, 13)[k % 3])                                   # no bytes: short whatever its AAD, and the long message behind still meets the short one in front
                continue
            a = A[k % 5]                                                        # a filler of this kind that steers: the next message (of the other kind) starts where it is needed
            base = 17 if kind == 0 else mark + 64
            f = next((f for f in range(16) if best(1 - kind, (r + base + f) % 16, k + 1)), 1 + k % 5)
            put(base + f, a)
        put(41 if k % 2 == 0 else mark + 75, 1)                                 # ... and behind everything
        self.n, self.lens, self.aads = len(lens), lens, aads
        self.doff = np.concatenate(([PG.GUARD], PG.GUARD + np.cumsum(lens))).astype(np.uint64)
        self.aoff = np.concatenate(([PG.GUARD], PG.GUARD + np.cumsum(aads))).astype(np.uint64)
        self.size, self.aad_size = int(self.doff[-1]) + PG.GUARD, int(self.aoff[-1]) + PG.GUARD
        self.check()

    def short(self, i):
        return self.lens[i] + self.aads[i] < self.mark

    @property
    def n_small(self):
        return sum(1 for i in range(self.n) if self.short(i))

    def boundary_cells(self):
        """from the finished arrays alone: the (boundary residue, short-then-long) cells, and (size, boundary residue, side) for the three sizes around the mark"""
        m = self.mark
        live = [i for i in range(self.n) if self.lens[i]]
        cells, sized = set(), set()
        for p, q in zip(live, live[1:]):
            if self.short(p) == self.short(q):
                continue
            assert int(self.doff[p + 1]) == int(self.doff[q]), "only messages of no bytes lie between two neighbours"
            res = int(self.doff[q]) % 16
            cells.add((res, self.short(p)))
            if self.lens[p] + self.aads[p] in (m - 1, m, m + 1):
                sized.add((self.lens[p] + self.aads[p], res, "e"))
            if self.lens[q] + self.aads[q] in (m - 1, m, m + 1):
                sized.add((self.lens[q] + self.aads[q], res, "s"))
        return cells, sized

    def check(self):
        m = self.mark
        cells, sized = self.boundary_cells()
        assert cells == {(r, o) for r in range(16) for o in (False, True)}, ("route grid: boundary cells missing", len(cells))
        want = {(s, r, side) for s in (m - 1, m, m + 1) for r in range(16) for side in "se"}
        assert want <= sized, ("route grid: sizes around the mark missing", sorted(want - sized)[:5])
        live = [i for i in range(self.n) if self.lens[i]]
        assert all(self.short(p) != self.short(q) for p, q in zip(live, live[1:])), "short and long alternate"
        for s in (m - 1, m, m + 1):
            assert {int(self.doff[i]) % 16 for i in range(self.n) if self.lens[i] + self.aads[i] == s} == set(range(16)), ("data starts of size", s)
        assert sum(1 for L in self.lens if L == 0) >= 3 and sum(1 for L, a in zip(self.lens, self.aads) if L and L + a == m // 4) >= 3
        assert 0 < self.n_small < self.n <= 4000

    def cell(self, i):
        return dict(pkt=i, in_res=int(self.doff[i]) % 16, in_res128=int(self.doff[i]) % 128, length=self.lens[i], aad=self.aads[i], aad_res=int(self.aoff[i]) % 16,
                    size=self.lens[i] + self.aads[i], by="packets" if self.short(i) else "rows", **geometry(self.lens[i], self.aads[i]))


class RouteScattered(PG.Scattered):
    """the route grid's messages wherever they live: the same lengths in the same order, every input at its packed residue, the output 5 residues on (in place: the
    same), 1 .. 19 guard bytes between neighbours -- a store of either kernel that spills over its message's end meets a canary"""

    def __init__(self, mark, inplace=False):
        self.route = Route(mark)
        self.mark = mark
        super().__init__(0, inplace)

    def order(self):
        r = self.route
        return [(int(r.doff[i]) % 16, (int(r.doff[i]) + (0 if self.inplace else 5)) % 16, r.lens[i]) for i in range(r.n)]

    def lay(self, order, aads=None):
        super().lay(order, self.route.aads)

    def check(self):
        r = self.route
        assert self.lens == r.lens and self.aads == r.aads and [p % 16 for p in self.pos_in] == [int(o) % 16 for o in r.doff[:-1]]
        assert all((q - p) % 16 == (0 if self.inplace else 5) for p, q in zip(self.pos_in, self.pos_out))
        for pos, ln in ((self.pos_in, self.lens), (self.pos_out, self.lens), (self.pos_aad, self.aads)):
            gaps = [pos[i + 1] - (pos[i] + ln[i]) for i in range(self.n - 1)]
            assert pos[0] >= PG.GUARD and min(gaps) >= 1 and max(gaps) <= 19, (min(gaps), max(gaps))

    n_small = property(lambda self: self.route.n_small)

    def cell(self, i):
        return dict(super().cell(i), size=self.lens[i] + self.aads[i], by="packets" if self.route.short(i) else "rows", **geometry(self.lens[i], self.aads[i]))
