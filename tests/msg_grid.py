"""The alignment grid of SINGLE MESSAGES on device pointers (aesgcm_encrypt_dev / aesgcm_decrypt_dev, aesgcm_shard_crypt_dev, aesgcm_stream_update_dev,
aesgcm_keystream_dev): one deterministic generator for the GPU tests (tests/test_gpu_msg_grid.py), for the CPU check of the generator and of the comparison
(tests/test_msg_grid_cpu.py) and for the walk of every cell over the fake runtime (tests/fake_hip/msg_grid_drive.py), which proves that a forced shape is taken.

What these calls can get wrong is a store or a load at the END of a range: the last block's bytes (store_block_bytes, load_block_bytes), the partial last row of a
launch, the seam between k_body and the k_main tail behind it, a wipe of another length than `len`.  So every message lies between canary bytes -- at least
PG.GUARD of them either side, CANARY_IN around inputs and AADs, CANARY_OUT around outputs, both non-zero and different: an over-read changes a tag, an over-write
changes the arena -- and every arena is compared WHOLE (grid_legs._same names the byte, the message, the side and the cell).

  shapes    SHAPES: each launch structure of the planner (csrc/aesgcm_msgplan.h) forced by context options; what a message of a shape must launch is `expected`
  lengths   rows x blocks behind the last whole row x tail bytes, in the planner's own units (units(): B a block, R a row of 64 blocks, A the 256-block alignment of
            the body, the waves of a k_main launch and of the cyclic launch and of its half shape -- read from the library, not written here)
  AAD       an arena of its own: starts at all 16 residues, 1 .. 19 canary bytes between neighbours, lengths 0 1 15 16 17 20 33 in a cycle of 7 (coprime to the
            residues' 16) and once per shape more than the front rows of the cyclic launch hold (the fallback of test_aad_longer_than_the_front_rows_falls_back)

Every generator asserts that every required cell occurred and that no two guarded spans overlap: a grid that lost a part fails."""
import numpy as np

import grid_legs as GL
import pkt_grid as PG

LAUNCH_MAIN, LAUNCH_CYCLIC, LAUNCH_CYCLIC_HALF, LAUNCH_DEALT = 1, 2, 3, 4          # aesgcm_ctx_last_launch (lib.py; the CPU tests assert they are the binding's)
SHIFT = 48                        # out-of-place outputs lie this many bytes further into their arena than the inputs into theirs: another place in the 128-byte line
TAIL_BLOCKS = (0, 1, 2, 62, 63)
TAIL_BYTES = (0, 1, 8, 15)
AAD_CYCLE = (0, 1, 15, 16, 17, 20, 33)
NOCYC = (("cyc_min", 0), ("cyc_max", 0))
CYC = (("cyc_min", 4096), ("cyc_max", 1 << 50))
BODY = (("body_min", 4096),) + NOCYC
KEY_SIZES = (16, 24, 32)

# what the fake device of tests/fake_hip answers (256 CUs); tests/fake_hip/msg_grid_drive.py asserts that it does
FAKE_UNITS = dict(B=16, R=64, A=256, main_waves=6144, W=4096, W_half=2048)


def units(lib, key=bytes(16)):
    """the planner's units from the library in force: B bytes of a block, R blocks of a row (the least range the cyclic rows take with cyc_min = 1 is one row),
    A blocks of the body's alignment (the head in front of a range from block 1), the waves of a full k_main launch and of the cyclic launch and its half shape"""
    with lib.Context(key) as c:
        g, b = c.geometry(), c.geometry(body=True)
        c.set_option("cyc_min", 1).set_option("cyc_max", 1 << 50)
        B = 16
        R = next(k for k in range(1, 1025) if c.split(B * k)[1])
        assert c.split(B * R) == (0, R)
        A = c.split(B * 8 * R * 8, 1)[0] + 1
    W = b["workgroups"] * b["wg_lanes"] // 64
    return dict(B=B, R=R, A=A, main_waves=g["workgroups"] * g["wg_lanes"] // 64, W=W, W_half=W // 2)


class Shape:
    """one row of the table of shapes: the context options that force it, what aesgcm_ctx_last_launch must answer, its kind (what `expected` keys on), the chunk
    width it forces and its row counts"""

    def __init__(self, name, kind, opts, launch, tw=1):
        self.name, self.kind, self.opts, self.launch, self.tw = name, kind, tuple(opts), launch, tw

    def opt(self, k, default):
        return dict(self.opts).get(k, default)

    def rows(self, u):
        """the shape's minimum and minimum + 1; 2 tw - 1, 2 tw, 2 tw + 1 where the shape takes so few rows -- k_body takes 4 tw rows at least, there the second
        super-chunk's edge (8 tw - 1, 8 tw, 8 tw + 1) stands for them; k_main's static waves take every count from 0, and 62 (64 chunk items with the ragged row and an AAD)"""
        tw = self.tw
        if self.kind == "main":
            return (0, 1, 2, 3, 62)
        if self.kind == "main_dealt":
            return (u["main_waves"], u["main_waves"] + 1)
        if self.kind == "fold":
            return (68, 69, 71, 72, 73)                      # 4 S chunk items, S = rows / 4: 68 > COMBINE_MAX_ITEMS = 64
        return (4 * tw, 4 * tw + 1, 8 * tw - 1, 8 * tw, 8 * tw + 1)

    def tails(self, rows, u):
        """(blocks behind the last whole row, tail bytes): the full cross, but for the messages of k_main's dealt chunks -- 6 MiB each: the edges once each at the
        minimum, the two ends at minimum + 1"""
        if self.kind != "main_dealt":
            return [(tb, by) for tb in TAIL_BLOCKS for by in TAIL_BYTES]
        return [(0, 0), (1, 1), (2, 8), (62, 15), (63, 0)] if rows == u["main_waves"] else [(0, 1), (63, 15)]

    def waves(self, u):
        return u["W_half"] if self.kind == "half" else u["W"]


SHAPES = (
    Shape("main_static", "main", (), LAUNCH_MAIN),
    Shape("main_dealt", "main_dealt", NOCYC + (("tw", 1),), LAUNCH_MAIN),
    Shape("body_tw1", "body", BODY + (("tw", 1),), LAUNCH_DEALT),
    Shape("body_tw3", "body", BODY + (("tw", 3),), LAUNCH_DEALT, tw=3),
    Shape("fold_close1", "fold", BODY + (("tw", 1), ("fold_close", 1)), LAUNCH_DEALT),
    Shape("fold_close0", "fold", BODY + (("tw", 1), ("fold_close", 0)), LAUNCH_DEALT),
    Shape("cyc_close1", "cyc", CYC + (("cyc_close", 1), ("cyc_half", 0)), LAUNCH_CYCLIC),
    Shape("cyc_close0", "cyc", CYC + (("cyc_close", 0), ("cyc_half", 0)), LAUNCH_CYCLIC),
    Shape("cyc_half", "half", CYC + (("cyc_close", 1), ("cyc_half", 1)), LAUNCH_CYCLIC_HALF),
)
SHAPE = {s.name: s for s in SHAPES}


def expected(shape, length, aad, u):
    """what a whole message of this shape must launch, from the planner's rules restated: dict(launch = aesgcm_ctx_last_launch, split = aesgcm_ctx_split or None
    where the AAD decides, body / cyc / half / main_dealt = which kernel takes the rows, tail = a k_main launch behind k_body, last = the launch that closes the tag)"""
    Rb = u["B"] * u["R"]
    rows = length // Rb
    e = dict(launch=shape.launch, split=(0, 0), body=False, cyc=False, half=False, main_dealt=False, tail=False, fold=False, last="k_combine")
    if shape.kind in ("cyc", "half"):
        front = ((aad + 15) // 16 + u["R"] - 1) // u["R"]
        if front > shape.waves(u):                           # more front rows than strands: the other path (body_min is the library's own: k_main)
            return dict(e, launch=LAUNCH_MAIN, split=None, last=None)
        e.update(cyc=True, body=True, half=shape.kind == "half", split=(0, rows * u["R"]))
        if shape.opt("cyc_close", 1):
            e["last"] = "k_body"
        else:
            e["fold"] = True
        return e
    if shape.kind in ("body", "fold"):
        S = rows // (4 * shape.tw)
        body = S * 4 * shape.tw
        whole = not aad and length == body * Rb
        e.update(body=True, split=(0, body * u["R"]), tail=length > body * Rb, fold=True)
        if whole and shape.opt("fold_close", 1):
            e["last"] = "k_fold"
        return e
    e["main_dealt"] = shape.kind == "main_dealt"
    e["last"] = None                                          # one chunk: k_main's tail; more: k_combine (k_fold between where the items are many)
    return e


class Grid:
    """the messages of one shape: pos_in / pos_out (the same offsets: both arenas are laid out alike, the out-of-place legs write SHIFT bytes further in) on 16-byte
    boundaries with at least PG.GUARD canary bytes between neighbours and at both ends; pos_aad in an arena of its own"""

    def __init__(self, shape, u):
        self.shape, self.u = shape, u
        Rb = u["B"] * u["R"]
        cells = [(r, tb, by) for r in shape.rows(u) for (tb, by) in shape.tails(r, u)]
        aads = [AAD_CYCLE[i % len(AAD_CYCLE)] for i in range(len(cells))]
        self.big_aad = shape.waves(u) * Rb + 4 * Rb + 9
        cells.append((shape.rows(u)[0], 1, 1)); aads.append(self.big_aad)
        if shape.kind in ("cyc", "half"):                    # a strand takes a second row while the partial last row exists
            cells.append((shape.waves(u) + 1, 63, 15)); aads.append(20)
        if shape.kind in ("body", "fold"):                   # the whole range one aligned body, no AAD: k_body's items go straight to the tag
            cells.append((shape.rows(u)[0], 0, 0)); aads.append(0)
            cells.append((shape.rows(u)[3], 0, 0)); aads.append(0)
        self.n, self.cells, self.aads = len(cells), cells, aads
        self.lens = [r * Rb + tb * u["B"] + by for (r, tb, by) in cells]
        self.pos_in, self.pos_aad = [], []
        a, c = 0, PG.GUARD - 1
        for i, L in enumerate(self.lens):
            a = (a + PG.GUARD + 16 * (i % 3) + 15) // 16 * 16                      # 256 .. 303 canary bytes in front, the start on a 16-byte boundary
            self.pos_in.append(a); a += L
            c = PG._place(c, i % 16, i); self.pos_aad.append(c); c += aads[i]
        self.pos_out = self.pos_in
        self.size_in = self.size_out = a + PG.GUARD
        self.size_aad = c + 1 + PG.GUARD
        self.check()

    def check(self):
        u, s = self.u, self.shape
        Rb = u["B"] * u["R"]
        assert PG.CANARY_IN and PG.CANARY_OUT and PG.CANARY_IN != PG.CANARY_OUT
        assert all(p % 16 == 0 for p in self.pos_in) and self.pos_in[0] >= PG.GUARD
        for pos, ln, g, size in ((self.pos_in, self.lens, PG.GUARD, self.size_in), (self.pos_aad, self.aads, 1, self.size_aad)):
            spans = [(p - g, p + l + g) for p, l in zip(pos, ln)]                   # a message with its guard either side
            assert all(pos[i] + ln[i] + g <= pos[i + 1] for i in range(self.n - 1)), "two guarded spans overlap"
            assert spans[0][0] >= 0 and spans[-1][1] <= size and pos[0] >= PG.GUARD and size - (pos[-1] + ln[-1]) >= PG.GUARD
        seen = set(self.cells[:self.n])
        for r in s.rows(u):
            want = set(s.tails(r, u))
            assert {(r, tb, by) for (tb, by) in want} <= seen, ("cells missing", s.name, r)
            assert s.kind == "main_dealt" or want == {(tb, by) for tb in TAIL_BLOCKS for by in TAIL_BYTES}
        assert {tb for (_r, tb, _b) in seen} >= set(TAIL_BLOCKS) and {by for (_r, _t, by) in seen} >= set(TAIL_BYTES)
        if s.kind == "main":
            assert {0, 1, 15, 16, 17, Rb - 1, Rb, Rb + 1} <= set(self.lens), "the sub-row lengths"
        if s.kind in ("cyc", "half"):
            assert (s.waves(u) + 1) * Rb + 63 * u["B"] + 15 in self.lens, "a message above one turn of the launch's strands"
        big = [L for L in self.lens if L > 136 << 10]
        assert len(big) == (1 if s.kind in ("cyc", "half") else self.n if s.kind == "main_dealt" else 0), (s.name, big)
        assert len({p % 16 for p in self.pos_aad}) == min(16, self.n), "AAD starts at every residue (k_main's dealt chunks: eight messages, eight residues)"
        assert set(self.aads) == set(AAD_CYCLE) | {self.big_aad} and self.aads.count(self.big_aad) == 1
        assert len({(p % 16, a) for p, a in zip(self.pos_aad, self.aads)}) >= min(self.n, 100), "residue and length walk with periods 16 and 7: no pair twice in 112"
        # every message takes what its shape's row of the table names
        ex = [expected(s, L, a, u) for L, a in zip(self.lens, self.aads)]
        if s.kind == "main":
            assert all(L < 64 << 10 for L in self.lens)
        if s.kind in ("body", "fold"):
            assert all(e["body"] for e in ex) and any(e["tail"] for e in ex) and any(not e["tail"] for e in ex)
            assert {e["last"] for e in ex} == ({"k_fold", "k_combine"} if s.opt("fold_close", 1) else {"k_combine"})
        if s.kind == "fold":
            assert all(4 * (L // Rb // 4) > 64 for L in self.lens), "more than 64 chunk items"
        if s.kind in ("cyc", "half"):
            assert [e["cyc"] for e in ex].count(False) == 1 and ex[self.aads.index(self.big_aad)]["launch"] == LAUNCH_MAIN

    def cell(self, i):
        r, tb, by = self.cells[i]
        return dict(msg=i, shape=self.shape.name, rows=r, tail_blocks=tb, tail_bytes=by, length=self.lens[i], aad=self.aads[i], aad_res=self.pos_aad[i] % 16)

    def coverage(self):
        """the (shape, rows, tail blocks, tail bytes, AAD residue, AAD length) cells that exist"""
        return [(self.shape.name, r, tb, by, self.pos_aad[i] % 16, self.aads[i]) for i, (r, tb, by) in enumerate(self.cells)]


_GRIDS = {}


def grid(name, u):
    k = (name, tuple(sorted(u.items())))
    if k not in _GRIDS:
        _GRIDS[k] = Grid(SHAPE[name], u)
    return _GRIDS[k]


# ---------------------------------------------------------------------------------------------- shards, streaming chunks, keystream runs
SHARD_LEN, SHARD_AAD = (40 << 10) + 9, 33
SHARD_FIRSTS = {3: (0, 860, 1707), 5: (0, 519, 1031, 1543, 2055)}                  # first blocks of the ranks: none but 0 a multiple of 256
SHARD_OPTS = {"dealt": BODY + (("tw", 1),), "cyclic": CYC}


def shard_ranges(ranks, u):
    """[(first block, bytes)] of the ranks; every rank's range keeps whole rows behind its head (asserted: the forced shapes must be taken)"""
    total = (SHARD_LEN + 15) // 16
    firsts = SHARD_FIRSTS[ranks] + (total,)
    out = []
    for r in range(ranks):
        f, e = firsts[r], firsts[r + 1]
        ln = (SHARD_LEN if e == total else 16 * e) - 16 * f
        head = (-f) % u["A"]
        assert (r == 0 or f % u["A"]) and (ln // 16 - head) // u["R"] >= 4, (ranks, r)
        out.append((f, ln))
    return out


def stream_sessions(u):
    """chunk sizes in bytes of the sessions of 1, 2 and 4 chunks: on and beside a row and the body's alignment, every chunk but the last whole blocks, the last ragged"""
    Rb, Ab = u["B"] * u["R"], u["B"] * u["A"]
    s = ((Rb + 16 + 5,), (Ab, Ab + Rb - 16 + 1), (Rb - 16, Ab + 16, 2 * Ab + Rb, Rb + 48 + 15))
    assert all(c % 16 == 0 for x in s for c in x[:-1]) and all(x[-1] % 16 for x in s)
    return s


STREAM_AAD = 20
STREAM_OPTS = {"main": (), "dealt": BODY + (("tw", 1),), "cyclic": CYC}
KS_NBLOCKS = (1, 2, 63, 64, 65, 255, 256, 257)
KS_FIRST = (0, 1, 255, (1 << 32) - 3)


def ks_fits(first, nblocks):
    """include/aesgcm.h: the counter must not wrap -- first_block + nblocks <= 2^32 - 2 (what lies above is refused with ETOOLONG and writes nothing)"""
    return first + nblocks <= (1 << 32) - 2


class Slots:
    """byte ranges of the given lengths in one arena, each on a 16-byte boundary between at least PG.GUARD canary bytes; the interface grid_legs._same reads"""

    def __init__(self, lens, names=None):
        self.n, self.lens, self.names = len(lens), list(lens), names or list(range(len(lens)))
        self.in_at, a = [], 0
        for i, L in enumerate(lens):
            a = (a + PG.GUARD + 16 * (i % 3) + 15) // 16 * 16
            self.in_at.append(a); a += L
        self.size = a + PG.GUARD
        self.aads, self.aad_at = [0] * self.n, [0] * self.n
        self.cell_extra = lambda j: dict(slot=self.names[j])
        assert all(self.in_at[i] + self.lens[i] + PG.GUARD <= self.in_at[i + 1] for i in range(self.n - 1))

    def arena(self, canary, parts=None):
        """canary everywhere; parts: {slot: bytes} put at the slots' places"""
        a = np.full(self.size, canary, dtype=np.uint8)
        for i, b in (parts or {}).items():
            a[self.in_at[i]:self.in_at[i] + len(b)] = np.frombuffer(bytes(b), dtype=np.uint8)
        return a


# ---------------------------------------------------------------------------------------------- references and the comparison
def reference(orc, name, klen, u):
    """the grid of a shape, its inputs and the oracle's ciphertexts and tags (grid_legs._reference_of: computed once per shape and key size, never written to)"""
    seed = 0x3E550000 + 4096 * [s.name for s in SHAPES].index(name) + 16 * klen
    R = GL._reference_of(orc, ("msg", name, klen, tuple(sorted(u.items()))), lambda: grid(name, u), klen, seed)
    R.cell_extra = lambda j: R.grid.cell(j)
    return R


class _Host:
    """bytes already downloaded, behind the interface grid_legs._same reads a device buffer through"""

    def __init__(self, b):
        self.b = b

    def download(self, n):
        assert n == len(self.b), (n, len(self.b))
        return self.b


def same(R, got, want, at, shift, label):
    """grid_legs._same over an arena that is on the host already: the whole arena; on a difference the byte, got and wanted, the message, how far behind or in
    front of it, and the cell"""
    GL._same(R, _Host(bytes(got)), want, at, shift, label)


def tags_same(R, got, label, tags=None):
    """every tag against the oracle's (tags: another expectation than R.tags)"""
    want = R.tags if tags is None else tags
    if got != want:
        i = next(i for i in range(R.n) if got[16 * i:16 * i + 16] != want[16 * i:16 * i + 16])
        raise AssertionError("%s: tag of message %d; cell %r" % (label, i, R.grid.cell(i)))


def perturbations(R, want, at, shift, i):
    """four wrong expectations around message i, each with what the report must say: [(what, arena or None, tags or None, words the message must hold)]"""
    L = R.lens[i]
    assert L >= 1
    out = []
    assert 0 < i < R.n - 1
    # (a guard byte is reported with the cell of the message it lies in front of; the message it lies behind is named with its length)
    for what, x, j, words in (("a byte inside the message", at[i] + shift + L // 2, i, ("byte %d of packet %d;" % (L // 2, i),)),
                              ("the first guard byte behind the message", at[i] + shift + L, i + 1, (" 1 bytes behind packet %d (length %d," % (i, L),)),
                              ("the last guard byte in front of the message", at[i] + shift - 1, i, ("guard byte 1 bytes in front of packet %d," % i,))):
        a = np.array(want, dtype=np.uint8)
        a[x] ^= 0x20
        out.append((what, a, None, words + ("arena byte %d is" % x, "'msg': %d," % j, "'rows': %d," % R.grid.cell(j)["rows"], "'shape': %r" % R.grid.cell(j)["shape"])))
    t = bytearray(R.tags)
    t[16 * i + 5] ^= 0x04
    out.append(("one bit of a tag", None, bytes(t), ("tag of message %d" % i, "'rows': %d" % R.grid.cell(i)["rows"])))
    return out
