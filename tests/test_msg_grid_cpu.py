"""CPU: the grid of single messages (tests/msg_grid.py) without a device -- its own coverage assertions with the fake device's geometry, every cell's planned
launches on the fake runtime (tests/fake_hip/msg_grid_drive.py: a forced shape is the shape taken), and the comparison's reports on synthetic arenas."""
import os
import subprocess
import sys

import numpy as np
import pytest

import grid_legs as GL
import msg_grid as MG
import pkt_grid as PG

HERE = os.path.dirname(os.path.abspath(__file__))
U = MG.FAKE_UNITS


def test_every_shape_has_its_cells():
    """Grid.check ran in the constructor: every (rows, tail blocks, tail bytes) of the shape, the sub-row lengths, the message above one turn of the strands, the
    AAD residues and lengths, no two guarded spans overlapping.  Here: the cells by name, and the sizes"""
    cover = set()
    for s in MG.SHAPES:
        g = MG.grid(s.name, U)
        cover.update(g.coverage())
        assert len(g.coverage()) == len(set(g.coverage())) == g.n, "a cell twice"
        lim = 56 << 20 if s.kind == "main_dealt" else 8 << 20
        assert g.size_in <= lim and g.size_aad <= 5 << 20, (s.name, g.size_in, g.size_aad)
        for i in range(g.n):                                   # guards as laid out: 256 canary bytes or more either side of every message
            end = g.pos_in[i] + g.lens[i]
            assert g.pos_in[i] - (g.pos_in[i - 1] + g.lens[i - 1] if i else 0) >= PG.GUARD and (g.pos_in[i + 1] if i + 1 < g.n else g.size_in) - end >= PG.GUARD
    names = {c[0] for c in cover}
    assert names == {s.name for s in MG.SHAPES} and len(names) == 9
    for s in MG.SHAPES:
        if s.kind != "main_dealt":
            for r in s.rows(U):
                assert {(tb, by) for (n, rr, tb, by, _res, _a) in cover if n == s.name and rr == r} >= {(tb, by) for tb in MG.TAIL_BLOCKS for by in MG.TAIL_BYTES}, (s.name, r)
        assert {res for (n, _r, _t, _b, res, _a) in cover if n == s.name} >= set(range(8)), s.name
        assert {a for (n, _r, _t, _b, _res, a) in cover if n == s.name} >= set(MG.AAD_CYCLE), s.name
    # the rows of the table: tw 1 and 3 for the dealt body, both closings of the fold and of the cyclic rows, the half shape
    assert MG.SHAPE["body_tw1"].rows(U) == (4, 5, 7, 8, 9) and MG.SHAPE["body_tw3"].rows(U) == (12, 13, 23, 24, 25)
    assert MG.SHAPE["main_dealt"].rows(U) == (6144, 6145) and MG.SHAPE["cyc_half"].waves(U) == 2048 and MG.SHAPE["cyc_close0"].waves(U) == 4096
    assert {dict(s.opts).get("fold_close") for s in MG.SHAPES if s.kind == "fold"} == {0, 1}
    assert {dict(s.opts).get("cyc_close") for s in MG.SHAPES if s.kind == "cyc"} == {0, 1}


def test_shards_sessions_and_keystream_runs():
    for ranks in (3, 5):
        rng = MG.shard_ranges(ranks, U)
        assert sum(ln for _f, ln in rng) == MG.SHARD_LEN and all(f % 256 for f, _ln in rng[1:]) and rng[-1][1] % 16 == 9
        assert all(f * 16 == sum(ln for _f, ln in rng[:r]) for r, (f, _ln) in enumerate(rng))
    s = MG.stream_sessions(U)
    assert [len(x) for x in s] == [1, 2, 4]
    flat = {c for x in s for c in x}
    assert {1024 - 16, 4096, 4096 + 16} <= flat and any(c % 1024 == 0 and c > 4096 for c in flat)
    assert [nb for nb in MG.KS_NBLOCKS if MG.ks_fits(MG.KS_FIRST[-1], nb)] == [1] and all(MG.ks_fits(f, nb) for f in MG.KS_FIRST[:-1] for nb in MG.KS_NBLOCKS)
    sl = MG.Slots([16 * nb for nb in MG.KS_NBLOCKS])
    a = sl.arena(PG.CANARY_OUT, {0: b"\x01" * 16})
    assert a[sl.in_at[0] - 1] == PG.CANARY_OUT and a[sl.in_at[0]] == 1 and a[sl.in_at[0] + 16] == PG.CANARY_OUT


def test_planned_launches_of_every_cell_on_the_fake_runtime():
    """tests/fake_hip/msg_grid_drive.py in a child process over libaesgcm_fake.so: every (shape, length) cell through encrypt_dev and decrypt_dev, the shards and
    the sessions -- the launch log holds the kernels the shape's row of the table names, last_launch and split answer what the GPU legs assert"""
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc (the HIP headers)")
    d = os.path.join(HERE, "fake_hip")
    subprocess.run(["make", "-C", d, "-s", "libaesgcm_fake.so"], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    env = dict(os.environ, AESGCM_LIB=os.path.join(d, "libaesgcm_fake.so"))
    out = subprocess.run([sys.executable, os.path.join(d, "msg_grid_drive.py")], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
    assert out.returncode == 0 and "MSG GRID PLAN OK (" in out.stdout, out.stdout[-3000:]
    lines = {ln.split()[0]: ln for ln in out.stdout.splitlines()}
    assert set(lines) >= {s.name for s in MG.SHAPES}, out.stdout
    assert "'k_fold'" in lines["fold_close1"] and "'k_fold'" not in lines["fold_close0"] and "'k_body'" in lines["cyc_half"]


class _Synthetic:
    """a reference as grid_legs._reference_of makes it, without an oracle: the `ciphertext` is the plaintext with every bit turned"""

    def __init__(self, name):
        self.grid = g = MG.grid(name, U)
        self.n, self.lens, self.aads = g.n, g.lens, g.aads
        self.in_at, self.out_at, self.aad_at = g.pos_in, g.pos_out, g.pos_aad
        self.pt_arena = GL._arena(g.size_in, PG.CANARY_IN, 7, g.pos_in, g.lens)
        self.ct = [self.pt_arena[p:p + l] ^ 0xFF for p, l in zip(g.pos_in, g.lens)]
        self.tags = bytes(range(256)) * (g.n // 16 + 1)
        self.tags = self.tags[:16 * g.n]
        self.forged = PG.forged(g.n)
        self.cell_extra = lambda j: g.cell(j)


@pytest.mark.parametrize("name", ["main_static", "body_tw3"])
def test_the_comparison_reports_perturbed_references(name):
    """one byte inside a message, the first guard byte behind it, the last guard byte in front of it, one bit of a tag: each raises and names the arena byte, the
    message, the side and the cell; the unperturbed arena passes; a wipe of one byte too many or too few is a difference"""
    R = _Synthetic(name)
    S = MG.SHIFT
    want = GL._assemble(R, GL._canary(R.grid.size_out, S), R.out_at, "ct", shift=S)
    got = want.tobytes()
    MG.same(R, got, want, R.out_at, S, "as it is")
    MG.tags_same(R, R.tags, "as they are")
    for i in (1, 37, R.n - 2):
        for what, arena, tags, words in MG.perturbations(R, want, R.out_at, S, i):
            with pytest.raises(AssertionError) as e:
                if arena is not None:
                    MG.same(R, got, arena, R.out_at, S, what)
                else:
                    MG.tags_same(R, R.tags, what, tags=tags)
            assert all(w in str(e.value) for w in words), (what, words, str(e.value))
    wiped = GL._assemble(R, GL._canary(R.grid.size_out, S), R.out_at, "pt", shift=S, wiped=True)
    i = next(i for i in R.forged if R.lens[i] > 1)
    for x, word in ((R.out_at[i] + S + R.lens[i], " 1 bytes behind packet %d " % i), (R.out_at[i] + S + R.lens[i] - 1, "byte %d of packet %d;" % (R.lens[i] - 1, i))):
        a = np.array(wiped)
        a[x] = 0 if a[x] else PG.CANARY_OUT                    # a wipe that went a byte too far; one that stopped a byte short
        with pytest.raises(AssertionError) as e:
            MG.same(R, a.tobytes(), wiped, R.out_at, S, "wipe")
        assert word in str(e.value), str(e.value)
