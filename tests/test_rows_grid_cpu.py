"""CPU: the row-scale alignment grid's generator (tests/rows_grid.py) -- every grid the GPU tests run (tests/test_gpu_rows_grid.py) is complete (the generators assert
every required cell themselves) and deterministic, its constants are the row code's, and the reference arenas the GPU is held to are self-consistent: what the
project's oracle made of them is what libcrypto makes of them."""
import os
import re

import numpy as np

import pkt_grid as PG
import rows_grid as RG
from grid_legs import _assemble, _reference_of
from kt_common import CSRC, evp  # noqa: F401  (the libcrypto handle: a fixture)

MARK = 2048


def _layout(g):
    if hasattr(g, "doff"):
        return g.lens, g.aads, g.doff.tobytes(), g.aoff.tobytes(), g.size, g.aad_size
    return g.lens, g.aads, g.pos_in, g.pos_out, g.pos_aad, g.size_in, g.size_out, g.size_aad


def test_the_constants_are_the_row_codes():
    h = open(os.path.join(CSRC, "aesgcm_rows.h")).read()
    assert int(re.search(r"#define ROWS_SMALL_TAIL (\d+)u", h).group(1)) == RG.SMALL_TAIL and int(re.search(r"#define ROWS_SMALL_AAD (\d+)u", h).group(1)) == RG.SMALL_AAD
    assert "g.R = (u32)(len >> 10)" in h and RG.ROW == 1 << 10
    assert "HD bool rows_is_small(u64 len, u64 alen, u32 route_min) { return rows_route_size(len, alen) < route_min; }" in h      # what rows_grid.Route.short restates


def test_every_grid_is_complete_and_deterministic():
    makes = (RG.Packed, RG.Scattered, lambda: RG.Scattered(True), lambda: RG.Route(MARK), lambda: RG.RouteScattered(MARK), lambda: RG.RouteScattered(MARK, True))
    for make in makes:
        a, b = make(), make()                                    # (construction runs the completeness assertions)
        assert _layout(a) == _layout(b)
    p = RG.Packed()
    full, lc = RG.full_lengths(), RG.lc_lengths()
    assert len(full) == 98 and 8 <= len(lc) <= 12 and p.n >= 16 * len(full) + 128 * len(lc) - 16 * len(set(full) & set(lc)) and p.n < 4000 and p.size < 11 << 20
    assert {(int(o) % 128, L) for o, L in zip(p.doff[:-1], p.lens)} >= {(r, L) for r in range(128) for L in lc}
    assert {(int(o) % 16, L) for o, L in zip(p.doff[:-1], p.lens)} >= {(r, L) for r in range(16) for L in full}
    # what the grid is for: runs of 1, 2, 3, 4, 5 and 9 rows, tails either side of ROWS_SMALL_TAIL behind whole rows, AADs either side of ROWS_SMALL_AAD
    geo = [RG.geometry(L, a) for L, a in zip(p.lens, p.aads)]
    assert {g["R"] for g in geo} >= {0, 1, 2, 3, 4, 5, 9}
    assert {(g["R"] > 0, g["tail_blocks"]) for g in geo} >= {(True, t) for t in (0, 1, 2, 16, 17, 32, 63, 64)} | {(False, 17), (False, 64)}
    assert {g["aad_blocks"] for g in geo} >= {0, 1, 2, 63, 64, 65, 129}
    s, si = RG.Scattered(), RG.Scattered(True)
    assert s.n == 256 * len(RG.SC_LENGTHS) and si.n == 16 * len(full) and si.pos_out is si.pos_in
    assert {(a % 16, b % 16, L) for a, b, L in zip(s.pos_in, s.pos_out, s.lens)} == {(a, b, L) for a in range(16) for b in range(16) for L in RG.SC_LENGTHS}


def test_the_route_grid_has_every_boundary_cell_and_the_sizes_around_the_mark():
    r = RG.Route(MARK)
    cells, sized = r.boundary_cells()
    assert len(cells) == 32 and cells == {(res, first_short) for res in range(16) for first_short in (False, True)}
    assert {(s, res, side) for s in (MARK - 1, MARK, MARK + 1) for res in range(16) for side in "se"} <= sized
    sizes = [l + a for l, a in zip(r.lens, r.aads)]
    assert r.n_small == sum(1 for s in sizes if s < MARK) and 0 < r.n_small < r.n
    assert all(r.short(i) == (sizes[i] <= MARK - 1) for i in range(r.n)) and not r.short(sizes.index(MARK)) and r.short(sizes.index(MARK - 1))
    assert 0 in r.lens and MARK // 4 in sizes
    for sc in (RG.RouteScattered(MARK), RG.RouteScattered(MARK, True)):
        assert sc.lens == r.lens and sc.aads == r.aads and sc.n_small == r.n_small
    assert RG.Route(4096).mark == 4096                            # (the rules close at another mark too)


def _evp(evp, key, ivs, aad, aoff, data, doff):
    n = len(doff) - 1
    out, tags = np.empty(max(len(data), 1), dtype=np.uint8), np.empty(16 * n, dtype=np.uint8)
    a, d = np.frombuffer(aad, dtype=np.uint8), np.frombuffer(data, dtype=np.uint8)
    ao, do = np.asarray(aoff, dtype=np.uint64), np.asarray(doff, dtype=np.uint64)
    assert evp.evp_frames_crypt(n, len(key), key, ivs, a.ctypes.data, ao.ctypes.data, 0, d.ctypes.data, do.ctypes.data, 0, out.ctypes.data, tags.ctypes.data) == 0
    return out[:len(data)].tobytes(), tags.tobytes()


def test_the_reference_arenas_open_under_libcrypto(orc, evp):  # noqa: F811
    """AES-256: libcrypto (oracle/evp_batch.c, one-shot GCM per message: encrypt only) seals every message of the packed grids to the oracle's ciphertext and tag -- so
    a receiver that verifies accepts every tag and refuses every forged one --, and its keystream over the oracle's ciphertext arena gives the plaintext arena back"""
    for kind, make in (("packed", RG.Packed), ("route", lambda: RG.Route(MARK))):
        R = _reference_of(orc, ("rows_grid_cpu", kind), make, 32, 0x7095DC00 + len(kind))
        g = R.grid
        doff, aoff = [int(x) for x in g.doff], [int(x) for x in g.aoff]
        ct, tags = _evp(evp, R.keys[0], R.ivs, R.aad_arena.tobytes(), aoff, R.pt_arena.tobytes(), doff)
        ct_arena = _assemble(R, R.pt_arena, R.in_at, "ct")
        x = PG.first_difference(ct[doff[0]:doff[-1]], ct_arena.tobytes()[doff[0]:doff[-1]])              # (libcrypto writes the messages' bytes only: the guards are not its)
        assert x is None, ("ciphertext", g.cell(PG.owner(R.in_at, R.lens, x + doff[0])[0]))
        assert tags == R.tags, ("tag", next(g.cell(i) for i in range(R.n) if tags[16 * i:16 * i + 16] != R.tags[16 * i:16 * i + 16]))
        refused = [i for i in range(R.n) if R.bad_tags[16 * i:16 * i + 16] != tags[16 * i:16 * i + 16]]
        assert refused == R.forged == PG.forged(R.n) and 0 in refused and R.n - 1 in refused
        back, _t = _evp(evp, R.keys[0], R.ivs, R.aad_arena.tobytes(), aoff, ct_arena.tobytes(), doff)      # CTR is its own inverse: the data path of a decrypt
        for i in range(R.n):
            assert back[doff[i]:doff[i + 1]] == R.pt_arena[doff[i]:doff[i + 1]].tobytes(), ("plaintext", g.cell(i))
        assert ct_arena[:PG.GUARD].tolist() == [PG.CANARY_IN] * PG.GUARD and ct_arena[doff[-1]:].tolist() == [PG.CANARY_IN] * PG.GUARD
