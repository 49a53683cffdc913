"""GPU: the row kernels (k_rows / k_rows_close, csrc/aesgcm_rows.h) and routed calls on the alignment grid of tests/rows_grid.py -- every start residue at ROW scale.

tests/test_gpu_pkt_grid.py stops at 272 bytes at every start mod 128 and at the group edges of 64 lanes at every start mod 16: no run of three or more rows, no run cut
by a block boundary, no tail either side of ROWS_SMALL_TAIL behind a whole row and no AAD either side of ROWS_SMALL_AAD ever stood at a controlled residue.  Here they
do (the generator asserts every cell), through the legs of tests/grid_legs.py: arenas with 256 canary bytes in front and behind -- and 1 .. 19 between neighbours in
the scattered form --, compared WHOLE with arenas assembled from the CPU oracle (orc.Fast; never another GPU path), the input and AAD arenas after the calls too.  A
mismatch names the first differing message and its cell: residues mod 16 and mod 128, R, tail blocks, AAD blocks, rows_block.

1. by rows (the debug library's pkt_rows = 1; every call asserts its status and that nothing took a packet kernel) for every key size and rows_block 0 (the library's
   cut) / 1 / 3 (a run of rows cut by block boundaries); fixed-size records -- the plan-free form, message m owns units [m U, (m + 1) U) -- by the library's own rule;
2. ROUTED calls of the product library with the mark at row scale: the row launches run on the context's side stream, the packet kernels on the caller's, and in the
   route grid every boundary of the byte-packed buffer lies between a message of the one and a message of the other, at every residue, with the sizes mark - 1, mark
   and mark + 1 on either side.  Every call asserts route_min (a constant derived below from the rule, never taken from a run) and n_small (counted here).

The same cells run through the lane code on the host in tests/host_emul/emul.cpp (test_rows_grid), the `lc` set under the sanitizers at level 1.

Measured on an MI355X, this file and tests/test_gpu_pkt_grid.py in one run: the slowest case here 0.45 s (rows_block 0, AES-128: the first case, which also
builds the references of its key size; the others 0.13 - 0.27 s, the routed cases 0.02 s), the slowest tests/test_gpu_pkt_grid.py case 0.21 s (wave, AES-128).
The mutations of the row code that this grid is meant to catch were run through the host emulation only, not on the GPU."""
import pytest

import rows_grid as RG
from grid_legs import SPLIT, _fixed_records_leg, _packed_leg, _reference_of, _route, _scattered_leg, _up

pytestmark = pytest.mark.gpu

# The mark of a routed call.  csrc/aesgcm_host.hip route_marks: the high mark is the size class c_hi = rows_min / 64 (64-byte classes, below PKT_LEN_CLASSES = 256), the low
# one (rows_min / 4) / 64.  csrc/aesgcm_kernels.hip route_decide: with route_mid_min = 0 the test `mid >= mid_min` always holds, so the mark is the high one (the band rule
# above it needs route_top_min = 458 752 messages); with route_blocks_min = 0 the "everything by rows" branch is never taken; so route_min = c_hi * 64: rows_min rounded
# DOWN to a size class.  rows_min = 2100 is deliberately no multiple of 64.
ROUTE_ROWS_MIN = 2100
ROUTE_MARK = ROUTE_ROWS_MIN // 64 * 64
assert ROUTE_MARK == 2048 == 2 * RG.ROW
FIXED_LENGTHS = [2048 + 17, 2048 + 257, 3 * 1024 + 1023, 4096]


def _ref(orc, kind, klen, D):
    """the reference of a grid of rows_grid.py (one per kind and key size: rows_block changes the cut, not the bytes); cell_extra names the cut of this case"""
    make = {"packed": RG.Packed, "scattered": RG.Scattered, "inplace": lambda: RG.Scattered(True),
            "route": lambda: RG.Route(ROUTE_MARK), "route_scattered": lambda: RG.RouteScattered(ROUTE_MARK), "route_inplace": lambda: RG.RouteScattered(ROUTE_MARK, True)}[kind]
    R = _reference_of(orc, ("rows_grid", kind, klen), make, klen, 0x7095D000 + 16 * klen + sorted(("packed", "scattered", "inplace", "route", "route_scattered", "route_inplace")).index(kind))
    R.cell_extra = lambda j: dict({k: v for k, v in R.grid.cell(j).items() if k in ("R", "tail_blocks", "aad_blocks", "size", "by")}, rows_block=D)
    return R


def _rows_case(hip, orc, klen, D):
    name = "rows D=%d AES-%d" % (D, 8 * klen)
    R, S, SI = _ref(orc, "packed", klen, D), _ref(orc, "scattered", klen, D), _ref(orc, "inplace", klen, D)
    d_ivs, d_aad, d_doff, d_aoff = _up(hip, R.ivs), _up(hip, R.aad_arena), _up(hip, R.grid.doff.tobytes()), _up(hip, R.grid.aoff.tobytes())
    ctx = hip.Context(R.keys[0]).set_option("rows_block", D)

    def crypt(dec, d_in, d_out, d_tags, d_exp, d_auth):
        ctx.packets_crypt_dev(dec, R.n, d_ivs.ptr, d_in, d_out, d_tags, d_data_off=d_doff.ptr, d_aad=d_aad.ptr, d_aad_off=d_aoff.ptr, d_expect_tags=d_exp, d_auth=d_auth)

    def wipe(on, d_out, d_auth):
        if d_out is None:
            ctx.set_option("wipe_on_auth_fail", int(on))

    _packed_leg(hip, R, d_aad, crypt, lambda lab: _route(hip, ctx, R.n, 0, lab), wipe, name)            # (_route, lanes 0: status OK and n_small == 0)
    assert S.keys == SI.keys == R.keys
    _scattered_leg(hip, ctx, S, SI, 0, name)
    ctx.close()
    return R.keys[0]


@pytest.mark.parametrize("klen", [16, 24, 32])
@pytest.mark.parametrize("rows_block", [0, 1, 3])
def test_row_kernels_on_the_row_scale_grid(hip, orc, rows_block, klen):
    """aesgcm_packets_crypt_dev (offset arrays) and aesgcm_messages_crypt_dev by rows: every (start, length) cell of rows_grid.Packed and every residue pair of
    rows_grid.Scattered, with the library's cut and with dealt blocks of 1 and of 3 units; then fixed-size records of 2 .. 4 rows with and without a long tail at all 16
    residues, by the product library's own rule"""
    with hip.debug_library() as dbg:
        dbg.force(pkt_rows=1)
        key = _rows_case(hip, orc, klen, rows_block)
    ctx = hip.Context(key).set_option("rows_block", rows_block)
    _fixed_records_leg(hip, orc, ctx, klen, key, "rows D=%d AES-%d" % (rows_block, 8 * klen), lens=FIXED_LENGTHS, aad_cycle=RG.AAD_CYCLE, shape=hip.SHAPE_ROWS,
                       form="plan-free form", cell_extra=lambda l, a: dict(RG.geometry(l, a), rows_block=rows_block))
    ctx.close()


@pytest.mark.parametrize("klen", [16, 32])
def test_routed_calls_at_the_mark_and_across_kernel_boundaries(hip, orc, klen):
    """the product library with the mark at two rows: messages of mark - 1 bytes (data + AAD) take a packet kernel, those of mark and mark + 1 go by rows, and they
    alternate in one byte-packed buffer -- or lie 1 .. 19 guard bytes apart -- so that the two kernels, on two streams, write either side of every boundary"""
    name = "routed AES-%d" % (8 * klen)
    R, S, SI = _ref(orc, "route", klen, 0), _ref(orc, "route_scattered", klen, 0), _ref(orc, "route_inplace", klen, 0)
    n_small = sum(1 for l, a in zip(R.lens, R.aads) if l + a < ROUTE_MARK)
    assert 0 < n_small < R.n and (S.lens, S.aads) == (SI.lens, SI.aads) == (R.lens, R.aads)
    assert {l + a for l, a in zip(R.lens, R.aads)} >= {ROUTE_MARK - 1, ROUTE_MARK, ROUTE_MARK + 1, 0, ROUTE_MARK // 4}
    d_ivs, d_aad, d_doff, d_aoff = _up(hip, R.ivs), _up(hip, R.aad_arena), _up(hip, R.grid.doff.tobytes()), _up(hip, R.grid.aoff.tobytes())
    ctx = hip.Context(R.keys[0]).set_option("rows_min", ROUTE_ROWS_MIN)
    for k, v in SPLIT.items():
        ctx.set_option(k, v)

    def route(n, lab):
        hip.dev_sync()
        assert ctx.status() == (hip.STATUS_OK, 0), lab
        r = ctx.last_route()
        assert r["route_min"] == ROUTE_MARK and r["n_small"] == n_small and 0 < r["n_small"] < n, (lab, r, n_small)
        return r

    def crypt(dec, d_in, d_out, d_tags, d_exp, d_auth):
        ctx.packets_crypt_dev(dec, R.n, d_ivs.ptr, d_in, d_out, d_tags, d_data_off=d_doff.ptr, d_aad=d_aad.ptr, d_aad_off=d_aoff.ptr, d_expect_tags=d_exp, d_auth=d_auth)

    def wipe(on, d_out, d_auth):
        if d_out is None:
            ctx.set_option("wipe_on_auth_fail", int(on))

    _packed_leg(hip, R, d_aad, crypt, lambda lab: route(R.n, lab), wipe, name)
    assert S.keys == SI.keys == R.keys
    _scattered_leg(hip, ctx, S, SI, route, name)
    ctx.close()
