"""What the GPU tests on the alignment grids share (tests/test_gpu_pkt_grid.py on tests/pkt_grid.py, tests/test_gpu_rows_grid.py on tests/rows_grid.py): the reference of
a grid -- its inputs and what the CPU oracle (orc.Fast; never another GPU path) makes of them, computed once per grid and key size and never written to --, the
comparison of WHOLE arenas that names the first differing packet with its cell, and the legs every case runs: encrypt out of place with the output 5 residues off and
in place, decrypt of the oracle's ciphertext with one tag in seven forged -- unwiped out of place, wiped in place, wiped out of place at the other residues --, the
scattered legs (messages wherever they live), and fixed-size records."""
import struct

import numpy as np

import pkt_grid as PG
from kt_common import Guarded, up_arena as _up
from util import splitmix_bytes

G_ = PG.GUARD
SPLIT = dict(route_mid_min=0, route_blocks_min=0)                # the library's own rule sends calls this small by rows altogether (tests/test_gpu_mixed.py)
N_KEYS = 11                                                      # distinct keys of the per-packet-key leg (every packet has a key of its own in the array; they repeat with period 11)


# ---------------------------------------------------------------------------------------------- references (computed once per grid and key size, never written to)
class Ref:
    pass


_REFS = {}


def _arena(size, canary, seed, starts, lens):
    """canary everywhere, seeded bytes inside the packets"""
    a = np.full(size, canary, dtype=np.uint8)
    r = np.frombuffer(splitmix_bytes(seed, size), dtype=np.uint8)
    for s, l in zip(starts, lens):
        a[s:s + l] = r[s:s + l]
    a.setflags(write=False)
    return a


def _reference(orc, kind, G, klen, per_packet_keys=False):
    """a grid of tests/pkt_grid.py"""
    seed = 0x9A1D0000 + 4096 * G + 16 * klen + {"packed": 0, "scattered": 1, "inplace": 2}[kind] + (8 if per_packet_keys else 0)
    return _reference_of(orc, (kind, G, klen, per_packet_keys), lambda: PG.Packed(G) if kind == "packed" else PG.Scattered(G, inplace=(kind == "inplace")), klen, seed,
                         N_KEYS if per_packet_keys else 1)


def _reference_of(orc, k, make_grid, klen, seed, n_keys=1):
    """the grid (byte-packed: it has doff / aoff; else scattered), its inputs and what the oracle makes of them: ct[i], tags; arenas are assembled from these by the legs.
    k: what the reference is kept under"""
    if k in _REFS:
        return _REFS[k]
    R = Ref()
    R.grid = g = make_grid()
    R.n, R.lens, R.aads = g.n, g.lens, g.aads
    if hasattr(g, "doff"):
        R.in_at, R.out_at, R.aad_at = [int(x) for x in g.doff[:-1]], [int(x) for x in g.doff[:-1]], [int(x) for x in g.aoff[:-1]]
        R.size_in, R.size_out, R.size_aad = g.size, g.size, g.aad_size
    else:
        R.in_at, R.out_at, R.aad_at, R.size_in, R.size_out, R.size_aad = g.pos_in, g.pos_out, g.pos_aad, g.size_in, g.size_out, g.size_aad
    R.keys = [splitmix_bytes(0x9A1DEE00 + 16 * klen + j, klen) for j in range(n_keys)]      # one key per key size: a case has one context
    R.ivs = splitmix_bytes(seed + 1, 12 * R.n)
    R.pt_arena = _arena(R.size_in, PG.CANARY_IN, seed + 2, R.in_at, R.lens)
    R.aad_arena = _arena(R.size_aad, PG.CANARY_IN, seed + 3, R.aad_at, R.aads)
    pt, aad = R.pt_arena.tobytes(), R.aad_arena.tobytes()
    fast = [orc.Fast(key) for key in R.keys]
    R.ct, tags = [], []
    for i in range(R.n):
        c, t = fast[i % len(fast)].encrypt(R.ivs[12 * i:12 * i + 12], aad[R.aad_at[i]:R.aad_at[i] + R.aads[i]], pt[R.in_at[i]:R.in_at[i] + R.lens[i]])
        R.ct.append(np.frombuffer(c, dtype=np.uint8))
        tags.append(t)
    R.tags = b"".join(tags)
    R.forged = PG.forged(R.n)
    bad = bytearray(R.tags)
    for i in R.forged:
        bad[16 * i + i % 16] ^= 1 << (i % 8)
    R.bad_tags = bytes(bad)
    _REFS[k] = R
    return R


def _assemble(R, base, at, what, shift=0, wiped=False):
    """a copy of arena `base` with every packet's ciphertext ("ct") or plaintext ("pt") at at[i] + shift; wiped: zeros in the forged packets' places"""
    a = np.array(base, dtype=np.uint8)
    for i in range(R.n):
        l = R.lens[i]
        if l:
            a[at[i] + shift:at[i] + shift + l] = R.ct[i] if what == "ct" else R.pt_arena[R.in_at[i]:R.in_at[i] + l]
    if wiped:
        for i in R.forged:
            a[at[i] + shift:at[i] + shift + R.lens[i]] = 0
    return a


# ---------------------------------------------------------------------------------------------- device side helpers
def _canary(size, shift=0):
    return np.full(size + shift, PG.CANARY_OUT, dtype=np.uint8)


def _same(R, d_buf, want, at, shift, label):
    """the whole arena: on a difference, the first differing packet and its cell"""
    got = bytes(d_buf.download(len(want)))
    x = PG.first_difference(got, want)
    if x is None:
        return
    j, off = PG.owner([a + shift for a in at], R.lens, x)
    if off is None:
        where = "guard byte %d bytes in front of packet %d" % (at[j] + shift - x, j) if j < R.n else "guard byte behind the last packet"
        if j > 0:
            where += ", %d bytes behind packet %d (length %d, output residue %d)" % (x - (at[j - 1] + shift + R.lens[j - 1]) + 1, j - 1, R.lens[j - 1], (at[j - 1] + shift) % 16)
        j = min(j, R.n - 1)
    else:
        where = "byte %d of packet %d" % (off, j)
    cell = dict(in_res=R.in_at[j] % 16, in_res128=R.in_at[j] % 128, out_res=(at[j] + shift) % 16, out_res128=(at[j] + shift) % 128, length=R.lens[j], aad=R.aads[j], aad_res=R.aad_at[j] % 16)
    cell.update(getattr(R, "cell_extra", lambda j: {})(j))          # (tests/rows_grid.py: R, tail blocks, AAD blocks, rows_block)
    raise AssertionError("%s: arena byte %d is %02x, wanted %02x: %s; cell %r" % (label, x, got[x], int(want[x]), where, cell))


def _tags_same(R, got, label):
    if got != R.tags:
        i = next(i for i in range(R.n) if got[16 * i:16 * i + 16] != R.tags[16 * i:16 * i + 16])
        raise AssertionError("%s: tag of packet %d; cell %r" % (label, i, R.grid.cell(i)))


def _verdicts(R, d_auth, label):
    auth = np.frombuffer(d_auth.read(label), dtype=np.int32)
    assert set(np.unique(auth).tolist()) <= {0, 1} and np.flatnonzero(auth == 0).tolist() == R.forged, (label, "d_auth names other packets than the forged ones",
                                                                                                      sorted(set(np.flatnonzero(auth == 0).tolist()) ^ set(R.forged))[:8])


def _route(hip, ctx, n, lanes, label):
    """after a routed call: not refused, and taken by the kernel the case names"""
    hip.dev_sync()
    assert ctx.status() == (hip.STATUS_OK, 0), label
    r = ctx.last_route()
    if lanes is None:
        return r                                                  # the product library's own choice: part of the assertion messages only
    if lanes == 0:
        assert r["n_small"] == 0, (label, "by rows: nothing may take the packet kernels", r)
    else:
        assert r["n_small"] == n and r["lanes"] == lanes, (label, r)
    return r


# ---------------------------------------------------------------------------------------------- the legs
def _packed_leg(hip, R, d_aad, crypt, route, wipe, name):
    """crypt(decrypt, d_in_ptr, d_out_ptr, d_tags_ptr, d_expect_ptr, d_auth_ptr); route(label); wipe(on, d_out_ptr, d_auth_ptr): the ways the one-key and the per-packet-key calls differ"""
    n, at = R.n, R.in_at
    d_pt = _up(hip, R.pt_arena)
    ct_arena = _assemble(R, R.pt_arena, at, "ct")                       # the oracle's ciphertext between the input's guards
    # encrypt out of place, the output 5 bytes off the input's residues
    lab = name + " packed enc out of place"
    d_out, d_tags = _up(hip, _canary(R.size_out, 16)), Guarded(hip, 16 * n)
    crypt(False, d_pt.ptr, d_out.ptr + 5, d_tags.ptr, None, None)
    r = route(lab)
    lab += " route %r" % (r,)
    _same(R, d_out, _assemble(R, _canary(R.size_out, 16), at, "ct", shift=5), at, 5, lab)
    _tags_same(R, d_tags.read(lab), lab)
    _same(R, d_pt, R.pt_arena, at, 0, lab + " (input arena)")
    _same(R, d_aad, R.aad_arena, R.aad_at, 0, lab + " (AAD arena)")
    # encrypt in place, both on 16-byte boundaries (the aligned paths)
    lab = name + " packed enc in place"
    d_io, d_tags = _up(hip, R.pt_arena), Guarded(hip, 16 * n)
    crypt(False, d_io.ptr, d_io.ptr, d_tags.ptr, None, None)
    route(lab)
    _same(R, d_io, ct_arena, at, 0, lab)
    _tags_same(R, d_tags.read(lab), lab)
    # decrypt the oracle's ciphertext out of place, forged tags, nothing wiped
    lab = name + " packed dec out of place"
    d_ct, d_exp = _up(hip, ct_arena), _up(hip, R.bad_tags)
    d_out, d_tags, d_auth = _up(hip, _canary(R.size_out)), Guarded(hip, 16 * n), Guarded(hip, 4 * n)
    wipe(False, None, None)
    crypt(True, d_ct.ptr, d_out.ptr, d_tags.ptr, d_exp.ptr, d_auth.ptr)
    route(lab)
    _same(R, d_out, _assemble(R, _canary(R.size_out), at, "pt"), at, 0, lab)
    _tags_same(R, d_tags.read(lab), lab)
    _verdicts(R, d_auth, lab)
    _same(R, d_ct, ct_arena, at, 0, lab + " (input arena)")
    # ... in place, the failed packets wiped
    lab = name + " packed dec in place, wiped"
    d_io, d_tags, d_auth = _up(hip, ct_arena), Guarded(hip, 16 * n), Guarded(hip, 4 * n)
    wipe(True, None, None)
    crypt(True, d_io.ptr, d_io.ptr, d_tags.ptr, d_exp.ptr, d_auth.ptr)
    wipe(True, d_io.ptr, d_auth.ptr)
    route(lab)
    _verdicts(R, d_auth, lab)
    _same(R, d_io, _assemble(R, R.pt_arena, at, "pt", wiped=True), at, 0, lab)
    _tags_same(R, d_tags.read(lab), lab)
    # ... out of place at the other residues, wiped
    lab = name + " packed dec out of place, wiped"
    d_out, d_tags, d_auth = _up(hip, _canary(R.size_out, 16)), Guarded(hip, 16 * n), Guarded(hip, 4 * n)
    crypt(True, d_ct.ptr, d_out.ptr + 5, d_tags.ptr, d_exp.ptr, d_auth.ptr)
    wipe(True, d_out.ptr + 5, d_auth.ptr)
    route(lab)
    _verdicts(R, d_auth, lab)
    _same(R, d_out, _assemble(R, _canary(R.size_out, 16), at, "pt", shift=5, wiped=True), at, 5, lab)
    _same(R, d_aad, R.aad_arena, R.aad_at, 0, lab + " (AAD arena)")
    wipe(False, None, None)


def _u64s(hip, base, at):
    return _up(hip, struct.pack("<%dQ" % len(at), *[base + a for a in at]))


def _scattered_leg(hip, ctx, R, RI, lanes, name):
    """aesgcm_messages_crypt_dev: R every (input residue, output residue) pair out of place, RI every (residue, length) in place.  lanes: what _route asserts of
    every call, or route(n, label) -> the route, a case's own assertion"""
    route = lanes if callable(lanes) else (lambda n, lab: _route(hip, ctx, n, lanes, lab))
    n = R.n
    d_ivs, d_len, d_alen = _up(hip, R.ivs), _up(hip, struct.pack("<%dI" % n, *R.lens)), _up(hip, struct.pack("<%dI" % n, *R.aads))
    d_pt, d_aad = _up(hip, R.pt_arena), _up(hip, R.aad_arena)
    ct_arena = _assemble(R, _canary(R.size_out), R.out_at, "ct")         # the oracle's ciphertext at the output's places
    d_inp, d_aadp = _u64s(hip, d_pt.ptr, R.in_at), _u64s(hip, d_aad.ptr, R.aad_at)
    lab = name + " scattered enc out of place"
    d_out, d_tags = _up(hip, _canary(R.size_out)), Guarded(hip, 16 * n)
    d_outp = _u64s(hip, d_out.ptr, R.out_at)
    ctx.set_option("wipe_on_auth_fail", 0)
    ctx.messages_crypt_dev(False, n, d_ivs.ptr, d_inp.ptr, d_len.ptr, d_outp.ptr, d_tags.ptr, d_aad_ptr=d_aadp.ptr, d_aad_len=d_alen.ptr)
    r = route(n, lab)
    lab += " route %r" % (r,)
    _same(R, d_out, ct_arena, R.out_at, 0, lab)
    _tags_same(R, d_tags.read(lab), lab)
    _same(R, d_pt, R.pt_arena, R.in_at, 0, lab + " (input arena)")
    _same(R, d_aad, R.aad_arena, R.aad_at, 0, lab + " (AAD arena)")
    # decrypt the oracle's ciphertext to a third arena at the input's places: first unwiped, then wiped
    d_ct, d_exp = _up(hip, ct_arena), _up(hip, R.bad_tags)
    d_ctp = _u64s(hip, d_ct.ptr, R.out_at)
    for wiped in (False, True):
        lab = name + " scattered dec out of place" + (", wiped" if wiped else "")
        d_back, d_tags, d_auth = _up(hip, _canary(R.size_in)), Guarded(hip, 16 * n), Guarded(hip, 4 * n)
        d_backp = _u64s(hip, d_back.ptr, R.in_at)
        ctx.set_option("wipe_on_auth_fail", int(wiped))
        ctx.messages_crypt_dev(True, n, d_ivs.ptr, d_ctp.ptr, d_len.ptr, d_backp.ptr, d_tags.ptr, d_aad_ptr=d_aadp.ptr, d_aad_len=d_alen.ptr, d_expect_tags=d_exp.ptr, d_auth=d_auth.ptr)
        route(n, lab)
        _verdicts(R, d_auth, lab)
        _same(R, d_back, _assemble(R, _canary(R.size_in), R.in_at, "pt", wiped=wiped), R.in_at, 0, lab)
        _tags_same(R, d_tags.read(lab), lab)
        _same(R, d_ct, ct_arena, R.out_at, 0, lab + " (input arena)")
    # in place: every residue x every length
    n = RI.n
    d_ivs, d_len, d_alen = _up(hip, RI.ivs), _up(hip, struct.pack("<%dI" % n, *RI.lens)), _up(hip, struct.pack("<%dI" % n, *RI.aads))
    d_aad = _up(hip, RI.aad_arena)
    d_aadp = _u64s(hip, d_aad.ptr, RI.aad_at)
    ct_arena = _assemble(RI, RI.pt_arena, RI.in_at, "ct")
    lab = name + " scattered enc in place"
    d_io, d_tags = _up(hip, RI.pt_arena), Guarded(hip, 16 * n)
    d_iop = _u64s(hip, d_io.ptr, RI.in_at)
    ctx.set_option("wipe_on_auth_fail", 0)
    ctx.messages_crypt_dev(False, n, d_ivs.ptr, d_iop.ptr, d_len.ptr, d_iop.ptr, d_tags.ptr, d_aad_ptr=d_aadp.ptr, d_aad_len=d_alen.ptr)
    route(n, lab)
    _same(RI, d_io, ct_arena, RI.in_at, 0, lab)
    _tags_same(RI, d_tags.read(lab), lab)
    lab = name + " scattered dec in place, wiped"
    d_io, d_tags, d_auth, d_exp = _up(hip, ct_arena), Guarded(hip, 16 * n), Guarded(hip, 4 * n), _up(hip, RI.bad_tags)
    d_iop = _u64s(hip, d_io.ptr, RI.in_at)
    ctx.set_option("wipe_on_auth_fail", 1)
    ctx.messages_crypt_dev(True, n, d_ivs.ptr, d_iop.ptr, d_len.ptr, d_iop.ptr, d_tags.ptr, d_aad_ptr=d_aadp.ptr, d_aad_len=d_alen.ptr, d_expect_tags=d_exp.ptr, d_auth=d_auth.ptr)
    route(n, lab)
    _verdicts(RI, d_auth, lab)
    _same(RI, d_io, _assemble(RI, RI.pt_arena, RI.in_at, "pt", wiped=True), RI.in_at, 0, lab)
    _tags_same(RI, d_tags.read(lab), lab)
    _same(RI, d_aad, RI.aad_arena, RI.aad_at, 0, lab + " (AAD arena)")
    ctx.set_option("wipe_on_auth_fail", 0)


def _fixed_records_leg(hip, orc, ctx, klen, key, name, lens=None, aad_cycle=PG.AAD_CYCLE, shape=1, form="ILP form", cell_extra=None):
    """(lens, aad_cycle, shape -- what packets_shape must say of every call --, form: the defaults are the packet kernels' leg; tests/test_gpu_rows_grid.py runs the
    plan-free form of the row kernels through the same code.)
    Fixed-size records -- the only calls that take k_pktl's ILP form (512-lane workgroups, eight keystream blocks side by side; offset arrays are routed and take the
    768-lane form): every length of L_c from 127 bytes, where the form's 128-byte loop and what follows it turn, at all 16 input residues, the output 5 residues
    on, five records per call; one arena each with guards between the calls, compared whole."""
    lens = [l for l in PG.compact_lengths() if l >= 127] if lens is None else lens
    calls, a, b, c, k = [], G_ - 1, G_ - 1, G_ - 1, 0
    nrec = 5
    for l in lens:
        for r in range(16):
            al = aad_cycle[len(calls) % len(aad_cycle)]
            a, b, c = PG._place(a, r, len(calls)), PG._place(b, (r + 5) % 16, len(calls) + 1), PG._place(c, (3 * len(calls) + 1) % 16, len(calls))
            calls.append((l, al, a, b, c, k))
            a, b, c, k = a + nrec * l, b + nrec * l, c + nrec * al, k + nrec
    n = k
    R = Ref()
    R.n, R.lens, R.aads = n, [l for (l, *_r) in calls for _ in range(nrec)], [al for (_l, al, *_r) in calls for _ in range(nrec)]
    R.in_at = [a + j * l for (l, al, a, b, c, k) in calls for j in range(nrec)]
    R.out_at = [b + j * l for (l, al, a, b, c, k) in calls for j in range(nrec)]
    R.aad_at = [c + j * al for (l, al, a, b, c, k) in calls for j in range(nrec)]
    assert {(x % 16, l) for x, l in zip(R.in_at[::nrec], R.lens[::nrec])} == {(r, l) for l in lens for r in range(16)}
    R.size_in, R.size_out, R.size_aad = a + 1 + G_, b + 1 + G_, c + 1 + G_
    R.ivs = splitmix_bytes(0x1F1D + klen, 12 * n)
    R.pt_arena, R.aad_arena = _arena(R.size_in, PG.CANARY_IN, 0x1F1E + klen, R.in_at, R.lens), _arena(R.size_aad, PG.CANARY_IN, 0x1F1F + klen, R.aad_at, R.aads)
    pt, aad, f = R.pt_arena.tobytes(), R.aad_arena.tobytes(), orc.Fast(key)
    res = [f.encrypt(R.ivs[12 * i:12 * i + 12], aad[R.aad_at[i]:R.aad_at[i] + R.aads[i]], pt[R.in_at[i]:R.in_at[i] + R.lens[i]]) for i in range(n)]
    R.ct, R.tags = [np.frombuffer(x[0], dtype=np.uint8) for x in res], b"".join(x[1] for x in res)
    R.forged = PG.forged(n)
    bad = bytearray(R.tags)
    for i in R.forged:
        bad[16 * i + i % 16] ^= 1 << (i % 8)
    R.grid = type("G", (), {"cell": staticmethod(lambda i: dict(pkt=i, in_res=R.in_at[i] % 16, out_res=R.out_at[i] % 16, length=R.lens[i], aad=R.aads[i]))})
    if cell_extra:
        R.cell_extra = lambda j: cell_extra(R.lens[j], R.aads[j])
    assert all({al for (l, al, *_r) in calls if l == ll} >= set(aad_cycle) for ll in lens)          # every AAD length of the cycle with every record length
    d_ivs, d_pt, d_aad, d_exp = _up(hip, R.ivs), _up(hip, R.pt_arena), _up(hip, R.aad_arena), _up(hip, bytes(bad))
    ct_arena = _assemble(R, _canary(R.size_out), R.out_at, "ct")
    lab = name + " fixed-size records (%s) enc" % form
    d_out, d_tags = _up(hip, _canary(R.size_out)), Guarded(hip, 16 * n)
    ctx.set_option("wipe_on_auth_fail", 0)
    for (l, al, a, b, c, k) in calls:
        assert ctx.packets_shape(nrec, l, False) == shape, lab
        ctx.packets_crypt_dev(False, nrec, d_ivs.ptr + 12 * k, d_pt.ptr + a, d_out.ptr + b, d_tags.ptr + 16 * k, pkt_len=l, d_aad=d_aad.ptr + c, aad_len=al)
    hip.dev_sync()
    _same(R, d_out, ct_arena, R.out_at, 0, lab)
    _tags_same(R, d_tags.read(lab), lab)
    _same(R, d_pt, R.pt_arena, R.in_at, 0, lab + " (input arena)")
    lab = name + " fixed-size records (%s) dec, wiped" % form
    d_ct, d_back, d_tags, d_auth = _up(hip, ct_arena), _up(hip, _canary(R.size_in)), Guarded(hip, 16 * n), Guarded(hip, 4 * n)
    ctx.set_option("wipe_on_auth_fail", 1)
    for (l, al, a, b, c, k) in calls:
        ctx.packets_crypt_dev(True, nrec, d_ivs.ptr + 12 * k, d_ct.ptr + b, d_back.ptr + a, d_tags.ptr + 16 * k, pkt_len=l, d_aad=d_aad.ptr + c, aad_len=al,
                              d_expect_tags=d_exp.ptr + 16 * k, d_auth=d_auth.ptr + 4 * k)
    hip.dev_sync()
    _verdicts(R, d_auth, lab)
    _same(R, d_back, _assemble(R, _canary(R.size_in), R.in_at, "pt", wiped=True), R.in_at, 0, lab)
    _tags_same(R, d_tags.read(lab), lab)
    _same(R, d_ct, ct_arena, R.out_at, 0, lab + " (input arena)")
    ctx.set_option("wipe_on_auth_fail", 0)
