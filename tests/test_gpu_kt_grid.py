"""GPU: the key-table family on the alignment grid of tests/kt_grid.py -- wire frames (k_kt_wire), their 64-bit-number forms (k_kt_wirex), TLS records (k_kt_tls) and
QUIC packets (k_kt_quic, k_kt_quic_hp) at every payload start residue, ragged end, ICV residue, turn of the lane group's loop and guard byte.

Each case forces a lane count (the debug library's batch_lanes) and runs one mode's grid, in which every cell occurs (the generator asserts it), in arenas with 256
canary bytes in front and behind: encrypt in place (both bases on 16: the per-packet `aligned` path wherever a payload starts on 16); encrypt out of place with the
output base 5 bytes off the input's (p.aligned false with an aligned input, input and output residues differ); decrypt of the reference's frames with one ICV in seven
forged (one bit inside its first tag_len bytes), in place and out of place, each with aesgcm_wipe_failed_dev behind it.  Compared every time: the WHOLE output arena,
canaries included; the input arena after out-of-place calls; the verdicts (and QUIC's decoded packet numbers) between guards; kt.status() == (OK, 0).  A mismatch names
the first differing frame and its cell.  The expected bytes are kt_common.grid_reference's: libcrypto (oracle/evp_batch.c) with nonce and AAD by each family's formulas,
QUIC by tests/quic_fixture.py -- never another GPU path; tests/test_kt_grid_cpu.py opens them again on the CPU.

The launch ordered by falling length class runs every mode at 8 and 16 lanes.  The library exports nothing that reports the order taken; the debug library's
batch_order forces it at any count (aesgcm_host.hip, batch_plan: `ordered = lg < 6 && p.data_off && g_force.batch_order == 1`), 2 switches it off.

TIMING: NOT MEASURED -- this file has not run on a GPU yet.  Off the GPU a case's reference (12 600 .. 13 600 frames, 5.5 .. 5.9 MB; QUIC 8 456 packets, 1.5 MB) takes
0.7 .. 0.8 s, from libcrypto and from the QUIC fixture alike, once per (mode, key size).  The neighbour to measure beside it is
test_gpu_pkt_grid.py::test_per_packet_key_batch_on_the_alignment_grid (10 641 packets, 4.6 MB at 64 lanes)."""
import struct

import numpy as np
import pytest

import kt_common as KC
import kt_grid as KG
import pkt_grid as PG
from kt_common import Guarded, evp, up_arena as _up  # noqa: F401

pytestmark = pytest.mark.gpu

KEY_LENS = (16, 24, 32)
FULL = ("macsec", "xpn", "esn16", "tls13", "tls12", "quic")            # lanes x key length: every (NR, DEC, LG) instance of every family kernel
ONE_KEY = ("esp16", "macsec_auth", "esp12", "esp8")                    # all three lane counts, the key length rotating
CASES = [(m, lanes, kl) for m in FULL for lanes in KG.LANES for kl in KEY_LENS] + \
        [(m, lanes, KEY_LENS[(i + j) % 3]) for i, m in enumerate(ONE_KEY) for j, lanes in enumerate(KG.LANES)]
# the ordered launch: every mode at 8 and 16 lanes, the key length rotating within each family so that all three occur (QUIC is one mode: a third case for it)
_FAMILIES = {}
for _m in KG.MODES:
    _FAMILIES.setdefault(KG.MODES[_m][0], []).append(_m)
ORDERED = [(m, lanes, KEY_LENS[(i + j) % 3]) for ms in _FAMILIES.values() for i, m in enumerate(ms) for j, lanes in enumerate((8, 16))] + [("quic", 8, 32)]
SHIFT = 5


def _canary(size):
    return np.full(size + 16, PG.CANARY_OUT, dtype=np.uint8)


def _shifted(g, src, wiped=False):
    """what an out-of-place call SHIFT bytes off leaves: canary, and the frames of arena `src` SHIFT bytes on"""
    a = _canary(g.size)
    lo, hi = PG.GUARD, int(g.off[-1])
    a[lo + SHIFT:hi + SHIFT] = src[lo:hi]
    return _wiped(g, a, SHIFT) if wiped else a


def _wiped(g, arena, shift=0):
    a = np.array(arena)
    for i in g.forged:
        a[g.at[i] + shift:g.at[i] + shift + g.flen[i]] = 0
    return a


def _same(g, d_buf, want, shift, label):
    """the whole arena: on a difference, the first differing frame and its cell"""
    got = bytes(d_buf.download(len(want)))
    x = PG.first_difference(got, want)
    if x is None:
        return
    j, off = PG.owner([a + shift for a in g.at], g.flen, x)
    if off is None:
        where = "guard byte %d bytes in front of frame %d" % (g.at[j] + shift - x, j) if j < g.n else "guard byte behind the last frame"
        if j > 0:
            where += ", %d bytes behind frame %d" % (x - (g.at[j - 1] + shift + g.flen[j - 1]) + 1, j - 1)
            j -= 1
        j = min(j, g.n - 1)
    else:
        front = g.fronts[j]
        part = "front" if off < front else "ICV" if off >= g.flen[j] - g.tag_len else "payload"
        where = "byte %d of frame %d (%s)" % (off, j, part)
    raise AssertionError("%s: arena byte %d is %02x, wanted %02x: %s; out residue %d; cell %r" % (label, x, got[x], int(want[x]), where, (g.at[j] + shift) % 16, g.cell(j)))


def _verdicts(R, d_auth, label):
    auth = np.frombuffer(d_auth.read(label), dtype=np.int32)
    bad = np.flatnonzero(auth != np.array(R.auth, dtype=np.int32)).tolist()
    assert not bad, (label, "d_auth: other frames than the forged ones fail", [R.g.cell(i) for i in bad[:4]])


class Call:
    """one mode's call with its device arrays; a QUIC decrypt gets fresh packet-number arrays (expected in, decoded out between guards)"""

    def __init__(self, hip, R, kt):
        g = self.g = R.g
        self.hip, self.R, self.kt = hip, R, kt
        self.d_slots, self.d_off = _up(hip, KC._u32(g.slots)), _up(hip, g.off.tobytes())
        if g.number == "hi":
            self.d_num = _up(hip, KC._u32(g.nums))
        elif g.number:
            self.d_num = _up(hip, KC._u64(g.nums))
        if g.family == "quic":
            self.d_hps, self.d_pn_off, self.d_exp = _up(hip, KC._u32(g.hps)), _up(hip, KC._u32(g.pn_off)), _up(hip, KC._u64(g.expected_pns))
        self.pn_out = None

    def __call__(self, dec, d_in, d_out, d_auth=None):
        g, kt, n = self.g, self.kt, self.g.n
        if g.family == "wire":
            kt.frames_crypt_dev(dec, self.R.fmt, n, self.d_slots.ptr, d_in, self.d_off.ptr, d_out, d_auth=d_auth)
        elif g.family == "wirex":
            kt.frames_crypt_x_dev(dec, self.R.fmt, n, self.d_slots.ptr, self.d_num.ptr, d_in, self.d_off.ptr, d_out, d_auth=d_auth)
        elif g.family == "tls":
            kt.records_crypt_dev(dec, self.R.fmt, n, self.d_slots.ptr, self.d_num.ptr, d_in, self.d_off.ptr, d_out, d_auth=d_auth)
        else:
            self.pn_out = Guarded(self.hip, 8 * n) if dec else None
            kt.quic_crypt_dev(dec, n, self.d_slots.ptr, self.d_hps.ptr, (self.d_exp if dec else self.d_num).ptr, self.d_pn_off.ptr, d_in, self.d_off.ptr, d_out,
                              d_pn_out=self.pn_out.ptr if dec else None, d_auth=d_auth)

    def done(self, label, dec=False):
        self.hip.dev_sync()
        assert self.kt.status() == (self.hip.OK, 0), label
        if dec and self.pn_out is not None:
            pns = list(struct.unpack("<%dQ" % self.g.n, self.pn_out.read(label)))
            bad = [i for i in range(self.g.n) if pns[i] != self.R.pn_out[i]]
            assert not bad, (label, "pn_out", [(pns[i], self.R.pn_out[i], self.g.cell(i)) for i in bad[:4]])

    def wipe(self, d_out, d_auth):
        self.hip.wipe_failed_dev(self.g.n, d_out, d_auth.ptr, d_data_off=self.d_off.ptr)
        self.hip.dev_sync()


def _legs(hip, R, kt, name, out_of_place=True):
    g = R.g
    call = Call(hip, R, kt)
    lab = name + " enc in place"
    d_io = _up(hip, g.arena)
    call(False, d_io.ptr, d_io.ptr)
    call.done(lab)
    _same(g, d_io, R.enc, 0, lab)
    if out_of_place:
        lab = name + " enc out of place, output %d bytes off" % SHIFT
        d_in, d_out = _up(hip, g.arena), _up(hip, _canary(g.size))
        call(False, d_in.ptr, d_out.ptr + SHIFT)
        call.done(lab)
        _same(g, d_out, _shifted(g, R.enc), SHIFT, lab)
        _same(g, d_in, g.arena, 0, lab + " (input arena)")
    lab = name + " dec in place, one ICV in %d forged" % PG.FORGE_EVERY
    d_io, d_auth = _up(hip, R.dec_in), Guarded(hip, 4 * g.n)
    call(True, d_io.ptr, d_io.ptr, d_auth.ptr)
    call.done(lab, dec=True)
    _verdicts(R, d_auth, lab)
    _same(g, d_io, R.dec_out, 0, lab)
    call.wipe(d_io.ptr, d_auth)
    _same(g, d_io, _wiped(g, R.dec_out), 0, lab + ", wiped")
    _verdicts(R, d_auth, lab + ", wiped")
    if out_of_place:
        lab = name + " dec out of place, output %d bytes off, one ICV in %d forged" % (SHIFT, PG.FORGE_EVERY)
        d_in, d_out, d_auth = _up(hip, R.dec_in), _up(hip, _canary(g.size)), Guarded(hip, 4 * g.n)
        call(True, d_in.ptr, d_out.ptr + SHIFT, d_auth.ptr)
        call.done(lab, dec=True)
        _verdicts(R, d_auth, lab)
        _same(g, d_out, _shifted(g, R.dec_out), SHIFT, lab)
        _same(g, d_in, R.dec_in, 0, lab + " (input arena)")
        call.wipe(d_out.ptr + SHIFT, d_auth)
        _same(g, d_out, _shifted(g, R.dec_out, wiped=True), SHIFT, lab + ", wiped")
        _same(g, d_in, R.dec_in, 0, lab + ", wiped (input arena)")


@pytest.mark.parametrize("mode, lanes, key_len", CASES)
def test_key_table_family_on_the_alignment_grid(hip, evp, mode, lanes, key_len):  # noqa: F811
    R = KC.grid_reference(hip, evp, mode, key_len)
    with hip.debug_library() as dbg:
        dbg.force(batch_lanes=lanes)
        with KC.grid_table(hip, R) as kt:
            _legs(hip, R, kt, "%s lanes %d AES-%d" % (mode, lanes, 8 * key_len))


def test_the_cases_run_every_instance():
    """every (key size, lane count) of every family kernel: 3 x 3 per kernel instantiation (direction is every case's); the rotating cases see every key size"""
    for fam, ms in _FAMILIES.items():
        assert {(l, k) for m, l, k in CASES if m in ms and m in FULL} == {(l, k) for l in KG.LANES for k in KEY_LENS}, fam
        assert {k for m, l, k in ORDERED if m in ms} == set(KEY_LENS), fam
    assert {m for m, _, _ in CASES} == set(KG.MODES) == {m for m, _, _ in ORDERED}
    for m in ONE_KEY:
        assert {l for mm, l, _ in CASES if mm == m} == set(KG.LANES) and len({k for mm, _, k in CASES if mm == m}) == 3


@pytest.mark.parametrize("mode, lanes, key_len", ORDERED)
def test_ordered_launch_on_the_alignment_grid(hip, evp, mode, lanes, key_len):  # noqa: F811
    """BatchParams::perm for every family kernel: under the order TLS 1.2 and ESN rebuild their AAD block from a recomputed packet index, QUIC reads seq, pn_off and
    hp_slots through the map.  batch_order = 1 forces the order at any count (aesgcm_host.hip, batch_plan: `ordered = lg < 6 && p.data_off && g_force.batch_order == 1`;
    8 and 16 lanes are lg 3 and 4), 2 switches it off; both must give the reference's bytes.  The order is a counting sort by falling length class, the class of a
    frame being min(frame bytes >> 6, 255) (aesgcm_pkt.h, pkt_len_class, on the frame's offsets: order_launch's LenSrc): the grid spans several, asserted here."""
    R = KC.grid_reference(hip, evp, mode, key_len)
    classes = KG.length_classes(R.g)
    assert len(classes) >= 8 and classes[0] == 0 and classes[-1] >= 32, classes
    for order in (1, 2):
        with hip.debug_library() as dbg:
            dbg.force(batch_lanes=lanes, batch_order=order)
            with KC.grid_table(hip, R) as kt:
                _legs(hip, R, kt, "%s lanes %d AES-%d batch_order %d" % (mode, lanes, 8 * key_len, order), out_of_place=False)
