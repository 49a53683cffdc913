"""GPU: the key-table family on the alignment grid of tests/kt_grid.py -- wire frames (k_kt_wire), their 64-bit-number forms (k_kt_wirex), TLS records (k_kt_tls),
QUIC packets (k_kt_quic, k_kt_quic_hp), DTLS records (k_kt_dtls, k_kt_dtls_sn) and SRTP / SRTCP packets (k_kt_srtp) at every payload start residue, ragged end, ICV
residue, turn of the lane group's loop and guard byte.

Each case forces a lane count (the debug library's batch_lanes) and runs one mode's grid, in which every cell occurs (the generator asserts it), in arenas with 256
canary bytes in front and behind: encrypt in place (both bases on 16: the per-packet `aligned` path wherever a payload starts on 16); encrypt out of place with the
output base 5 bytes off the input's (p.aligned false with an aligned input, input and output residues differ); decrypt of the reference's frames with one ICV in seven
forged (one bit inside its first tag_len bytes), in place and out of place, each with aesgcm_wipe_failed_dev behind it.  Compared every time: the WHOLE output arena,
canaries included; the input arena after out-of-place calls; the verdicts (and QUIC's and DTLS 1.3's decoded numbers) between guards; kt.status() == (OK, 0).  A mismatch
names the first differing frame, the part of it (front, payload, tag, trailer: Grid.part) and its cell.  The expected bytes are kt_common.grid_reference's: libcrypto
(oracle/evp_batch.c) with nonce and AAD by each family's formulas, QUIC by tests/quic_fixture.py, DTLS by tests/dtls_fixture.py, SRTP and SRTCP by tests/srtp_fixture.py
-- never another GPU path; tests/test_kt_grid_cpu.py opens them again on the CPU.

DTLS and SRTP / SRTCP: k_kt_dtls is instantiated per version and k_kt_srtp per kind, so dtls13, dtls12, srtp and srtcp each run 3 lane counts x 3 key sizes; srtp_mki
(a 4-byte MKI behind the tag) and srtcp_clear (E clear: nothing encrypted, the AAD in two pieces, a trailer of 7) rotate the key size.  A wipe zeroes the whole packet,
trailer included.  Two things stay with the family files, because one grid is one kind of packet and its expected numbers lie just below the records' own: SRTCP packets
with E set and E clear in one call (tests/test_gpu_srtp.py), and DTLS 1.3 decodes that wrap up or down (tests/test_gpu_dtls.py::test_dtls13_grid).

The launch ordered by falling length class runs every mode at 8 and 16 lanes.  The library exports nothing that reports the order taken; the debug library's
batch_order forces it at any count (aesgcm_host.hip, batch_plan: `ordered = lg < 6 && p.data_off && g_force.batch_order == 1`), 2 switches it off.

TIMING, measured on an MI355X (pytest --durations, all 141 cases in one process, 12.8 s together): a case is its reference, built on the CPU once per (mode, key size) and
kept, and 20 ms or less of GPU calls, transfers and comparisons.  So the slowest cases are the ones that build a reference: of the ten older modes macsec-8-16, 0.50 s
(the first case, which also loads both libraries), then xpn-8-16 and esp16-8-16, 0.28 s; of the six newer ones srtcp_clear-8-32 and srtcp-8-16, 0.36 s, dtls12-8-16
0.34 s, dtls13-8-16 0.21 s, srtp-8-16 0.17 s, beside their neighbour quic-8-16 at 0.22 s; every case that finds its reference made takes 0.01 .. 0.02 s, the ordered
ones (two orders each) included.  No new case takes twice its neighbour's time and none is split.  The references alone, off the GPU on a slower host, once per
(mode, key size), AES-128 / 192 / 256: the ten older modes 0.7 .. 0.8 s (12 600 .. 13 600 frames, 5.5 .. 5.9 MB; QUIC 8 456 packets, 1.5 MB), from libcrypto's batch
and from the QUIC fixture alike; dtls12 (12 640 records, 5.7 MB) 1.01 / 0.79 / 1.08 s; dtls13 (8 403, 1.3 MB) 0.64 / 0.70 / 0.59 s; srtp (8 417 packets, 1.6 MB)
0.53 / 0.55 / 0.54 s; srtp_mki (8 405, 1.6 MB) 0.54 / 0.47 / 0.45 s; srtcp (12 641, 5.6 MB) 0.91 / 0.93 / 1.11 s; srtcp_clear (13 648, 5.9 MB) 0.96 / 0.97 / 1.02 s
-- the DTLS and SRTP fixtures call libcrypto once per packet, which costs the large grids a third more than the batch does."""
import struct

import numpy as np
import pytest

import kt_common as KC
import kt_grid as KG
import pkt_grid as PG
from kt_common import Guarded, evp, up_arena as _up  # noqa: F401

pytestmark = pytest.mark.gpu

KEY_LENS = (16, 24, 32)
# lanes x key length: every (NR, DEC, LG) instance of every family kernel -- k_kt_dtls and k_kt_srtp have an instance per version / kind, so two modes each
FULL = ("macsec", "xpn", "esn16", "tls13", "tls12", "quic", "dtls13", "dtls12", "srtp", "srtcp")
ONE_KEY = ("esp16", "macsec_auth", "esp12", "esp8", "srtp_mki", "srtcp_clear")                    # all three lane counts, the key length rotating
PER_MODE = ("dtls", "srtp")                                            # the families in which a kernel instantiation belongs to one mode
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
        where = "byte %d of frame %d (%s)" % (off, j, g.part(j, off))
    raise AssertionError("%s: arena byte %d is %02x, wanted %02x: %s; out residue %d; cell %r" % (label, x, got[x], int(want[x]), where, (g.at[j] + shift) % 16, g.cell(j)))


def _verdicts(R, d_auth, label):
    auth = np.frombuffer(d_auth.read(label), dtype=np.int32)
    bad = np.flatnonzero(auth != np.array(R.auth, dtype=np.int32)).tolist()
    assert not bad, (label, "d_auth: other frames than the forged ones fail", [R.g.cell(i) for i in bad[:4]])


class Call:
    """one mode's call with its device arrays; a QUIC or DTLS 1.3 decrypt gets fresh number arrays (expected in, decoded out between guards)"""

    def __init__(self, hip, R, kt):
        g = self.g = R.g
        self.hip, self.R, self.kt = hip, R, kt
        self.d_slots, self.d_off = _up(hip, KC._u32(g.slots)), _up(hip, g.off.tobytes())
        if g.number in ("hi", "roc"):
            self.d_num = _up(hip, KC._u32(g.nums))
        elif g.number:
            self.d_num = _up(hip, KC._u64(g.nums))
        if g.family == "quic":
            self.d_hps, self.d_pn_off, self.d_exp = _up(hip, KC._u32(g.hps)), _up(hip, KC._u32(g.pn_off)), _up(hip, KC._u64(g.expected_pns))
        self.d13 = g.mode == "dtls13"
        if self.d13:
            self.d_hps, self.d_pn_off, self.d_exp = _up(hip, KC._u32(g.hps)), _up(hip, KC._u32(g.sn_off)), _up(hip, KC._u64(g.expected_seqs))
        self.pn_out = None

    def __call__(self, dec, d_in, d_out, d_auth=None):
        g, kt, n = self.g, self.kt, self.g.n
        if g.family == "wire":
            kt.frames_crypt_dev(dec, self.R.fmt, n, self.d_slots.ptr, d_in, self.d_off.ptr, d_out, d_auth=d_auth)
        elif g.family == "wirex":
            kt.frames_crypt_x_dev(dec, self.R.fmt, n, self.d_slots.ptr, self.d_num.ptr, d_in, self.d_off.ptr, d_out, d_auth=d_auth)
        elif g.family == "tls":
            kt.records_crypt_dev(dec, self.R.fmt, n, self.d_slots.ptr, self.d_num.ptr, d_in, self.d_off.ptr, d_out, d_auth=d_auth)
        elif g.family == "dtls":
            self.pn_out = Guarded(self.hip, 8 * n) if dec and self.d13 else None
            kw = dict(d_sn_slots=self.d_hps.ptr, d_seq=(self.d_exp if dec else self.d_num).ptr, d_sn_off=self.d_pn_off.ptr,
                      d_seq_out=self.pn_out.ptr if dec else None) if self.d13 else {}
            kt.dtls_crypt_dev(dec, self.R.fmt, n, self.d_slots.ptr, d_in, self.d_off.ptr, d_out, d_auth=d_auth, **kw)
        elif g.family == "srtp":
            kt.srtp_crypt_dev(dec, self.R.fmt, n, self.d_slots.ptr, d_in, self.d_off.ptr, d_out, d_roc=None if g.rtcp else self.d_num.ptr, d_auth=d_auth)
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
    """every (key size, lane count) of every family kernel: 3 x 3 per kernel instantiation (direction is every case's); the rotating cases see every key size.  k_kt_dtls
    is instantiated per version and k_kt_srtp per kind (k_kt_dtls_sn runs under dtls13 alone): there each FULL mode has its own 3 x 3"""
    every = {(l, k) for l in KG.LANES for k in KEY_LENS}
    for fam, ms in _FAMILIES.items():
        assert {(l, k) for m, l, k in CASES if m in ms and m in FULL} == every, fam
        assert {k for m, l, k in ORDERED if m in ms} == set(KEY_LENS), fam
        if fam in PER_MODE:
            assert [m for m in ms if m in FULL] and all({(l, k) for mm, l, k in CASES if mm == m} == every for m in ms if m in FULL), fam
    assert {m for f in PER_MODE for m in _FAMILIES[f] if m in FULL} == {"dtls13", "dtls12", "srtp", "srtcp"}
    assert len(CASES) == len(set(CASES)) == 9 * len(FULL) + 3 * len(ONE_KEY) and len(ORDERED) == len(set(ORDERED)) == 2 * len(KG.MODES) + 1
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
