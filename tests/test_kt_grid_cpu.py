"""CPU: the key-table family's alignment grid (tests/kt_grid.py) -- every mode's grid is complete (the generator asserts every required cell itself) and
deterministic; and for one mode per family the reference arena that tests/test_gpu_kt_grid.py holds the GPU to (kt_common.grid_reference: libcrypto through
oracle/evp_batch.c with nonce and AAD by the family's formulas, QUIC through tests/quic_fixture.py) opens again on the CPU under the same formulas: the plaintext
back, every tag accepted, every forged tag refused.  The expected bytes are self-consistent before any GPU sees them."""
import pytest

import aesgcm_amd  # noqa: F401
from aesgcm_amd import lib
from oracle import libcrypto_ref as R

import kt_common as KC
import kt_grid as KG
import pkt_grid as PG
import quic_fixture as Q
import tls_fixture as T
from kt_common import evp  # noqa: F401


@pytest.mark.parametrize("mode", list(KG.MODES))
def test_every_grid_is_complete_and_deterministic(mode):
    a, b = KG.Grid(mode), KG.Grid(mode)                        # (construction runs the completeness assertions)
    assert a.lens == b.lens and a.nums == b.nums and (a.arena == b.arena).all() and (a.off == b.off).all()
    assert a.size == 2 * PG.GUARD + sum(a.flen) and (a.arena[:PG.GUARD] == PG.CANARY_IN).all() and (a.arena[-PG.GUARD:] == PG.CANARY_IN).all()
    assert len(KG.length_classes(a)) >= 8                      # the ordered launch has classes to sort
    assert a.forged[0] == 0 and a.forged[-1] == a.n - 1
    # a grid that lost a part fails
    a.lens = [L if L != 17 else 18 for L in a.lens]
    with pytest.raises(AssertionError):
        a.check()


def test_slot_edges_lie_either_side_of_a_turn():
    assert KG.slot_edges(1)[:6] == [95, 96, 97, 111, 112, 113] and 16 * 128 + 1 in KG.slot_edges(1) and 16 * 127 + 1 in KG.slot_edges(2)
    g = KG.grid("quic")
    assert {a for a, _ in g.edge_cells} == {1, 2, 3, 4} and (4, 16 * 3 - 1) in g.edge_cells


@pytest.mark.parametrize("mode, key_len", [("macsec", 16), ("esn16", 24), ("tls12", 32), ("quic", 24)])
def test_the_reference_opens_again_on_the_cpu(evp, mode, key_len):  # noqa: F811
    ref = KC.grid_reference(lib, evp, mode, key_len)
    g = ref.g
    plain, enc, bad, dec = g.frames(), g.frames(ref.enc), g.frames(ref.dec_in), g.frames(ref.dec_out)
    forged = set(g.forged)
    assert ref.auth == [0 if i in forged else 1 for i in range(g.n)]
    for arena in (ref.enc, ref.dec_in, ref.dec_out):           # nothing outside the frames differs from the plaintext arena
        assert (arena[:PG.GUARD] == PG.CANARY_IN).all() and (arena[int(g.off[-1]):] == PG.CANARY_IN).all() and arena.size == g.size
    for i in range(g.n):
        key = ref.keys[key_len * g.slots[i]:key_len * (g.slots[i] + 1)]
        for frame, good in ((enc[i], True),) + (((bad[i], False),) if i in forged else ()):
            if g.family == "quic":
                back, pn, ok = Q.unprotect(key, ref.ivs[g.slots[i]], ref.key(g.hps[i]), g.expected_pns[i], g.pn_off[i], frame)
                assert ok == good and (not good or (pn == g.nums[i] and back == plain[i][:-16] + frame[-16:])), (mode, g.cell(i))
                continue
            if g.family == "wire":
                nonce, aad, ct = KC.wire_split(ref.fmt, ref.salts[g.slots[i]], frame)
            elif g.family == "wirex":
                nonce, aad, ct = KC.x_split(ref.fmt, ref.sa, g.slots[i], g.nums[i], frame)
            else:
                ver = ref.fmt.version
                nonce, aad, ct = T.nonce_of(ver, ref.ivs[g.slots[i]], g.nums[i], frame), T.aad_of(ver, g.nums[i], frame), frame[g.fronts[i]:-16]
            pt, ok = R.decrypt(key, nonce, aad, ct, frame[-16:])
            assert bool(ok) == good and frame[:g.fronts[i]] == plain[i][:g.fronts[i]], (mode, g.cell(i))
            assert pt == plain[i][g.fronts[i]:-16], (mode, g.cell(i))
        if i not in forged:
            assert dec[i] == plain[i][:-g.tag_len] + enc[i][-g.tag_len:]
        elif g.family != "quic":
            assert dec[i] == plain[i][:-g.tag_len] + bad[i][-g.tag_len:] and bad[i][:-g.tag_len] == enc[i][:-g.tag_len] and bad[i] != enc[i]
