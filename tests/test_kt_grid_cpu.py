"""CPU: the key-table family's alignment grid (tests/kt_grid.py) -- every mode's grid is complete (the generator asserts every required cell itself) and
deterministic; and for one mode per family the reference arena that tests/test_gpu_kt_grid.py holds the GPU to (kt_common.grid_reference: libcrypto through
oracle/evp_batch.c with nonce and AAD by the family's formulas, QUIC through tests/quic_fixture.py, DTLS through tests/dtls_fixture.py, SRTP and SRTCP through
tests/srtp_fixture.py) opens again on the CPU under the same formulas: the plaintext back, every tag accepted, every forged tag refused.  The expected bytes are
self-consistent before any GPU sees them.  The two formats that no published vector pins (DTLS 1.3, SRTCP with E clear) are opened by formulas written out here."""
import pytest

import aesgcm_amd  # noqa: F401
from aesgcm_amd import lib
from oracle import libcrypto_ref as R

import dtls_fixture as D
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


def _xor(a, b):
    return bytes(x ^ y for x, y in zip(a, b))


@pytest.mark.parametrize("mode, key_len", [("macsec", 16), ("esn16", 24), ("tls12", 32), ("quic", 24), ("dtls13", 16), ("srtp_mki", 32), ("srtcp_clear", 24)])
def test_the_reference_opens_again_on_the_cpu(evp, mode, key_len):  # noqa: F811
    """DTLS 1.3 and SRTCP with E clear have no published vector, so their frames are opened by oracle.libcrypto_ref.decrypt with nonce and AAD written out here from the
    RFCs' text, not through tests/dtls_fixture.py or tests/srtp_fixture.py, which made them: the grid's expected bytes do not rest on the fixtures alone"""
    ref = KC.grid_reference(lib, evp, mode, key_len)
    g = ref.g
    plain, enc, bad, dec = g.frames(), g.frames(ref.enc), g.frames(ref.dec_in), g.frames(ref.dec_out)
    forged = set(g.forged)
    assert ref.auth == [0 if i in forged else 1 for i in range(g.n)]
    for arena in (ref.enc, ref.dec_in, ref.dec_out):           # nothing outside the frames differs from the plaintext arena
        assert (arena[:PG.GUARD] == PG.CANARY_IN).all() and (arena[int(g.off[-1]):] == PG.CANARY_IN).all() and arena.size == g.size
    for i in range(g.n):
        key = ref.keys[key_len * g.slots[i]:key_len * (g.slots[i] + 1)]
        h, t = g.fronts[i], g.tag_at(i)                         # where the payload and the tag start (the tag is 16 bytes in every mode here)
        for frame, good in ((enc[i], True),) + (((bad[i], False),) if i in forged else ()):
            if g.family == "quic":
                back, pn, ok = Q.unprotect(key, ref.ivs[g.slots[i]], ref.key(g.hps[i]), g.expected_pns[i], g.pn_off[i], frame)
                assert ok == good and (not good or (pn == g.nums[i] and back == plain[i][:-16] + frame[-16:])), (mode, g.cell(i))
                continue
            front = frame[:h]
            if g.family == "wire":
                nonce, aad, ct = KC.wire_split(ref.fmt, ref.salts[g.slots[i]], frame)
            elif g.family == "wirex":
                nonce, aad, ct = KC.x_split(ref.fmt, ref.sa, g.slots[i], g.nums[i], frame)
            elif g.family == "tls":
                ver = ref.fmt.version
                nonce, aad, ct = T.nonce_of(ver, ref.ivs[g.slots[i]], g.nums[i], frame), T.aad_of(ver, g.nums[i], frame), frame[g.fronts[i]:-16]
            elif mode == "dtls13":
                # RFC 9147 4: nonce = the IV XOR the 64-bit record sequence number, padded on the left; AAD = the header as it was before its sequence bytes were
                # masked; 4.2.3: the mask = AES-ECB under the sn key of the first 16 bytes of ciphertext (the tag's bytes where the payload is shorter), XORed on
                # the 1 or 2 sequence bytes
                nonce = _xor(ref.ivs[g.slots[i]], bytes(4) + g.nums[i].to_bytes(8, "big"))
                so, sl = g.sn_off[i], 2 if g.s16[i] else 1
                mask = Q.aes_ecb(ref.key(g.hps[i]), enc[i][h:h + 16])
                front = frame[:so] + _xor(frame[so:so + sl], mask) + frame[so + sl:h]
                aad, ct = front, frame[h:t]
                assert len(enc[i][h:h + 16]) == 16 and front[so:so + sl] == (g.nums[i] & (0xFFFF if g.s16[i] else 0xFF)).to_bytes(sl, "big")
            elif mode == "srtp_mki":
                # RFC 7714 8.1: salt XOR (00 00 | SSRC | ROC | SEQ); 8.2: AAD = the RTP header
                nonce = _xor(ref.ivs[g.slots[i]], bytes(2) + frame[8:12] + g.nums[i].to_bytes(4, "big") + frame[2:4])
                aad, ct = frame[:h], frame[h:t]
                assert frame[t + 16:] == plain[i][t + 16:] and len(frame) - t - 16 == 4                  # the MKI passes through
            else:
                # RFC 7714 9.1: salt XOR (00 00 | SSRC | 00 00 | 0, the 31-bit index); 9.3 with E clear: AAD = the packet's bytes in front of the tag | W, nothing encrypted
                w = frame[t + 16:t + 20]
                assert mode == "srtcp_clear" and w[0] < 0x80 and int.from_bytes(w, "big") == g.index[i]
                nonce = _xor(ref.ivs[g.slots[i]], bytes(2) + frame[4:8] + bytes(2) + w)
                aad, ct = frame[:t] + w, b""
                assert frame[:t] == plain[i][:t] and frame[t + 16:] == plain[i][t + 16:] and len(frame) - t - 20 == 3
            pt, ok = R.decrypt(key, nonce, aad, ct, frame[t:t + 16])
            assert bool(ok) == good and front == plain[i][:h], (mode, g.cell(i))
            assert pt == (b"" if mode == "srtcp_clear" else plain[i][h:t]), (mode, g.cell(i))
        if i not in forged:
            assert dec[i] == plain[i][:t] + enc[i][t:] and enc[i][t + 16:] == plain[i][t + 16:]
        elif g.family != "quic":
            assert bad[i][:t] == enc[i][:t] and bad[i][t + 16:] == enc[i][t + 16:] and bad[i] != enc[i] and dec[i][t:] == bad[i][t:]
            if mode != "dtls13" or g.lens[i] >= 16:            # (a shorter DTLS 1.3 payload has the forged tag in its sample: another mask, another number)
                assert dec[i] == plain[i][:t] + bad[i][t:]
        if mode == "dtls13":
            assert ref.pn_out[i] == g.nums[i] or (i in forged and g.lens[i] < 16), g.cell(i)
            if i not in forged:                                # the fixture's receiver finds the number from the expected one
                assert D.unprotect13(key, ref.ivs[g.slots[i]], ref.key(g.hps[i]), g.expected_seqs[i], g.sn_off[i], enc[i]) == (dec[i], g.nums[i], True)
    if mode == "dtls13":                                       # the forged tags did reach a sample, and changed a mask
        assert any(dec[i][:g.fronts[i]] != plain[i][:g.fronts[i]] for i in forged) and any(ref.pn_out[i] != g.nums[i] for i in forged)


def test_a_byte_is_named_by_its_part_of_the_frame():
    """Grid.part / Grid.where, which the GPU test's failure message uses: srtcp_clear frames are hdr[8] | body | tag[16] | W[4] | mki[3]"""
    g = KG.grid("srtcp_clear")
    i = next(i for i in range(1, g.n) if g.lens[i] == 5)
    assert g.flen[i] == 8 + 5 + 16 + 7 and g.tag_at(i) == 13 and g.trail[i] == 7
    assert [g.part(i, o) for o in (0, 7, 8, 12, 13, 28, 29, 35)] == ["front", "front", "payload", "payload", "tag", "tag", "trailer", "trailer"]
    assert g.where(g.at[i] + 28) == (i, 28, "tag") and g.where(g.at[i] + 29 + 5, shift=5) == (i, 29, "trailer") and g.where(g.at[i] + 36) == (i + 1, 0, "front")
    assert g.where(PG.GUARD - 1) == (0, None, "guard") and g.where(int(g.off[-1])) == (g.n, None, "guard") and g.where(int(g.off[-1]) - 1) == (g.n - 1, g.flen[-1] - 1, "trailer")
    z = next(i for i in range(g.n) if g.lens[i] == 0)          # no body: the tag follows the header
    assert [g.part(z, o) for o in (7, 8, 23, 24)] == ["front", "tag", "tag", "trailer"]
    m = KG.grid("macsec")                                      # the tag is last where there is no trailer
    assert m.part(0, m.flen[0] - 1) == "tag" and m.part(0, m.flen[0] - 17) in ("payload", "front") and m.trail[0] == 0
    with pytest.raises(AssertionError):
        g.part(i, g.flen[i])
