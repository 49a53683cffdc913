"""GPU: the packet kernels on the alignment grid of tests/pkt_grid.py -- every start residue, ragged end and guard byte.

k_pktl / k_pktls (a lane per packet), k_pktg / k_pktgs (lane groups), the row kernels' per-block lanes and k_batch3's body read and write at any byte address.
What such code gets wrong is a shift for one (address & 15, length & 15) pair, a loop boundary that meets a 128-byte line, or a store that spills into the
neighbour.  Each case here runs a grid in which every such cell occurs (the generator asserts it), in arenas with 256 canary bytes in front and behind and -- in
the scattered form -- 1 .. 19 canary bytes between neighbours, and compares WHOLE arenas with arenas assembled from the CPU oracle (oracle/aesgcm_oracle.c through
orc.Fast; never another GPU path): encrypt out of place and in place, decrypt of the oracle's ciphertext with one tag in seven forged, and the same decrypt with the
failed packets wiped.  A mismatch names the first differing packet with its cell (shape, key size, direction, input residue, output residue, length).  Every
routed call asserts its status and its route, so that no case passes on another kernel than the one it names.

The same cells run through the lane code on the host in tests/host_emul/emul.cpp (test_packet_grid), under the sanitizers at level 1."""
import pytest

from grid_legs import N_KEYS, SPLIT, _fixed_records_leg, _packed_leg, _reference, _route, _scattered_leg, _up

pytestmark = pytest.mark.gpu

#        forced shape (debug library) or None, lanes of the grid's group edges, lanes last_route reports: packed / scattered (None: the device's choice, 0: by rows)
SHAPES = {
    "lane": (dict(pkt_lanes=1, pkt_ilp=2), 0, 1, 1),
    "lane_ilp": (dict(pkt_lanes=1, pkt_ilp=1), 0, 1, 1),
    "g4": (dict(pkt_lanes=4), 4, 4, 4),
    "g8": (dict(pkt_lanes=8), 8, 8, 8),
    "group16": (dict(pkt_lanes=16), 16, 16, 16),
    "wave": (dict(pkt_lanes=64), 64, 64, 16),                    # (messages wherever they live have no wave-per-packet kernel: 16 lanes)
    "rows": (dict(pkt_rows=1), 0, 0, 0),
    "default": (None, 0, None, None),
}


# ---------------------------------------------------------------------------------------------- the cases
def _one_key_case(hip, orc, shape, klen):
    force, G, lanes_p, lanes_s = SHAPES[shape]
    name = "%s AES-%d" % (shape, 8 * klen)
    R = _reference(orc, "packed", G, klen)
    S, SI = _reference(orc, "scattered", min(G, 16), klen), _reference(orc, "inplace", 0, klen)
    d_ivs, d_aad, d_doff, d_aoff = _up(hip, R.ivs), _up(hip, R.aad_arena), _up(hip, R.grid.doff.tobytes()), _up(hip, R.grid.aoff.tobytes())
    ctx = hip.Context(R.keys[0])
    if force is None:
        for k, v in SPLIT.items():
            ctx.set_option(k, v)

    def crypt(dec, d_in, d_out, d_tags, d_exp, d_auth):
        ctx.packets_crypt_dev(dec, R.n, d_ivs.ptr, d_in, d_out, d_tags, d_data_off=d_doff.ptr, d_aad=d_aad.ptr, d_aad_off=d_aoff.ptr, d_expect_tags=d_exp, d_auth=d_auth)

    def wipe(on, d_out, d_auth):
        if d_out is None:
            ctx.set_option("wipe_on_auth_fail", int(on))          # the context's own wipe behind the decrypt

    _packed_leg(hip, R, d_aad, crypt, lambda lab: _route(hip, ctx, R.n, lanes_p, lab), wipe, name)
    assert S.keys == SI.keys == R.keys
    _scattered_leg(hip, ctx, S, SI, lanes_s, name)
    if shape == "lane_ilp":
        _fixed_records_leg(hip, orc, ctx, klen, R.keys[0], name)
    ctx.close()


@pytest.mark.parametrize("klen", [16, 24, 32])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_one_key_packet_kernels_on_the_alignment_grid(hip, orc, shape, klen):
    """aesgcm_packets_crypt_dev (offset arrays) and aesgcm_messages_crypt_dev through every packet kernel shape, by rows, and by the product library's own choice"""
    if SHAPES[shape][0] is None:
        _one_key_case(hip, orc, shape, klen)
        return
    with hip.debug_library() as dbg:
        dbg.force(**SHAPES[shape][0])
        _one_key_case(hip, orc, shape, klen)


@pytest.mark.parametrize("klen", [16, 24, 32])
@pytest.mark.parametrize("lanes", [8, 16, 64])
def test_per_packet_key_batch_on_the_alignment_grid(hip, orc, lanes, klen):
    """aesgcm_batch_crypt_var_dev: the packed grid with a key per packet through k_batch3's body (aesgcm_batch3_body.inc, which the key tables share) at 8, 16 and 64
    lanes per packet, aesgcm_wipe_failed_dev behind the decrypts"""
    name = "batch%d AES-%d" % (lanes, 8 * klen)
    R = _reference(orc, "packed", lanes, klen, per_packet_keys=True)
    keys = b"".join(R.keys[i % N_KEYS] for i in range(R.n))
    with hip.debug_library() as dbg:
        dbg.force(batch_lanes=lanes)
        d_keys, d_ivs, d_aad, d_doff, d_aoff = _up(hip, keys), _up(hip, R.ivs), _up(hip, R.aad_arena), _up(hip, R.grid.doff.tobytes()), _up(hip, R.grid.aoff.tobytes())
        assert hip.batch_shape(R.n, 0, True) == lanes

        def crypt(dec, d_in, d_out, d_tags, d_exp, d_auth):
            hip.batch_crypt_var_dev(dec, R.n, klen, d_keys.ptr, d_ivs.ptr, d_in, d_doff.ptr, d_out, d_tags, d_aad=d_aad.ptr, d_aad_off=d_aoff.ptr, d_expect_tags=d_exp, d_auth=d_auth)

        def wipe(on, d_out, d_auth):
            if on and d_out is not None:
                hip.wipe_failed_dev(R.n, d_out, d_auth, d_data_off=d_doff.ptr)

        def route(lab):
            hip.dev_sync()
            return {"lanes": lanes}

        _packed_leg(hip, R, d_aad, crypt, route, wipe, name)
