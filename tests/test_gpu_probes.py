"""GPU: the ceiling probes' launch paths -- k_body<NR, MODE_PROBE>, k_pktl<NR, 2, 0> / k_pktg<NR, 2, LG> and k_batch3<NR, 2, 3> -- which only bench.py and the fake
runtime reached.  A probe runs a kernel's instruction stream without the data's loads and stores, so there is no output to compare: each call must return OK and the
device must synchronise without error; after the probes the same context still encrypts correctly.  The shape the device chose for each frames call is printed.
The batch probe runs twice: at a count where the library's own rule takes 8 lanes per packet, and at 4096 x 256 B with that shape forced (the debug build)."""
import numpy as np
import pytest

from util import splitmix_bytes

pytestmark = pytest.mark.gpu


def _batch_probe(hip, n, key_bytes, pkt):
    d_keys, d_ivs, d_tags = hip.DeviceBuffer(key_bytes * n), hip.DeviceBuffer(12 * n + 16), hip.DeviceBuffer(16 * n)
    d_keys.upload(splitmix_bytes(0x4B4559, key_bytes * n))
    d_ivs.upload(splitmix_bytes(0x4956, 12 * n))
    hip.batch_ceiling_probe_dev(n, key_bytes, d_keys.ptr, d_ivs.ptr, pkt, d_tags.ptr)
    hip.dev_sync(0)
    for b in (d_keys, d_ivs, d_tags):
        b.free()


@pytest.mark.parametrize("key_bytes", [16, 24, 32])
def test_probes_run_and_leave_the_context_sound(hip, orc, key_bytes):
    key = splitmix_bytes(0x50524F42 + key_bytes, key_bytes)
    with hip.Context(key) as ctx:
        ms, blocks = ctx.ceiling_probe(1 << 20)                               # k_body's dealt chunks in PROBE mode
        assert ms > 0 and 0 < blocks <= (1 << 20) // 16
        hip.dev_sync(0)
        for n in (64, 4096, 65536):                                           # the packet kernels' probes, in the shape the device picks for the count
            lens = np.uint64(64) + np.frombuffer(splitmix_bytes(0x4C454E + n, 8 * n), dtype="<u8") % np.uint64(1437)
            assert lens.min() >= 64 and lens.max() <= 1500
            doff = np.zeros(n + 1, dtype=np.uint64)
            doff[1:] = np.cumsum(lens)
            d_ivs, d_doff, d_tags = hip.DeviceBuffer(12 * n + 16), hip.DeviceBuffer(8 * (n + 1)), hip.DeviceBuffer(16 * n)
            d_ivs.upload(splitmix_bytes(0x4956 + n, 12 * n))
            d_doff.upload(doff.tobytes())
            ctx.frames_ceiling_probe_dev(n, d_ivs.ptr, d_doff.ptr, d_tags.ptr)
            hip.dev_sync(0)
            assert ctx.status() == (hip.STATUS_OK, 0)
            print("frames probe: key %d bits, %d frames -> %r" % (8 * key_bytes, n, ctx.last_route()))
            for b in (d_ivs, d_doff, d_tags):
                b.free()
        # per-packet keys: the batch probe exists in the 8-lanes-per-packet shape alone.  The library's own rule (batch_pick_lg) gives 256-byte packets 8 lanes from
        # 64 packets per CU, so 65536 of them take it on any chip of up to 1024 CUs; 4096 take 16 lanes on a chip of more than 64 CUs and reach the probe's 8-lane
        # instance only with the shape forced through the debug build.
        pkt = 256
        assert hip.batch_shape(65536, pkt) == 8
        _batch_probe(hip, 65536, key_bytes, pkt)
        with hip.debug_library() as dbg:
            dbg.force(batch_lanes=8)
            assert hip.batch_shape(4096, pkt) == 8
            _batch_probe(hip, 4096, key_bytes, pkt)
        iv, aad, pt = splitmix_bytes(1, 12), splitmix_bytes(2, 20), splitmix_bytes(3, 4096)
        assert ctx.encrypt(iv, aad, pt) == orc.Fast(key).encrypt(iv, aad, pt)
