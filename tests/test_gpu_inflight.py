"""GPU: messages in flight -- K contexts rotate, calls are enqueued with tag = NULL and each tag is collected through the pinned host
slot (aesgcm_last_tag) when its context comes round again: what `bench.py --inflight K` times.  Every tag and every ciphertext against the
oracle.  Reference counterpart: frame after frame under one key with H kept (src/gcm_gctr.vhd:142-144, tb/gcm_test.py:76-85)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from util import splitmix_bytes

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MiB = 1 << 20


@pytest.mark.parametrize("K,size", [(1, 96 * 1024 + 5), (2, MiB + 16), (4, 5 * MiB + 7), (3, 40 * 1024)])
def test_rotating_contexts_tags_one_turn_late(hip, orc, K, size):
    key = splitmix_bytes(0x1F00 + K, 32)
    ctxs = [hip.Context(key) for _ in range(K)]
    R = 6                                                                    # ring of message buffers
    d_pt, d_ct = hip.DeviceBuffer(R * (size + 16)), hip.DeviceBuffer(R * (size + 16))
    stride = (size + 15) // 16 * 16
    d_pt.fill_splitmix64(0x1F10 + K)
    pt = bytes(d_pt.download())
    ivs = [splitmix_bytes(0x1F20 + r, 12) for r in range(R)]
    f = orc.Fast(key)
    want = [f.encrypt(ivs[r], b"", pt[r * stride:r * stride + size]) for r in range(R)]
    pending, got = [None] * K, []
    for i in range(5 * R + 1):
        j, r = i % K, i % R
        if pending[j] is not None:
            got.append((pending[j], ctxs[j].last_tag()))
        ctxs[j].encrypt_dev(ivs[r], d_pt.ptr + r * stride, size, d_ct.ptr + r * stride, want_tag=False)
        pending[j] = r
    for j in range(K):
        if pending[j] is not None:
            got.append((pending[j], ctxs[j].last_tag()))
    assert len(got) == 5 * R + 1
    for r, t in got:
        assert t == want[r][1], (K, size, r)
    hip.dev_sync()
    ct = bytes(d_ct.download())
    for r in range(R):
        assert ct[r * stride:r * stride + size] == want[r][0], r
    for c in ctxs:
        c.close()


def test_last_tag_of_a_waited_call_and_of_nothing_enqueued(hip, orc):
    key = splitmix_bytes(0x1F80, 16)
    with hip.Context(key) as c:
        d = hip.DeviceBuffer(4096)
        d.fill_splitmix64(1)
        iv = splitmix_bytes(0x1F81, 12)
        t = c.encrypt_dev(iv, d.ptr, 1000, d.ptr)
        assert c.last_tag() == t                                             # the same slot, the same generation: no new work needed


def test_bench_inflight_line(hip, orc):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gib-per-gpu", str(4 / 1024), "--inflight", "2", "--ring-gib", "0.03125",
                        "--steps", "64", "--warmup", "8", "--full", "--no-cpu-baseline"], env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    line = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["tag_ok"] is True and line["tags_checked"] == 72 and line["config"]["inflight"] == 2 and line["config"]["ring"] == 8
    assert line["value"] > 0 and line["roofline"]["frac"] > 0
    # the first ring slot's tag, recomputed by the oracle from the same streams, is what the waited call of the bench derived its references from:
    # check the definition of the workload here (key / IV / plaintext streams), the bench checks queued == waited
    import aesgcm_amd  # noqa: F401
    from aesgcm_amd import sharding
    key, iv0 = sharding.splitmix64_bytes(0x4B4559, 32), sharding.splitmix64_bytes(0x4956, 12)
    n = 4 * MiB
    pt = np.frombuffer(orc.fill_splitmix64(n, 0xAE5C0003), dtype=np.uint8)
    ct = np.empty_like(pt)
    _, want = orc.Fast(key).crypt(False, iv0[:8] + (0).to_bytes(4, "big"), b"", pt, ct)
    with hip.Context(key) as c:
        d = hip.DeviceBuffer(n)
        d.fill_splitmix64(0xAE5C0003)
        assert c.encrypt_dev(iv0[:8] + (0).to_bytes(4, "big"), d.ptr, n, d.ptr) == want
