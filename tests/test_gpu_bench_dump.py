"""GPU: `bench.py --dump-outputs DIR` writes what the timed path computed in its last step -- a fixed, seeded sample of the
ciphertext with its byte offsets and the tag -- and a plain run (no --full) prints the headline line without the passes of
its own (`roofline`, `cpu_baseline`).  The dumped bytes are checked against the CPU oracle over the same SplitMix64 stream."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_bench_dumps_the_last_steps_outputs(hip, orc, tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
    n = 16 << 20                                                        # 16 MiB: more than the dump's 8 MiB, so it is sampled
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gib-per-gpu", str(n / (1 << 30)), "--steps", "5", "--warmup", "1",
                        "--dump-outputs", str(tmp_path)], env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    line = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["steps"] == 5 and line["ms_per_step"] > 0 and line["unit"] == "GiB/s" and line["higher_is_better"] is True
    assert "roofline" not in line and "cpu_baseline" not in line
    ct = np.load(tmp_path / "ciphertext.npy")
    off = np.load(tmp_path / "ciphertext_offsets.npy")
    tags = np.load(tmp_path / "tags.npy")
    assert ct.dtype == np.float32 and off.dtype == np.float64 and tags.dtype == np.float32
    assert ct.ndim == 2 and ct.shape == (len(off), 4096) and tags.shape == (1, 16)
    assert off[0] == 0 and off[-1] == n - 4096 and np.all(np.diff(off) > 0)
    import aesgcm_amd  # noqa: F401
    from aesgcm_amd import sharding
    key, iv = sharding.splitmix64_bytes(0x4B4559, 32), sharding.splitmix64_bytes(0x4956, 12)
    pt = np.frombuffer(orc.fill_splitmix64(n, 0xAE5C0003), dtype=np.uint8)
    want = np.empty_like(pt)
    _, want_tag = orc.Fast(key).crypt(False, iv, b"", pt, want)
    assert bytes(tags.astype(np.uint8).tobytes()) == want_tag and line["tags"] == [want_tag.hex()]
    rows = want.reshape(-1, 4096)[(off // 4096).astype(np.int64)]
    assert np.array_equal(ct.astype(np.uint8), rows)
