"""What the key-table tests share: for the GPU tests of the family (tests/test_gpu_keytab.py, _wire, _wirex, _tls, _quic) the upload and packing helpers, the layout of
packets between guard bytes and the libcrypto handle; for their CPU counterparts (tests/test_keytab_cpu.py, ...) the census of a family's gfx950 listing and what every
kernel of the family owes it.  Helpers that differ per family (_run, _ref_encrypt, _table, _make_*) stay in the family's file."""
import os
import struct
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "aes-gcm-128-192-256-bits_amd", "csrc")

CANARY = 0xC5
TRAIL = 37


def _up(hip, data):
    b = hip.DeviceBuffer(max(len(data), 16))
    if data:
        b.upload(data)
    return b


def _u32(v):
    return struct.pack("<%dI" % len(v), *v)


def _u64(v):
    return struct.pack("<%dQ" % len(v), *v)


@pytest.fixture(scope="module")
def evp():
    from oracle import cpu_baseline
    return cpu_baseline.evp_batch_lib()


def _layout(pkts, lead, trail=TRAIL):
    off = [lead]
    for r in pkts:
        off.append(off[-1] + len(r))
    return off, bytes([CANARY]) * lead + b"".join(pkts) + bytes([CANARY]) * trail


def _collect(hip, d):
    """what a wire-format _run left in d: -> (the whole output buffer, auth or None, d)"""
    hip.dev_sync()
    out = bytes(d["out"].download(d["nbytes"]))
    auth = list(struct.unpack("<%di" % d["n"], bytes(d["auth"].download(4 * d["n"])))) if d["auth"] is not None else None
    return out, auth, d


def asm_census(family):
    """`make -C csrc asm_<family>`, then tools/isa_census.py over the listing -> {kernel: ...}; skips where there is no hipcc"""
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    subprocess.run(["make", "-C", CSRC, "-s", "asm_" + family], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_census
    return isa_census.census(os.path.join(CSRC, "aesgcm_%s.gfx950.s" % family))


def assert_in_budget(census, body="k_"):
    """every kernel: no scratch, at most the 128 registers of a 1024-lane workgroup; those that run the block loop (names starting with `body`): no scratch
    instruction at the loop depth where the AES rounds read their tables"""
    for name, k in census.items():
        assert k["scratch"] == 0, (name, k["scratch"])
        assert k["vgpr"] <= 128, (name, k["vgpr"])
        if name.startswith(body):
            depths = [d for d, ops in k["depth"].items() if ops.get("ds_read", 0) >= 16]
            assert depths, name
            assert all(k["depth"][d].get("scratch", 0) == 0 for d in depths), (name, k["depth"])
