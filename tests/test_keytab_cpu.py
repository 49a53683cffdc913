"""CPU: key tables (aesgcm_keytab_*) without a GPU.  Builds the gfx950 assembly of the key tables' kernels (`make -C csrc asm_keytab`) and reads it with
tools/isa_census.py -- 18 k_kt_batch instances (3 key sizes x encrypt / decrypt x 8, 16, 64 lanes per packet), none with scratch, none above the 128 registers
of their 1024-lane workgroups -- and checks that the entry points refuse to run (no CPU fallback) where there is no device."""
import os
import subprocess
import sys

import pytest

import aesgcm_amd  # noqa: F401
from aesgcm_amd import lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
CSRC = os.path.join(ROOT, "aes-gcm-128-192-256-bits_amd", "csrc")


@pytest.fixture(scope="module")
def census():
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    subprocess.run(["make", "-C", CSRC, "-s", "asm_keytab"], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    import isa_census
    return isa_census.census(os.path.join(CSRC, "aesgcm_keytab.gfx950.s"))


def test_keytab_kernel_set(census):
    fam = {}
    for name in census:
        fam.setdefault(name.split("<")[0], []).append(name)
    assert sorted(fam) == ["k_kt_batch", "k_kt_setup"], sorted(fam)
    want = {"k_kt_batch<%d, %d, %d>" % (nr, dec, lg) for nr in (10, 12, 14) for dec in (0, 1) for lg in (3, 4, 6)}
    assert set(fam["k_kt_batch"]) == want
    assert len(fam["k_kt_setup"]) == 3


def test_keytab_kernels_scratch_free_and_in_budget(census):
    for name, k in census.items():
        assert k["scratch"] == 0, (name, k["scratch"])
        assert k["vgpr"] <= 128, (name, k["vgpr"])
        if name.startswith("k_kt_batch<"):
            depths = [d for d, ops in k["depth"].items() if ops.get("ds_read", 0) >= 16]
            assert depths, name
            assert all(k["depth"][d].get("scratch", 0) == 0 for d in depths), (name, k["depth"])


def test_keytab_symbols_in_the_binding():
    for s in ("aesgcm_keytab_create", "aesgcm_keytab_set", "aesgcm_keytab_set_dev", "aesgcm_keytab_clear", "aesgcm_keytab_crypt_dev",
              "aesgcm_keytab_status", "aesgcm_keytab_destroy"):
        assert s in lib.SYMBOLS


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="a GPU is present")
def test_keytab_create_fails_loudly_without_gpu():
    with pytest.raises(lib.AesGcmError) as e:
        lib.KeyTable(16, 8)
    assert e.value.code == lib.EHIP


def test_keytab_create_refuses_bad_arguments():
    """argument checks come before the device is touched: AESGCM_EARG with or without a GPU"""
    for key_len, n in ((15, 8), (16, 0), (33, 8)):
        with pytest.raises(lib.AesGcmError) as e:
            lib.KeyTable(key_len, n)
        assert e.value.code == lib.EARG, (key_len, n)
