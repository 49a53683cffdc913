"""CPU: key tables (aesgcm_keytab_*) without a GPU.  Builds the gfx950 assembly of the key tables' kernels (`make -C csrc asm_keytab`) and reads it with
tools/isa_census.py -- 18 k_kt_batch instances (3 key sizes x encrypt / decrypt x 8, 16, 64 lanes per packet), none with scratch, none above the 128 registers
of their 1024-lane workgroups -- and checks that the entry points refuse to run (no CPU fallback) where there is no device."""
import os

import pytest

import aesgcm_amd  # noqa: F401
from aesgcm_amd import lib

from kt_common import asm_census, assert_in_budget


@pytest.fixture(scope="module")
def census():
    return asm_census("keytab")


def test_keytab_kernel_set(census):
    fam = {}
    for name in census:
        fam.setdefault(name.split("<")[0], []).append(name)
    assert sorted(fam) == ["k_kt_batch", "k_kt_setup"], sorted(fam)
    want = {"k_kt_batch<%d, %d, %d>" % (nr, dec, lg) for nr in (10, 12, 14) for dec in (0, 1) for lg in (3, 4, 6)}
    assert set(fam["k_kt_batch"]) == want
    assert len(fam["k_kt_setup"]) == 3


def test_keytab_kernels_scratch_free_and_in_budget(census):
    assert_in_budget(census, body="k_kt_batch<")


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
