"""CPU: TLS records through key tables (aesgcm_keytab_records_crypt_dev: TLS 1.3 and TLS 1.2 AES-GCM) without a GPU.  The binding names the three entry points;
aesgcm_tls_fmt_check -- which needs no device -- accepts the two presets and refuses everything else; the crypt call refuses a NULL or bad format and a missing
d_seq before it looks at a table or a device; the gfx950 assembly of the kernels (`make -C csrc asm_tls`, read with tools/isa_census.py) holds exactly the 36
k_kt_tls instances (3 key sizes x encrypt / decrypt x 8, 16, 64 lanes per record x TLS 1.3 / 1.2), none with scratch, none above the 128 registers of their
1024-lane workgroups; and the fixture of tests/golden/tls_records.json, records of a real TLS stack, authenticates under libcrypto with keys and IVs derived here
(that pins derivation and fixture; what the GPU makes of them is tests/test_gpu_tls.py's business)."""
import ctypes
import os

import pytest

import aesgcm_amd  # noqa: F401
from aesgcm_amd import lib

from kt_common import asm_census, assert_in_budget

import tls_fixture as T
from util import GOLDEN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "aes-gcm-128-192-256-bits_amd", "csrc")


def test_tls_symbols_in_the_binding():
    for s in ("aesgcm_tls_fmt_check", "aesgcm_keytab_set_tls_iv", "aesgcm_keytab_records_crypt_dev"):
        assert s in lib.SYMBOLS
    assert ctypes.sizeof(lib.TlsFormat) == 8
    assert (lib.TLS_13, lib.TLS_12) == (1, 2)
    hdr = open(os.path.join(ROOT, "include", "aesgcm.h")).read()
    assert "#define AESGCM_TLS_13 1u" in hdr and "#define AESGCM_TLS_12 2u" in hdr
    assert "#define AESGCM_ABI_VERSION 5 " in hdr


def test_presets_pass_the_check():
    for f, want in ((lib.TlsFormat.tls13(), (1, 0)), (lib.TlsFormat.tls12(), (2, 0))):
        assert (f.version, f.reserved) == want
        assert f.check() == lib.OK, f
        assert repr(f) == "TlsFormat(version=%d, reserved=0)" % want[0]


@pytest.mark.parametrize("version, reserved", [(0, 0), (3, 0), (4, 0), (1, 1), (2, 1), (0x80000001, 0)])
def test_malformed_formats_are_refused(version, reserved):
    assert lib.TlsFormat(version, reserved).check() == lib.EARG


def test_refused_before_any_table_or_device():
    L = lib._keytab_typed(lib.load())
    assert L.aesgcm_tls_fmt_check(None) == lib.EARG
    # the crypt call runs the check before anything else: no table, no device
    assert L.aesgcm_keytab_records_crypt_dev(None, 0, None, 1, None, None, None, None, None, None, None) == lib.EARG
    for bad in (lib.TlsFormat(0, 0), lib.TlsFormat(3, 0), lib.TlsFormat(1, 1)):
        assert L.aesgcm_keytab_records_crypt_dev(None, 0, ctypes.byref(bad), 1, 16, 16, 16, 16, 16, None, None) == lib.EARG
    # d_seq NULL (every other pointer a placeholder that is never followed: there is no table)
    for f in (lib.TlsFormat.tls13(), lib.TlsFormat.tls12()):
        assert L.aesgcm_keytab_records_crypt_dev(None, 0, ctypes.byref(f), 1, 16, None, 16, 16, 16, None, None) == lib.EARG
    assert L.aesgcm_keytab_set_tls_iv(None, 0, 1, bytes(12), None) == lib.EARG


@pytest.fixture(scope="module")
def census():
    return asm_census("tls")


def test_tls_kernel_set(census):
    want = {"k_kt_tls<%d, %d, %d, %du>" % (nr, dec, lg, ver) for nr in (10, 12, 14) for dec in (0, 1) for lg in (3, 4, 6) for ver in (lib.TLS_13, lib.TLS_12)}
    assert len(want) == 36
    assert set(census) == want, sorted(census)


def test_tls_kernels_scratch_free_and_in_budget(census):
    assert_in_budget(census)


def test_tls_source_is_a_unit_of_its_own():
    """the other translation units name no k_kt_tls: their censuses stay what they were"""
    for f in ("aesgcm_wirex_kernels.hip", "aesgcm_wire_kernels.hip", "aesgcm_keytab_kernels.hip", "aesgcm_kernels.hip"):
        assert "k_kt_tls" not in open(os.path.join(CSRC, f)).read(), f
    assert '#include "aesgcm_tls_kernels.hip"' in open(os.path.join(CSRC, "aesgcm_device.hip")).read()


def test_fixture_shape():
    conns = T.golden("tls_records.json")["connections"]
    assert [(c["version"], c["suite"], c["key_len"]) for c in conns] == [
        ("1.3", "TLS_AES_128_GCM_SHA256", 16), ("1.3", "TLS_AES_256_GCM_SHA384", 32),
        ("1.2", "ECDHE-RSA-AES128-GCM-SHA256", 16), ("1.2", "ECDHE-RSA-AES256-GCM-SHA384", 32)]
    for ver in ("1.3", "1.2"):
        lens = [sorted(r["len"] for r in c["dirs"][who]["records"]) for c in conns if c["version"] == ver for who in ("client", "server")]
        assert all(x[:6] == [1, 15, 16, 17, 100, 1400] for x in lens)
        assert sorted(len(x) for x in lens) == [6, 6, 6, 7] and [x[6] for x in lens if len(x) == 7] == [16384]
    largest = max(os.path.getsize(os.path.join(GOLDEN, f)) for f in os.listdir(GOLDEN) if f != "tls_records.json")
    assert os.path.getsize(os.path.join(GOLDEN, "tls_records.json")) <= largest


def test_fixture_authenticates_under_libcrypto():
    """every recorded record, with key and IV derived from the logged secrets and nonce and AAD built by the RFCs' formulas, opens under libcrypto to the seeded
    plaintext (TLS 1.3: followed by the content type 0x17)"""
    from oracle import libcrypto_ref as R
    assert R.available()
    n = 0
    for conn, who, ver, key, iv, recs in T.directions():
        assert len(key) == conn["key_len"]
        for seq, rec, pt in recs:
            h = T.HDR[ver]
            assert rec[0] == 23 and int.from_bytes(rec[3:5], "big") == len(rec) - 5
            got, ok = R.decrypt(key, T.nonce_of(ver, iv, seq, rec), T.aad_of(ver, seq, rec), rec[h:-16], rec[-16:])
            assert ok, (conn["suite"], who, seq)
            assert bytes(got) == pt, (conn["suite"], who, seq)
            # ... and by no neighbouring sequence number
            assert not R.decrypt(key, T.nonce_of(ver, iv, seq + 1, rec), T.aad_of(ver, seq + 1, rec), rec[h:-16], rec[-16:])[1]
            n += 1
    assert n == 50
