"""CPU: wire frames with 64-bit numbers (aesgcm_keytab_frames_crypt_x_dev: MACsec XPN, ESP with extended sequence numbers) without a GPU.  The binding names the
three entry points; aesgcm_wire_xfmt_check -- which needs no device -- accepts the presets and refuses every malformed extension, a malformed base format inside a
well-formed extension included; the crypt call refuses a NULL or bad format and a missing d_hi before it looks at a table or a device; and the gfx950 assembly of the
kernels (`make -C csrc asm_wirex`, read with tools/isa_census.py) holds exactly the 36 k_kt_wirex instances (3 key sizes x encrypt / decrypt x 8, 16, 64 lanes per
frame x XPN / ESN: the mode is a template argument), none with scratch, none above the 128 registers of their 1024-lane workgroups."""
import ctypes
import os

import pytest

import aesgcm_amd  # noqa: F401
from aesgcm_amd import lib

from kt_common import asm_census, assert_in_budget

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "aes-gcm-128-192-256-bits_amd", "csrc")


def test_wirex_symbols_in_the_binding():
    for s in ("aesgcm_wire_xfmt_check", "aesgcm_keytab_set_xpn", "aesgcm_keytab_frames_crypt_x_dev"):
        assert s in lib.SYMBOLS
    assert ctypes.sizeof(lib.WireFormatX) == 32
    assert ctypes.sizeof(lib.WireFormat) == 24
    assert (lib.WIREX_XPN, lib.WIREX_ESN) == (1, 2)
    hdr = open(os.path.join(ROOT, "include", "aesgcm.h")).read()
    assert "#define AESGCM_WIREX_XPN 1u" in hdr and "#define AESGCM_WIREX_ESN 2u" in hdr


def _xfmt(fields, ext, reserved=0):
    return lib.WireFormatX(lib.WireFormat(*fields), ext, reserved)


def _flat(x):
    return tuple(getattr(x.f, n) for n, _ in x.f._fields_) + (x.ext, x.reserved)


def test_presets_pass_the_check():
    presets = [
        (lib.WireFormatX.macsec_xpn(), (28, 28, 16, 8, 16, 0, 1, 0)),
        (lib.WireFormatX.macsec_xpn(sci=False), (20, 20, 16, 8, 16, 0, 1, 0)),
        (lib.WireFormatX.macsec_xpn(sci=False, auth_only=True), (20, 20, 16, 8, 16, 1, 1, 0)),
        (lib.WireFormatX.macsec_xpn(sci=True, auth_only=True), (28, 28, 16, 8, 16, 1, 1, 0)),
        (lib.WireFormatX.esp_esn(), (8, 16, 8, 4, 16, 0, 2, 0)),
        (lib.WireFormatX.esp_esn(tag_len=12), (8, 16, 8, 4, 12, 0, 2, 0)),
        (lib.WireFormatX.esp_esn(tag_len=8), (8, 16, 8, 4, 8, 0, 2, 0)),
    ]
    for x, want in presets:
        assert _flat(x) == want, x
        assert x.check() == lib.OK, x
    # ext 0: every base format the base check takes
    for f in (lib.WireFormat.macsec(), lib.WireFormat.esp(12), lib.WireFormat(0, 12, 0, 0, 16, 0)):
        assert lib.WireFormatX(f, 0, 0).check() == lib.OK
    # XPN with a confidentiality offset (authenticated header of 28 + 30 bytes); ESN with a longer pass-through header
    assert _xfmt((58, 58, 16, 8, 16, 0), lib.WIREX_XPN).check() == lib.OK
    assert _xfmt((8, 20, 8, 4, 12, 0), lib.WIREX_ESN).check() == lib.OK


@pytest.mark.parametrize("name, fields, ext, reserved", [
    ("reserved set", (28, 28, 16, 8, 16, 0), 1, 1),
    ("reserved set, ext 0", (28, 28, 16, 8, 16, 0), 0, 7),
    ("unknown bit", (28, 28, 16, 8, 16, 0), 4, 0),
    ("unknown bit beside XPN", (28, 28, 16, 8, 16, 0), 0x80000001, 0),
    ("unknown bit beside ESN", (8, 16, 8, 4, 16, 0), 6, 0),
    ("both bits", (28, 28, 16, 8, 16, 0), 3, 0),
    ("both bits on an ESP format", (8, 16, 8, 4, 16, 0), 3, 0),
    ("XPN, salt_len 4", (8, 16, 8, 4, 16, 0), 1, 0),
    ("XPN, salt_len 0", (0, 12, 0, 0, 16, 0), 1, 0),
    ("ESN, aad_len 28", (28, 28, 16, 8, 16, 0), 2, 0),
    ("ESN, aad_len 12", (12, 16, 8, 4, 16, 0), 2, 0),
    ("ESN, aad_len 0", (0, 16, 8, 4, 16, 0), 2, 0),
    ("ESN, auth-only", (8, 16, 8, 4, 16, 1), 2, 0),
    # a malformed base format inside a well-formed extension
    ("XPN, base tag_len 10", (28, 28, 16, 8, 10, 0), 1, 0),
    ("XPN, base salt_len 12", (28, 28, 16, 12, 16, 0), 1, 0),
    ("XPN, base flag 2", (28, 28, 16, 8, 16, 2), 1, 0),
    ("ESN, base nonce bytes past hdr_len", (8, 12, 8, 4, 16, 0), 2, 0),
    ("ESN, base hdr_len < aad_len", (8, 4, 0, 8, 16, 0), 2, 0),
    ("ext 0, base tag_len 4", (28, 28, 16, 8, 4, 0), 0, 0),
])
def test_malformed_extensions_are_refused(name, fields, ext, reserved):
    assert _xfmt(fields, ext, reserved).check() == lib.EARG, name


def test_refused_before_any_table_or_device():
    L = lib._keytab_typed(lib.load())
    assert L.aesgcm_wire_xfmt_check(None) == lib.EARG
    # the crypt call runs the check before anything else: no table, no device
    assert L.aesgcm_keytab_frames_crypt_x_dev(None, 0, None, 1, None, None, None, None, None, None, None) == lib.EARG
    bad = _xfmt((28, 28, 16, 8, 16, 0), 3)
    assert L.aesgcm_keytab_frames_crypt_x_dev(None, 0, ctypes.byref(bad), 1, None, None, None, None, None, None, None) == lib.EARG
    badbase = _xfmt((28, 28, 16, 8, 10, 0), 1)
    assert L.aesgcm_keytab_frames_crypt_x_dev(None, 0, ctypes.byref(badbase), 1, None, None, None, None, None, None, None) == lib.EARG
    # ext != 0 and d_hi NULL (every other pointer a placeholder that is never followed: there is no table)
    for x in (lib.WireFormatX.macsec_xpn(), lib.WireFormatX.esp_esn()):
        assert L.aesgcm_keytab_frames_crypt_x_dev(None, 0, ctypes.byref(x), 1, 16, None, 16, 16, 16, None, None) == lib.EARG
    assert L.aesgcm_keytab_set_xpn(None, 0, 1, bytes(12), bytes(4), None) == lib.EARG


@pytest.fixture(scope="module")
def census():
    return asm_census("wirex")


def test_wirex_kernel_set(census):
    want = {"k_kt_wirex<%d, %d, %d, %du>" % (nr, dec, lg, ext) for nr in (10, 12, 14) for dec in (0, 1) for lg in (3, 4, 6) for ext in (lib.WIREX_XPN, lib.WIREX_ESN)}
    assert len(want) == 36
    assert set(census) == want, sorted(census)


def test_wirex_kernels_scratch_free_and_in_budget(census):
    assert_in_budget(census)


def test_wirex_source_is_a_unit_of_its_own():
    """the key tables' and k_kt_wire's translation units name no k_kt_wirex: their censuses (tests/test_wire_cpu.py) stay what they were"""
    for f in ("aesgcm_wire_kernels.hip", "aesgcm_keytab_kernels.hip", "aesgcm_kernels.hip"):
        assert "k_kt_wirex" not in open(os.path.join(CSRC, f)).read(), f
    assert '#include "aesgcm_wirex_kernels.hip"' in open(os.path.join(CSRC, "aesgcm_device.hip")).read()
