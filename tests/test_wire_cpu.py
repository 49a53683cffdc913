"""CPU: key tables on frames in wire format (aesgcm_keytab_frames_crypt_dev) without a GPU.  The binding names the three entry points; aesgcm_wire_fmt_check -- which
needs no device -- accepts every documented format and refuses every malformed one; and the gfx950 assembly of the wire kernels (`make -C csrc asm_wire`, read
with tools/isa_census.py) holds exactly the 18 k_kt_wire instances (3 key sizes x encrypt / decrypt x 8, 16, 64 lanes per frame), none with scratch, none above the
128 registers of their 1024-lane workgroups."""
import ctypes

import pytest

import aesgcm_amd  # noqa: F401
from aesgcm_amd import lib

from kt_common import asm_census, assert_in_budget


def test_wire_symbols_in_the_binding():
    for s in ("aesgcm_wire_fmt_check", "aesgcm_keytab_set_salt", "aesgcm_keytab_frames_crypt_dev"):
        assert s in lib.SYMBOLS
    assert lib.ABI_VERSION == 5


def _fmt(aad_len, hdr_len, iv_off, salt_len, tag_len, flags):
    return lib.WireFormat(aad_len, hdr_len, iv_off, salt_len, tag_len, flags)


def test_documented_formats_pass_the_check():
    presets = [
        (lib.WireFormat.macsec(), (28, 28, 16, 8, 16, 0)),
        (lib.WireFormat.macsec(sci=False), (20, 20, 16, 8, 16, 0)),
        (lib.WireFormat.macsec(sci=False, auth_only=True), (20, 20, 16, 8, 16, 1)),
        (lib.WireFormat.macsec(sci=True, auth_only=True), (28, 28, 16, 8, 16, 1)),
        (lib.WireFormat.esp(), (8, 16, 8, 4, 16, 0)),
        (lib.WireFormat.esp(tag_len=12), (8, 16, 8, 4, 12, 0)),
        (lib.WireFormat.esp(tag_len=8), (8, 16, 8, 4, 8, 0)),
    ]
    for f, want in presets:
        assert tuple(getattr(f, n) for n, _ in f._fields_) == want, f
        assert f.check() == lib.OK, f
    assert ctypes.sizeof(lib.WireFormat) == 24
    assert _fmt(0, 12, 0, 0, 16, 0).check() == lib.OK                     # the whole nonce in the frame, nothing authenticated but the payload
    assert _fmt(0, 65535, 65523, 0, 8, 0).check() == lib.OK               # the longest header, the nonce at its very end
    assert _fmt(40, 20, 16, 8, 16, lib.WIRE_AUTH_ONLY).check() == lib.OK  # auth-only: aad_len is ignored


@pytest.mark.parametrize("name, fields", [
    ("salt_len 2", (28, 28, 16, 2, 16, 0)),
    ("salt_len 12", (28, 28, 16, 12, 16, 0)),
    ("tag_len 0", (28, 28, 16, 8, 0, 0)),
    ("tag_len 4", (28, 28, 16, 8, 4, 0)),
    ("tag_len 10", (28, 28, 16, 8, 10, 0)),
    ("tag_len 20", (28, 28, 16, 8, 20, 0)),
    ("hdr_len < aad_len", (28, 20, 16, 8, 16, 0)),
    ("nonce bytes past hdr_len", (28, 28, 25, 8, 16, 0)),
    ("nonce bytes past hdr_len, no salt", (16, 16, 8, 0, 16, 0)),
    ("iv_off past hdr_len", (8, 16, 17, 4, 16, 0)),
    ("iv_off wraps", (8, 16, 0xFFFFFFFC, 4, 16, 0)),
    ("unknown flag", (28, 28, 16, 8, 16, 2)),
    ("unknown flag beside a known one", (28, 28, 16, 8, 16, 0x80000001)),
    ("hdr_len 2^16", (28, 65536, 16, 8, 16, 0)),
    ("auth-only, nonce bytes past hdr_len", (20, 20, 17, 8, 16, 1)),
])
def test_malformed_formats_are_refused(name, fields):
    assert _fmt(*fields).check() == lib.EARG, name


def test_null_format_is_refused():
    L = lib._keytab_typed(lib.load())
    assert L.aesgcm_wire_fmt_check(None) == lib.EARG
    # the crypt call runs the check before anything else: a bad format is AESGCM_EARG with no table and no device
    bad = _fmt(28, 28, 16, 8, 10, 0)
    assert L.aesgcm_keytab_frames_crypt_dev(None, 0, ctypes.byref(bad), 1, None, None, None, None, None, None) == lib.EARG
    assert L.aesgcm_keytab_frames_crypt_dev(None, 0, None, 1, None, None, None, None, None, None) == lib.EARG


@pytest.fixture(scope="module")
def census():
    return asm_census("wire")


def test_wire_kernel_set(census):
    want = {"k_kt_wire<%d, %d, %d>" % (nr, dec, lg) for nr in (10, 12, 14) for dec in (0, 1) for lg in (3, 4, 6)}
    assert set(census) == want, sorted(census)


def test_wire_kernels_scratch_free_and_in_budget(census):
    assert_in_budget(census)
