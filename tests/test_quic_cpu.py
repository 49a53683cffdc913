"""CPU: QUIC packets through key tables (aesgcm_keytab_quic_crypt_dev, RFC 9001 section 5) without a GPU.  The binding and the header name the entry point and the ABI
version is still 5; the call refuses its argument errors before it looks at a table or a device; tests/quic_fixture.py -- the reference tests/test_gpu_quic.py holds the
GPU to -- reproduces RFC 9001 Appendix A (Initial keys, the header-protection mask, the protected header and the whole client Initial packet) and RFC 9000 Appendix
A.3 (packet-number decoding, at wrap-around and beside 2^62); the gfx950 assembly of the kernels (`make -C csrc asm_quic`, read with tools/isa_census.py) holds exactly
the 18 k_kt_quic and 6 k_kt_quic_hp instances, none with scratch, none above 128 registers."""
import ctypes
import os

import pytest

import aesgcm_amd  # noqa: F401
from aesgcm_amd import lib

from kt_common import asm_census, assert_in_budget

import quic_fixture as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "aes-gcm-128-192-256-bits_amd", "csrc")

DCID = bytes.fromhex("8394c8f03e515708")


def test_quic_symbol_in_binding_and_header():
    assert "aesgcm_keytab_quic_crypt_dev" in lib.SYMBOLS
    hdr = open(os.path.join(ROOT, "include", "aesgcm.h")).read()
    assert "AESGCM_API int aesgcm_keytab_quic_crypt_dev(aesgcm_keytab *t, int decrypt, size_t n_pkts," in hdr
    assert "#define AESGCM_ABI_VERSION 5 " in hdr
    assert "DTLS and QUIC" not in hdr
    L = lib._keytab_typed(lib.load())
    assert L.aesgcm_abi_version() == 5
    assert len(L.aesgcm_keytab_quic_crypt_dev.argtypes) == 13
    for m in ("quic_crypt_dev", "crypt_quic"):
        assert callable(getattr(lib.KeyTable, m))


def test_argument_errors_before_any_table_or_device():
    """t = NULL and placeholder pointers that are never followed: the call returns before it touches a table or a device"""
    f = lib._keytab_typed(lib.load()).aesgcm_keytab_quic_crypt_dev
    P = 16                                                                   # a placeholder pointer

    def call(t=None, decrypt=0, n=1, slots=P, hp=P, pn=P, pn_out=P, pn_off=P, d_in=P, pkt_off=P, d_out=P, auth=P):
        return f(t, decrypt, n, slots, hp, pn, pn_out, pn_off, d_in, pkt_off, d_out, auth, None)

    assert call() == lib.EARG                                                # t NULL
    assert call(n=0) == lib.EARG                                             # ... whatever else
    for d in (2, -1, 7):
        assert call(t=P, decrypt=d) == lib.EARG                              # decrypt not 0 / 1 (checked with t: the placeholder is not followed)
    for name in ("slots", "hp", "pn", "pn_off", "d_in", "pkt_off", "d_out"):
        for d in (0, 1):
            assert call(t=P, decrypt=d, **{name: None}) == lib.EARG, name
    assert call(t=P, decrypt=1, auth=None) == lib.EARG
    assert call(t=P, decrypt=1, pn_out=None) == lib.EARG
    assert call(t=P, n=2 ** 31) == lib.EARG
    assert call(t=P, decrypt=1, n=2 ** 31 + 5) == lib.EARG
    assert call(t=P, n=0) == lib.OK                                          # nothing to do: nothing is looked at
    assert call(t=P, n=0, decrypt=1, auth=None, pn_out=None) == lib.OK


# ---------------------------------------------------------------- RFC 9001 Appendix A
def test_initial_keys_of_rfc9001_appendix_a():
    assert tuple(x.hex() for x in Q.initial_keys(DCID, "client")) == ("1f369613dd76d5467730efcbe3b1a22d", "fa044b2f42a3fd3b46fb255c", "9f50449e04a0e810283a1e9933adedd2")
    assert tuple(x.hex() for x in Q.initial_keys(DCID, "server")) == ("cf3a5331653c364c88f0f379b6067e37", "0ac1493ca1905853b0bba03e", "c206b8d9b9f0f37644430b490eeaa314")


def test_header_protection_of_rfc9001_appendix_a2():
    _, _, hp = Q.initial_keys(DCID, "client")
    mask = Q.aes_ecb(hp, bytes.fromhex("d1b1c98dd7689fb8ec11d242b123dc9b"))
    assert mask[:5].hex() == "437b9aec36"
    header = bytes.fromhex("c300000001088394c8f03e5157080000449e00000002")
    pn_off = 18
    assert len(header) == pn_off + 4 and (header[0] & 3) + 1 == 4
    assert Q.apply_mask(header, pn_off, 4, mask).hex() == "c000000001088394c8f03e5157080000449e7b9aec34"
    # ... and through hp_mask, which finds the sample itself: four bytes behind the packet-number field's start
    packet = header + bytes.fromhex("d1b1c98dd7689fb8ec11d242b123dc9b") + bytes(40)
    assert Q.hp_mask(hp, packet, pn_off) == mask


def test_protect_and_unprotect_are_inverse_and_reject():
    key, iv, hp = Q.initial_keys(DCID, "client")
    header = bytes.fromhex("c300000001088394c8f03e5157080000449e00000002")
    plain = header + bytes(range(200)) + b"\xAA" * 16
    wire = Q.protect(key, iv, hp, 2, 18, plain)
    assert wire[1:18] == header[1:18] and wire[0] & 0xF0 == 0xC0 and len(wire) == len(plain)
    back, pn, ok = Q.unprotect(key, iv, hp, 0, 18, wire)
    assert ok and pn == 2 and back[:-16] == plain[:-16] and back[-16:] == wire[-16:]
    for at in (0, 19, 30, len(wire) - 1):
        bad = bytearray(wire)
        bad[at] ^= 1
        assert not Q.unprotect(key, iv, hp, 0, 18, bytes(bad))[2], at
    # a short header: five bits of the first byte are masked
    short = bytes([0x43]) + bytes(8) + bytes([0x12, 0x34, 0x56, 0x78]) + bytes(range(30)) + b"\xAA" * 16
    w2 = Q.protect(key, iv, hp, 0x12345678, 9, short)
    b2, pn2, ok2 = Q.unprotect(key, iv, hp, 0x12345600, 9, w2)
    assert ok2 and pn2 == 0x12345678 and b2[:-16] == short[:-16]
    assert (w2[0] ^ short[0]) & 0xE0 == 0


# ---------------------------------------------------------------- RFC 9000 Appendix A.3
def test_decode_pn():
    assert Q.decode_pn(0xa82f30ea, 0x9b32, 16) == 0xa82f9b32                 # the RFC's example
    for nbits in (8, 16, 24, 32):
        win, hwin = 1 << nbits, 1 << (nbits - 1)
        for base in (5 * win, (1 << 40) + 3 * win):
            assert Q.decode_pn(base + 10, 5, nbits) == base + 5                              # same window
            assert Q.decode_pn(base + win - 2, 1, nbits) == base + win + 1                   # wrapped upwards
            assert Q.decode_pn(base + 1, win - 2, nbits) == base - 2                         # wrapped downwards
            assert Q.decode_pn(base + hwin, 0, nbits) == base + win                          # exactly half a window away: up
            assert Q.decode_pn(base + hwin - 1, 0, nbits) == base
        # at the start of the number space nothing wraps below zero
        assert Q.decode_pn(0, win - 1, nbits) == win - 1
        assert Q.decode_pn(1, win - 1, nbits) == win - 1
        # at, below and above 2^62: the guard keeps the candidate from growing beyond the number space
        top = 1 << 62
        assert Q.decode_pn(top - 1, 0, nbits) == top - win                    # would be 2^62: the guard holds it back
        assert Q.decode_pn(top - 1, win - 1, nbits) == top - 1
        assert Q.decode_pn(top - 1 - win, 0, nbits) == top - win              # below the guard: wraps upwards
        assert Q.decode_pn(top, 3, nbits) == top + 3
        assert Q.decode_pn(top + 1, win - 1, nbits) == top - 1


# ---------------------------------------------------------------- the kernels' assembly
@pytest.fixture(scope="module")
def census():
    return asm_census("quic")


def test_quic_kernel_set(census):
    aead = {"k_kt_quic<%d, %d, %d>" % (nr, dec, lg) for nr in (10, 12, 14) for dec in (0, 1) for lg in (3, 4, 6)}
    hp = {"k_kt_quic_hp<%d, %d>" % (nr, dec) for nr in (10, 12, 14) for dec in (0, 1)}
    assert (len(aead), len(hp)) == (18, 6)
    assert set(census) == aead | hp, sorted(census)


def test_quic_kernels_scratch_free_and_in_budget(census):
    assert_in_budget(census, body="k_kt_quic<")


def test_quic_source_is_a_unit_of_its_own():
    """the other translation units name neither kernel: their censuses stay what they were"""
    for f in ("aesgcm_tls_kernels.hip", "aesgcm_wirex_kernels.hip", "aesgcm_wire_kernels.hip", "aesgcm_keytab_kernels.hip", "aesgcm_kernels.hip"):
        assert "k_kt_quic" not in open(os.path.join(CSRC, f)).read(), f
    assert '#include "aesgcm_quic_kernels.hip"' in open(os.path.join(CSRC, "aesgcm_device.hip")).read()


def test_the_quic_mode_is_no_public_extension():
    """KT_WIREX_QUIC is internal: aesgcm_wire_xfmt_check refuses it like every unknown bit"""
    xf = lib.WireFormatX.macsec_xpn()
    xf.ext = 0x40
    assert xf.check() == lib.EARG
    xf.ext = 0x40 | lib.WIREX_XPN
    assert xf.check() == lib.EARG
