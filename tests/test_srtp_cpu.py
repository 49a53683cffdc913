"""CPU: SRTP and SRTCP packets through key tables (aesgcm_keytab_srtp_crypt_dev; RFC 7714 AES-GCM over RFC 3711's packets) without a GPU.  The binding and the header
name the entry points and the ABI version is still 5; aesgcm_srtp_fmt_check refuses what it must; the call refuses its argument errors before it looks at a table or a
device; tests/srtp_fixture.py -- the reference tests/test_gpu_srtp.py holds the GPU to -- reproduces RFC 7714's test vectors (tests/golden/srtp_rfc7714.json), is an
inverse of itself for both kinds and rejects a flipped bit everywhere but in the MKI; the gfx950 assembly of the kernels (`make -C csrc asm_srtp`) holds exactly the 36
k_kt_srtp instances, none with scratch, none above 128 registers.  SRTCP with E clear has no published vector: it rests on the RFC's formulas."""
import os

import pytest

import aesgcm_amd  # noqa: F401
from aesgcm_amd import lib

from kt_common import asm_census, assert_in_budget
from util import splitmix_bytes

import srtp_fixture as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "aes-gcm-128-192-256-bits_amd", "csrc")


# ---------------------------------------------------------------- binding and header
def test_srtp_symbols_in_binding_and_header():
    assert "aesgcm_keytab_srtp_crypt_dev" in lib.SYMBOLS and "aesgcm_srtp_fmt_check" in lib.SYMBOLS
    hdr = open(os.path.join(ROOT, "include", "aesgcm.h")).read()
    assert ("AESGCM_API int aesgcm_keytab_srtp_crypt_dev(aesgcm_keytab *t, int decrypt, const aesgcm_srtp_fmt *fmt, size_t n_pkts,\n"
            "                                 const uint32_t *d_slots, const uint32_t *d_roc,\n"
            "                                 const void *d_in, const uint64_t *d_pkt_off, void *d_out, int *d_auth, void *stream);") in hdr
    assert "AESGCM_API int aesgcm_srtp_fmt_check(const aesgcm_srtp_fmt *fmt);" in hdr
    assert "#define AESGCM_ABI_VERSION 5 " in hdr
    assert "#define AESGCM_SRTP_RTP  1u" in hdr and "#define AESGCM_SRTP_RTCP 2u" in hdr
    section = hdr[hdr.index("SRTP AND SRTCP PACKETS"):hdr.index("aesgcm_srtp_fmt;")]
    for out in ("ROC estimation and replay windows", "key derivation", "RFC 3711 4.3", "DTLS-SRTP exporter", "AES-CM / HMAC-SHA1", "RFC 8723", "RFC 6904", "MKI lookup",
                "reduced-size or multiplexed"):
        assert out in section, out
    L = lib._keytab_typed(lib.load())
    assert L.aesgcm_abi_version() == 5
    assert len(L.aesgcm_keytab_srtp_crypt_dev.argtypes) == 11 and len(L.aesgcm_srtp_fmt_check.argtypes) == 1
    assert (lib.SRTP_RTP, lib.SRTP_RTCP) == (1, 2) == (S.RTP, S.RTCP)
    for m in ("srtp_crypt_dev", "crypt_srtp"):
        assert callable(getattr(lib.KeyTable, m))
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "SRTP and SRTCP packets" in integ


def test_format_check():
    import ctypes
    assert ctypes.sizeof(lib.SrtpFormat) == 8
    assert (lib.SrtpFormat.rtp().kind, lib.SrtpFormat.rtp().mki_len, lib.SrtpFormat.rtcp(4).kind, lib.SrtpFormat.rtcp(4).mki_len) == (1, 0, 2, 4)
    for mki in (0, 1, 4, 127, 128):
        assert lib.SrtpFormat.rtp(mki).check() == lib.OK and lib.SrtpFormat.rtcp(mki).check() == lib.OK
    assert lib._keytab_typed(lib.load()).aesgcm_srtp_fmt_check(None) == lib.EARG
    for k in (0, 3, 4, 0x10, 0x200, 0x400, 0xFFFFFFFF):
        assert lib.SrtpFormat(k, 0).check() == lib.EARG, k
    for k in (1, 2):
        for mki in (129, 256, 0x80000000, 0xFFFFFFFF):
            assert lib.SrtpFormat(k, mki).check() == lib.EARG, (k, mki)


def test_argument_errors_before_any_table_or_device():
    """t = NULL and placeholder pointers that are never followed: the call returns before it touches a table or a device"""
    import ctypes
    f = lib._keytab_typed(lib.load()).aesgcm_keytab_srtp_crypt_dev
    P = 16                                                                   # a placeholder pointer
    rtp, rtcp = lib.SrtpFormat.rtp(), lib.SrtpFormat.rtcp(4)

    def call(fmt=rtp, t=None, decrypt=0, n=1, slots=P, roc=P, d_in=P, pkt_off=P, d_out=P, auth=P):
        return f(t, decrypt, ctypes.byref(fmt) if fmt is not None else None, n, slots, roc, d_in, pkt_off, d_out, auth, None)

    assert call(fmt=None, t=P) == lib.EARG                                   # the format first
    assert call(fmt=lib.SrtpFormat(3, 0), t=P, n=0) == lib.EARG
    assert call(fmt=lib.SrtpFormat(1, 129), t=P, n=0) == lib.EARG
    for fmt in (rtp, rtcp):
        assert call(fmt) == lib.EARG                                         # t NULL
        assert call(fmt, n=0) == lib.EARG                                    # ... whatever else
        for d in (2, -1, 7):
            assert call(fmt, t=P, decrypt=d) == lib.EARG                     # decrypt not 0 / 1 (checked with t: the placeholder is not followed)
        for name in ("slots", "d_in", "pkt_off", "d_out"):
            for d in (0, 1):
                assert call(fmt, t=P, decrypt=d, **{name: None}) == lib.EARG, name
        assert call(fmt, t=P, decrypt=1, auth=None) == lib.EARG
        assert call(fmt, t=P, n=2 ** 31) == lib.EARG
        assert call(fmt, t=P, decrypt=1, n=2 ** 31 + 5) == lib.EARG
        assert call(fmt, t=P, n=0) == lib.OK                                 # nothing to do: nothing is looked at
        assert call(fmt, t=P, n=0, decrypt=1, auth=None, roc=None) == lib.OK
    for d in (0, 1):
        assert call(rtp, t=P, decrypt=d, roc=None) == lib.EARG               # SRTP alone needs the rollover counters
    # SRTCP ignores them: with d_roc NULL the next refusal is n_pkts
    assert call(rtcp, t=P, decrypt=1, n=2 ** 31, roc=None) == lib.EARG


# ---------------------------------------------------------------- the fixture
def test_fixture_reproduces_rfc7714_vectors():
    vs = S.vectors()
    assert [(k, len(key)) for _, k, key, _, _, _, _, _ in vs] == [(S.RTP, 16), (S.RTP, 32), (S.RTCP, 16)]
    for name, kind, key, salt, roc, plain, nonce, wire in vs:
        assert len(plain) == len(wire), name
        if kind == S.RTP:
            assert S.rtp_hdr_len(plain) == 12 and S.nonce_rtp(salt, plain, roc) == nonce, name
        else:
            assert S.nonce_rtcp(salt, plain, int.from_bytes(plain[-4:], "big")) == nonce and plain[-4] & 0x80, name
        assert S.protect(kind, key, salt, roc, plain) == wire, name
        back, ok = S.unprotect(kind, key, salt, roc, wire)
        assert ok and back == plain[:len(plain) - (16 if kind == S.RTP else 20)] + wire[len(wire) - (16 if kind == S.RTP else 20):], name
        # the same packets with an MKI behind them: the same bytes in front of it
        assert S.protect(kind, key, salt, roc, plain + b"\x01\x02\x03\x04", 4) == wire + b"\x01\x02\x03\x04", name


def _rtp(cc, ext, n, seed, mki=b""):
    fill = splitmix_bytes(seed, 200 + n)
    return S.rtp_header(cc, ext, 0x1234 + seed, 0xCAFE0000 + seed, 0xDECAFBAD ^ seed, fill) + fill[200:200 + n] + b"\xAA" * 16 + mki


def _rtcp(e, n_words, index, seed, mki=b""):
    fill = splitmix_bytes(seed, 8 + 4 * n_words)
    hdr = bytes([0x81, 200]) + (1 + n_words).to_bytes(2, "big") + fill[:4]
    return hdr + fill[8:] + b"\xAA" * 16 + ((e << 31) | index).to_bytes(4, "big") + mki


@pytest.mark.parametrize("key_len", [16, 32])
def test_srtp_protect_and_unprotect_are_inverse_and_reject(key_len):
    key, salt = splitmix_bytes(0x5270 + key_len, key_len), splitmix_bytes(0x5271, 12)
    for cc, ext in ((0, None), (1, None), (15, None), (0, 0), (2, 1), (15, 5)):
        for n in (0, 1, 16, 100):
            for mki in (b"", b"\x11\x22\x33\x44"):
                roc = 7
                plain = _rtp(cc, ext, n, 1 + n + cc, mki)
                h = 12 + 4 * cc + (0 if ext is None else 4 + 4 * ext)
                assert S.rtp_hdr_len(plain) == h and len(plain) == h + n + 16 + len(mki)
                wire = S.protect_rtp(key, salt, roc, plain, len(mki))
                t = len(wire) - len(mki) - 16
                assert len(wire) == len(plain) and wire[:h] == plain[:h] and wire[t + 16:] == mki
                back, ok = S.unprotect_rtp(key, salt, roc, wire, len(mki))
                assert ok and back == plain[:t] + wire[t:]
                assert not S.unprotect_rtp(key, salt, roc + 1, wire, len(mki))[1]              # a wrong rollover counter
                # header (marker bit), sequence number, SSRC, a CSRC, the extension (profile byte, a word), payload, tag
                ats = {1, 3, 8, 11, t, t + 15}
                if cc:
                    ats |= {12, 12 + 4 * cc - 1}
                if ext is not None:
                    ats |= {12 + 4 * cc, h - 1}
                if n:
                    ats |= {h, t - 1}
                for at in ats:
                    bad = bytearray(wire)
                    bad[at] ^= 0x80 if at == 1 else 1
                    assert not S.unprotect_rtp(key, salt, roc, bytes(bad), len(mki))[1], (cc, ext, n, at)
                for at in range(t + 16, len(wire)):                                            # the MKI is not authenticated
                    bad = bytearray(wire)
                    bad[at] ^= 1
                    assert S.unprotect_rtp(key, salt, roc, bytes(bad), len(mki)) == (back[:at] + bytes([bad[at]]) + back[at + 1:], True)


@pytest.mark.parametrize("key_len", [16, 32])
def test_srtcp_protect_and_unprotect_are_inverse_and_reject(key_len):
    key, salt = splitmix_bytes(0x5280 + key_len, key_len), splitmix_bytes(0x5281, 12)
    for e in (1, 0):
        for n_words in (0, 1, 2, 3, 4, 5, 30):
            for mki in (b"", b"\x11\x22\x33"):
                plain = _rtcp(e, n_words, 0x5d4 + n_words, 3 + n_words, mki)
                wire = S.protect_rtcp(key, salt, plain, len(mki))
                t = len(wire) - len(mki) - 20
                assert t == 8 + 4 * n_words and len(wire) == len(plain) and wire[:8] == plain[:8] and wire[t + 16:] == plain[t + 16:]
                assert (wire[8:t] == plain[8:t]) == (e == 0 or n_words == 0)                   # E clear: nothing is encrypted
                back, ok = S.unprotect_rtcp(key, salt, wire, len(mki))
                assert ok and back == plain[:t] + wire[t:]
                # header, SSRC, payload, tag, W: the E bit, the index
                ats = {0, 1, 4, 7, t, t + 15, t + 16, t + 19}
                if n_words:
                    ats |= {8, t - 1}
                for at in ats:
                    bad = bytearray(wire)
                    bad[at] ^= 0x80 if at == t + 16 else 1
                    assert not S.unprotect_rtcp(key, salt, bytes(bad), len(mki))[1], (e, n_words, at)
                for at in range(t + 20, len(wire)):
                    bad = bytearray(wire)
                    bad[at] ^= 1
                    assert S.unprotect_rtcp(key, salt, bytes(bad), len(mki))[1]
    # a bare header: the same nonce with E set or clear (it takes the index alone) and the same 12 AAD bytes but for the E bit, which the tag covers
    a, b = _rtcp(1, 0, 9, 5), _rtcp(0, 0, 9, 5)
    assert S.nonce_rtcp(salt, a, 0x80000009) == S.nonce_rtcp(salt, b, 9) and S.protect_rtcp(key, salt, a)[8:24] != S.protect_rtcp(key, salt, b)[8:24]


# ---------------------------------------------------------------- the kernels' assembly
@pytest.fixture(scope="module")
def census():
    return asm_census("srtp")


def test_srtp_kernel_set(census):
    want = {"k_kt_srtp<%d, %d, %d, %du>" % (nr, dec, lg, kind) for nr in (10, 12, 14) for dec in (0, 1) for lg in (3, 4, 6) for kind in (1, 2)}
    assert len(want) == 36
    assert set(census) == want, sorted(census)


def test_srtp_kernels_scratch_free_and_in_budget(census):
    assert_in_budget(census, body="k_kt_srtp<")


def test_srtp_source_is_a_unit_of_its_own():
    """no other translation unit names the kernel: their censuses stay what they were"""
    others = [f for f in os.listdir(CSRC) if f.endswith("_kernels.hip") and f != "aesgcm_srtp_kernels.hip"]
    assert len(others) >= 7
    for f in others:
        assert "k_kt_srtp" not in open(os.path.join(CSRC, f)).read(), f
    assert '#include "aesgcm_srtp_kernels.hip"' in open(os.path.join(CSRC, "aesgcm_device.hip")).read()
    assert "srtp" in [w for ln in open(os.path.join(CSRC, "Makefile")) if ln.startswith("FAMILIES") for w in ln.split()]


def test_the_srtp_modes_are_no_public_extension():
    """KT_WIREX_SRTP / KT_WIREX_SRTCP are internal: aesgcm_wire_xfmt_check refuses them like every unknown bit"""
    kh = open(os.path.join(CSRC, "aesgcm_keytab.h")).read()
    assert "#define KT_WIREX_SRTP 0x200u" in kh and "#define KT_WIREX_SRTCP 0x400u" in kh
    for v in (0x200, 0x400):
        xf = lib.WireFormatX.macsec_xpn()
        xf.ext = v
        assert xf.check() == lib.EARG
        xf.ext = v | lib.WIREX_XPN
        assert xf.check() == lib.EARG
