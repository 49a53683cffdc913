"""CPU: DTLS records through key tables (aesgcm_keytab_dtls_crypt_dev; DTLS 1.3: RFC 9147, DTLS 1.2 AES-GCM: RFC 6347 / RFC 5288) without a GPU.  The binding and the
header name the entry points and the ABI version is still 5; aesgcm_dtls_fmt_check refuses what it must; the call refuses its argument errors before it looks at a table
or a device; tests/dtls_fixture.py -- the reference tests/test_gpu_dtls.py holds the GPU to -- is an inverse of itself, rejects every flipped bit and decodes sequence
numbers as RFC 9000 Appendix A.3 does between 0 and 2^64 - 1; the gfx950 assembly of the kernels (`make -C csrc asm_dtls`) holds exactly the 36 k_kt_dtls and 6
k_kt_dtls_sn instances, none with scratch, none above 128 registers.  DTLS 1.2 has a witness: the records of tests/golden/dtls12_records.json, as OpenSSL sent them,
decrypt under keys derived here and are reproduced byte for byte.  DTLS 1.3 has none: it rests on the RFC's formulas."""
import os

import pytest

import aesgcm_amd  # noqa: F401
from aesgcm_amd import lib

from kt_common import asm_census, assert_in_budget
from util import splitmix_bytes

import dtls_fixture as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "aes-gcm-128-192-256-bits_amd", "csrc")


# ---------------------------------------------------------------- binding and header
def test_dtls_symbols_in_binding_and_header():
    assert "aesgcm_keytab_dtls_crypt_dev" in lib.SYMBOLS and "aesgcm_dtls_fmt_check" in lib.SYMBOLS
    hdr = open(os.path.join(ROOT, "include", "aesgcm.h")).read()
    assert "AESGCM_API int aesgcm_keytab_dtls_crypt_dev(aesgcm_keytab *t, int decrypt, const aesgcm_dtls_fmt *fmt, size_t n_recs," in hdr
    assert "AESGCM_API int aesgcm_dtls_fmt_check(const aesgcm_dtls_fmt *fmt);" in hdr
    assert "#define AESGCM_ABI_VERSION 5 " in hdr
    assert "#define AESGCM_DTLS_13 1u" in hdr and "#define AESGCM_DTLS_12 2u" in hdr
    assert "; DTLS;" not in hdr                                              # no out-of-scope list names it any more
    for out in ("RFC 9146", "coalesced datagrams", "epoch bits", "anti-replay", "key derivation", "ChaCha20 and CCM"):
        assert out in hdr[hdr.index("DTLS RECORDS"):hdr.index("aesgcm_dtls_fmt;")], out
    L = lib._keytab_typed(lib.load())
    assert L.aesgcm_abi_version() == 5
    assert len(L.aesgcm_keytab_dtls_crypt_dev.argtypes) == 14
    assert (lib.DTLS_13, lib.DTLS_12) == (1, 2)
    for m in ("dtls_crypt_dev", "crypt_dtls"):
        assert callable(getattr(lib.KeyTable, m))


def test_format_check():
    import ctypes
    assert ctypes.sizeof(lib.DtlsFormat) == 8
    assert lib.DtlsFormat.dtls13().check() == lib.OK and lib.DtlsFormat.dtls12().check() == lib.OK
    assert lib._keytab_typed(lib.load()).aesgcm_dtls_fmt_check(None) == lib.EARG
    for v in (0, 3, 4, 0x10, 0x80, 0x100, 0xFFFFFFFF):
        assert lib.DtlsFormat(v, 0).check() == lib.EARG, v
    for v in (1, 2):
        for r in (1, 0x80000000):
            assert lib.DtlsFormat(v, r).check() == lib.EARG, (v, r)


def test_argument_errors_before_any_table_or_device():
    """t = NULL and placeholder pointers that are never followed: the call returns before it touches a table or a device"""
    import ctypes
    f = lib._keytab_typed(lib.load()).aesgcm_keytab_dtls_crypt_dev
    P = 16                                                                   # a placeholder pointer
    f13, f12 = lib.DtlsFormat.dtls13(), lib.DtlsFormat.dtls12()

    def call(fmt=f13, t=None, decrypt=0, n=1, slots=P, sn=P, seq=P, seq_out=P, sn_off=P, d_in=P, rec_off=P, d_out=P, auth=P):
        return f(t, decrypt, ctypes.byref(fmt) if fmt is not None else None, n, slots, sn, seq, seq_out, sn_off, d_in, rec_off, d_out, auth, None)

    assert call(fmt=None, t=P) == lib.EARG                                   # the format first
    assert call(fmt=lib.DtlsFormat(3, 0), t=P, n=0) == lib.EARG
    assert call(fmt=lib.DtlsFormat(1, 1), t=P, n=0) == lib.EARG
    for fmt in (f13, f12):
        assert call(fmt) == lib.EARG                                         # t NULL
        assert call(fmt, n=0) == lib.EARG                                    # ... whatever else
        for d in (2, -1, 7):
            assert call(fmt, t=P, decrypt=d) == lib.EARG                     # decrypt not 0 / 1 (checked with t: the placeholder is not followed)
        for name in ("slots", "d_in", "rec_off", "d_out"):
            for d in (0, 1):
                assert call(fmt, t=P, decrypt=d, **{name: None}) == lib.EARG, name
        assert call(fmt, t=P, decrypt=1, auth=None) == lib.EARG
        assert call(fmt, t=P, n=2 ** 31) == lib.EARG
        assert call(fmt, t=P, decrypt=1, n=2 ** 31 + 5) == lib.EARG
        assert call(fmt, t=P, n=0) == lib.OK                                 # nothing to do: nothing is looked at
        assert call(fmt, t=P, n=0, decrypt=1, auth=None, seq_out=None, sn=None, seq=None, sn_off=None) == lib.OK
    for name in ("sn", "seq", "sn_off"):                                     # DTLS 1.3 alone needs them
        for d in (0, 1):
            assert call(f13, t=P, decrypt=d, **{name: None}) == lib.EARG, name
    assert call(f13, t=P, decrypt=1, seq_out=None) == lib.EARG
    # DTLS 1.2 ignores them: with every one NULL the next refusal is n_recs
    assert call(f12, t=P, decrypt=1, n=2 ** 31, sn=None, seq=None, seq_out=None, sn_off=None) == lib.EARG


# ---------------------------------------------------------------- the fixture
def _rec13(cid, seq, s16, with_len, payload):
    h = D.header13(cid, seq, s16, with_len, 2, len(payload) + 16)
    return h + payload + b"\xAA" * 16


@pytest.mark.parametrize("key_len, hname", [(16, "sha256"), (32, "sha384")])
def test_dtls13_protect_and_unprotect_are_inverse_and_reject(key_len, hname):
    key, iv, sn = D.keys13(splitmix_bytes(0xD713, 48), key_len, hname)
    assert (len(key), len(iv), len(sn)) == (key_len, 12, key_len) and key != sn
    for cid in (b"", b"\x01", bytes(range(7)), bytes(range(20))):
        for s16 in (False, True):
            for with_len in (False, True):
                for n in (0, 1, 16, 100):
                    seq = (2 << 48) | 0x1234
                    plain = _rec13(cid, seq, s16, with_len, splitmix_bytes(n + 1, n))
                    sn_off = 1 + len(cid)
                    assert D.hdr_len13(plain, sn_off) == 1 + len(cid) + (2 if s16 else 1) + (2 if with_len else 0)
                    wire = D.protect13(key, iv, sn, seq, sn_off, plain)
                    assert len(wire) == len(plain) and wire[:sn_off] == plain[:sn_off]
                    back, got, ok = D.unprotect13(key, iv, sn, seq - 3, sn_off, wire)
                    assert ok and got == seq and back[:-16] == plain[:-16] and back[-16:] == wire[-16:]
                    h = D.hdr_len13(plain, sn_off)
                    for at in {0, sn_off, h - 1, h, len(wire) - 17 if n else h, len(wire) - 1, len(wire) - 16}:
                        bad = bytearray(wire)
                        bad[at] ^= 0x10 if at == 0 else 1                    # (byte 0: the C bit, which moves nothing: the header is AAD)
                        assert not D.unprotect13(key, iv, sn, seq - 3, sn_off, bytes(bad))[2], (len(cid), s16, with_len, n, at)


def test_dtls13_mask_is_ecb_of_the_first_ciphertext_bytes():
    key, iv, sn = D.keys13(b"s" * 32, 16)
    plain = _rec13(b"\x07" * 4, 0x0102, True, True, bytes(40))
    wire = D.protect13(key, iv, sn, 0x0102, 5, plain)
    mask = D.aes_ecb(sn, wire[9:25])
    assert D.sn_mask(sn, wire, 5) == mask
    assert bytes(a ^ b for a, b in zip(wire[5:7], mask)) == b"\x01\x02" and wire[7:9] == plain[7:9]


@pytest.mark.parametrize("key_len, hname", [(16, "sha256"), (32, "sha384")])
def test_dtls12_protect_and_unprotect_are_inverse_and_reject(key_len, hname):
    master, cr, sr = splitmix_bytes(0xD712, 48), splitmix_bytes(0xD7C, 32), splitmix_bytes(0xD75, 32)
    key, iv = D.keys12(master, cr, sr, key_len, "client", hname)
    key_s, iv_s = D.keys12(master, cr, sr, key_len, "server", hname)
    assert len(key) == key_len and iv[4:] == bytes(8) and key != key_s and iv != iv_s
    for n in (0, 1, 15, 16, 17, 1400):
        plain = D.header12(23, 1, 5 + n, n) + splitmix_bytes(n, 8) + splitmix_bytes(n + 100, n) + b"\xAA" * 16
        assert len(plain) == n + 37 and D.aad12(plain) == plain[3:11] + b"\x17\xfe\xfd" + n.to_bytes(2, "big")
        wire = D.protect12(key, iv, plain)
        assert wire[:21] == plain[:21] and len(wire) == len(plain)
        back, ok = D.unprotect12(key, iv, wire)
        assert ok and back[:-16] == plain[:-16]
        for at in {0, 1, 3, 5, 10, 13, 20, 21 if n else 36, len(wire) - 1, len(wire) - 16}:      # type, version, epoch, sequence number, nonce, payload, tag
            bad = bytearray(wire)
            bad[at] ^= 1
            assert not D.unprotect12(key, iv, bytes(bad))[1], (n, at)
        # the header's own length bytes are not authenticated as such: the AAD's length comes from the record's size
        bad = bytearray(wire)
        bad[12] ^= 1
        assert D.unprotect12(key, iv, bytes(bad))[1]


def test_recorded_openssl_records_decrypt_and_are_reproduced():
    """DTLS 1.2 records of OpenSSL: two suites, both directions, writes of 1, 15, 16, 17, 100 and 1400 bytes"""
    dirs = D.directions()
    assert [(c["suite"], c["key_len"], who) for c, who, _, _, _ in dirs] == [(s, k, w) for s, k in (("ECDHE-RSA-AES128-GCM-SHA256", 16), ("ECDHE-RSA-AES256-GCM-SHA384", 32))
                                                                            for w in ("client", "server")]
    for conn, who, key, iv, recs in dirs:
        assert [len(pt) for _, pt in recs] == [1, 15, 16, 17, 100, 1400]
        for wire, pt in recs:
            assert wire[0] == 23 and wire[1:3] == b"\xfe\xfd" and wire[3:5] == b"\x00\x01" and int.from_bytes(wire[11:13], "big") == len(wire) - 13 == len(pt) + 24
            back, ok = D.unprotect12(key, iv, wire)
            assert ok and back[21:-16] == pt, (conn["suite"], who, len(pt))
            assert D.protect12(key, iv, wire[:21] + pt + bytes(16)) == wire
            wrong, _ = D.keys12(bytes.fromhex(conn["master_secret"]), bytes.fromhex(conn["client_random"]), bytes.fromhex(conn["server_random"]), conn["key_len"],
                                "server" if who == "client" else "client", conn["hash"])
            assert not D.unprotect12(wrong, iv, wire)[1]


def test_decode_seq():
    for nbits in (8, 16):
        win, hwin = 1 << nbits, 1 << (nbits - 1)
        for base in (5 * win, (1 << 48) + 3 * win, (1 << 63) + 7 * win):
            assert D.decode_seq(base + 10, 5, nbits) == base + 5                              # inside the window
            assert D.decode_seq(base + win - 2, 1, nbits) == base + win + 1                   # wrapped upwards
            assert D.decode_seq(base + 1, win - 2, nbits) == base - 2                         # wrapped downwards
            assert D.decode_seq(base + hwin, 0, nbits) == base + win                          # exactly half a window away: up
            assert D.decode_seq(base + hwin - 1, 0, nbits) == base
            assert D.decode_seq(base, hwin, nbits) == base + hwin                             # half a window above: stays
            assert D.decode_seq(base, hwin + 1, nbits) == base - hwin + 1
        # at 0 nothing is looked for below zero
        for t in (0, 1, hwin, hwin + 1, win - 1):
            assert D.decode_seq(0, t, nbits) == t
        assert D.decode_seq(1, win - 1, nbits) == win - 1
        assert D.decode_seq(hwin, win - 1, nbits) == win - 1
        # at 2^64 - 1 nothing above it: the candidate of the last window
        top = D.LAST
        for t in (0, 1, hwin - 1, hwin, win - 1):
            assert D.decode_seq(top, t, nbits) == top - (win - 1) + t
        assert D.decode_seq(top - win, 0, nbits) == top - win + 1                             # one window below the top: still upwards
        assert D.decode_seq(top - win + 1, 0, nbits) == top - win + 1                         # the candidate itself
        assert D.decode_seq(top - hwin, 0, nbits) == top - win + 1                            # the candidate below is the closer one
        assert D.decode_seq(top - hwin + 1, 0, nbits) == top - win + 1                        # a tie, and up would pass the last number: held back


# ---------------------------------------------------------------- the kernels' assembly
@pytest.fixture(scope="module")
def census():
    return asm_census("dtls")


def test_dtls_kernel_set(census):
    aead = {"k_kt_dtls<%d, %d, %d, %du>" % (nr, dec, lg, ver) for nr in (10, 12, 14) for dec in (0, 1) for lg in (3, 4, 6) for ver in (1, 2)}
    sn = {"k_kt_dtls_sn<%d, %d>" % (nr, dec) for nr in (10, 12, 14) for dec in (0, 1)}
    assert (len(aead), len(sn)) == (36, 6)
    assert set(census) == aead | sn, sorted(census)


def test_dtls_kernels_scratch_free_and_in_budget(census):
    assert_in_budget(census, body="k_kt_dtls<")


def test_dtls_source_is_a_unit_of_its_own():
    """the other translation units name neither kernel: their censuses stay what they were"""
    for f in ("aesgcm_quic_kernels.hip", "aesgcm_tls_kernels.hip", "aesgcm_wirex_kernels.hip", "aesgcm_wire_kernels.hip", "aesgcm_keytab_kernels.hip", "aesgcm_kernels.hip"):
        assert "k_kt_dtls" not in open(os.path.join(CSRC, f)).read(), f
    assert '#include "aesgcm_dtls_kernels.hip"' in open(os.path.join(CSRC, "aesgcm_device.hip")).read()
    assert "dtls" in [w for ln in open(os.path.join(CSRC, "Makefile")) if ln.startswith("FAMILIES") for w in ln.split()]
    # what the two mask kernels share is one header, included by both
    for f in ("aesgcm_quic_kernels.hip", "aesgcm_dtls_kernels.hip"):
        src = open(os.path.join(CSRC, f)).read()
        assert '#include "aesgcm_mask.h"' in src and "mask_take(" in src and "mask_of_sample<NR>(" in src, f


def test_the_dtls_modes_are_no_public_extension():
    """KT_WIREX_DTLS13 / KT_WIREX_DTLS12 are internal: aesgcm_wire_xfmt_check refuses them like every unknown bit"""
    kh = open(os.path.join(CSRC, "aesgcm_keytab.h")).read()
    assert "#define KT_WIREX_DTLS13 0x80u" in kh and "#define KT_WIREX_DTLS12 0x100u" in kh
    for v in (0x80, 0x100):
        xf = lib.WireFormatX.macsec_xpn()
        xf.ext = v
        assert xf.check() == lib.EARG
        xf.ext = v | lib.WIREX_XPN
        assert xf.check() == lib.EARG
