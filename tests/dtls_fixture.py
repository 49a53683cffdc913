"""What tests/test_dtls_cpu.py and tests/test_gpu_dtls.py share: DTLS record protection in plain Python over libcrypto, written from the RFCs and from nothing else -- it is
the GPU's reference and does not import the library.
DTLS 1.3 (RFC 9147): the unified header of 4, its record-number encryption (4.2.3: AES-ECB of the first 16 ciphertext bytes under the `sn` key, through
quic_fixture.aes_ecb), the AEAD of 4.2.1 / RFC 8446 5.2, 5.3 (nonce = iv XOR the 64-bit record sequence number, AAD = the unprotected header) by oracle.libcrypto_ref, and
the keys of 5.9: HKDF-Expand-Label as tls_fixture.hkdf_expand_label writes it, with the label prefix "dtls13" in place of "tls13 ".  decode_seq: RFC 9000 Appendix A.3's
rule on Python's unbounded integers, with 2^64 - 1 as the last number.
DTLS 1.2 (RFC 6347 with RFC 5288): hdr[13] | explicit nonce[8] | payload | tag[16]; nonce = the write IV's four bytes | explicit nonce; AAD = epoch | sequence number
| type | version | payload length (RFC 6347 4.1.2.1); the key block by tls_fixture.prf12.  tests/golden/dtls12_records.json holds records of a real
DTLS 1.2 stack, OpenSSL's (tests/golden/gen_dtls_records.py; directions() below); DTLS 1.3 has no such witness here and rests on the formulas alone."""
import base64
import hmac
import struct

from oracle import libcrypto_ref as R

import tls_fixture as T
from quic_fixture import aes_ecb
from util import golden, splitmix_bytes

DTLS13, DTLS12 = 1, 2
LAST = (1 << 64) - 1


# ---------------------------------------------------------------- keys
def hkdf_expand_label13(hname, secret, label, length):
    """RFC 9147 5.9: RFC 8446 7.1's HkdfLabel with the prefix "dtls13" (no blank), an empty context; the expansion is tls_fixture's"""
    full = b"dtls13" + label
    info = struct.pack(">HB", length, len(full)) + full + b"\0"
    out, t, i = b"", b"", 1
    while len(out) < length:
        t = hmac.new(secret, t + info + bytes([i]), hname).digest()
        out += t
        i += 1
    return out[:length]


assert T.hkdf_expand_label("sha256", b"k" * 32, b"key", 16) != hkdf_expand_label13("sha256", b"k" * 32, b"key", 16)


def keys13(secret, key_len, hname="sha256"):
    """what becomes what: `key` the AEAD key, `iv` its 12-byte IV, `sn` the record-number key -- all from one direction's traffic secret of one epoch"""
    return hkdf_expand_label13(hname, secret, b"key", key_len), hkdf_expand_label13(hname, secret, b"iv", 12), hkdf_expand_label13(hname, secret, b"sn", key_len)


def keys12(master, client_random, server_random, key_len, who, hname="sha256"):
    """RFC 5246 6.3 for an AEAD suite: client_write_key | server_write_key | client_write_IV[4] | server_write_IV[4] -> (key, 12-byte slot IV: four bytes, then zeros)"""
    block = T.prf12(hname, master, b"key expansion", server_random + client_random, 2 * key_len + 8)
    i = 0 if who == "client" else 1
    return block[i * key_len:(i + 1) * key_len], block[2 * key_len + 4 * i:2 * key_len + 4 * i + 4] + bytes(8)


# ---------------------------------------------------------------- DTLS 1.3
def header13(cid, seq, s16, with_len, epoch, body_len):
    """the unified header 0 0 1 C S L E E | connection ID | 8 or 16 bits of the sequence number | (length); body_len = ciphertext and tag"""
    b0 = 0x20 | (0x10 if cid else 0) | (0x08 if s16 else 0) | (0x04 if with_len else 0) | (epoch & 3)
    return bytes([b0]) + cid + (seq & (0xFFFF if s16 else 0xFF)).to_bytes(2 if s16 else 1, "big") + (struct.pack(">H", body_len & 0xFFFF) if with_len else b"")


def hdr_len13(rec, sn_off):
    return sn_off + (2 if rec[0] & 0x08 else 1) + (2 if rec[0] & 0x04 else 0)


def nonce13(iv, seq):
    return bytes(a ^ b for a, b in zip(iv, bytes(4) + struct.pack(">Q", seq)))


def sn_mask(sn, rec, sn_off):
    """RFC 9147 4.2.3: the mask from the first 16 bytes of the ciphertext (the tag belongs to it)"""
    h = hdr_len13(rec, sn_off)
    sample = rec[h:h + 16]
    assert len(sample) == 16
    return aes_ecb(sn, sample)


def _xor_seq(rec, sn_off, mask):
    out = bytearray(rec)
    for i in range(2 if rec[0] & 0x08 else 1):
        out[sn_off + i] ^= mask[i]
    return bytes(out)


def protect13(key, iv, sn, seq, sn_off, rec):
    """rec = unprotected header (truncated number written) | plaintext | 16 placeholder bytes -> the record on the wire"""
    h = hdr_len13(rec, sn_off)
    ct, tag = R.encrypt(key, nonce13(iv, seq), rec[:h], rec[h:-16])
    sealed = rec[:h] + bytes(ct) + bytes(tag)
    return _xor_seq(sealed, sn_off, sn_mask(sn, sealed, sn_off))


def decode_seq(expected, truncated, nbits):
    """RFC 9000 A.3's DecodePacketNumber with 2^64 - 1 as the last number: closest to expected, a tie upwards; never below 0, never above 2^64 - 1"""
    win = 1 << nbits
    hwin = win // 2
    cand = (expected & ~(win - 1)) | truncated
    if cand <= expected - hwin and cand + win <= LAST:
        return cand + win
    if cand > expected + hwin and cand >= win:
        return cand - win
    return cand


def unprotect13(key, iv, sn, expected, sn_off, rec):
    """the record on the wire -> (unprotected header | plaintext | tag, full sequence number, authentic)"""
    clear = _xor_seq(rec, sn_off, sn_mask(sn, rec, sn_off))
    h = hdr_len13(rec, sn_off)
    n = 2 if rec[0] & 0x08 else 1
    seq = decode_seq(expected, int.from_bytes(clear[sn_off:sn_off + n], "big"), 8 * n)
    pt, ok = R.decrypt(key, nonce13(iv, seq), clear[:h], rec[h:-16], rec[-16:])
    return clear[:h] + bytes(pt) + rec[-16:], seq, bool(ok)


# ---------------------------------------------------------------- DTLS 1.2
def header12(ctype, epoch, seq48, payload_len, version=b"\xfe\xfd"):
    """type | version | epoch | 48-bit sequence number | length of what follows the header (explicit nonce, payload, tag)"""
    return bytes([ctype]) + version + struct.pack(">H", epoch) + seq48.to_bytes(6, "big") + struct.pack(">H", (payload_len + 24) & 0xFFFF)


def nonce12(iv, rec):
    return iv[:4] + rec[13:21]


def aad12(rec):
    return rec[3:11] + rec[0:3] + struct.pack(">H", len(rec) - 37)


def protect12(key, iv, rec):
    """rec = hdr[13] | explicit nonce[8] | plaintext | 16 placeholder bytes -> the record on the wire"""
    ct, tag = R.encrypt(key, nonce12(iv, rec), aad12(rec), rec[21:-16])
    return rec[:21] + bytes(ct) + bytes(tag)


def unprotect12(key, iv, rec):
    """-> (hdr | explicit nonce | plaintext | tag, authentic)"""
    pt, ok = R.decrypt(key, nonce12(iv, rec), aad12(rec), rec[21:-16], rec[-16:])
    return rec[:21] + bytes(pt) + rec[-16:], bool(ok)


# ---------------------------------------------------------------- the recorded DTLS 1.2 records
def directions():
    """every (connection, direction) of tests/golden/dtls12_records.json: (conn, who, key, iv, [(wire record, plaintext as written)]), the keys derived here from the
    connection's master secret and randoms"""
    out = []
    for conn in golden("dtls12_records.json")["connections"]:
        for who in ("client", "server"):
            key, iv = keys12(bytes.fromhex(conn["master_secret"]), bytes.fromhex(conn["client_random"]), bytes.fromhex(conn["server_random"]), conn["key_len"], who,
                             conn["hash"])
            out.append((conn, who, key, iv, [(base64.b64decode(r["wire"]), splitmix_bytes(r["seed"], r["len"])) for r in conn["dirs"][who]["records"]]))
    return out
