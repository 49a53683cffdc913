"""What tests/test_quic_cpu.py and tests/test_gpu_quic.py share: QUIC packet protection in plain Python, written from the RFCs and from nothing else.  HKDF-Expand-Label
(RFC 8446 7.1) with hashlib / hmac; the Initial secrets of RFC 9001 5.2; header protection (RFC 9001 5.4: AES-ECB of a 16-byte sample through libcrypto's
EVP_aes_{128,256}_ecb, loaded the way oracle/libcrypto_ref.py loads its library); protect() / unprotect() (RFC 9001 5.3: the AEAD by oracle.libcrypto_ref, nonce = iv XOR
the packet number, AAD = the header up to and including the packet-number field); decode_pn() (RFC 9000 Appendix A.3, on Python's unbounded integers as the RFC writes it)."""
import ctypes
import ctypes.util
import hashlib
import hmac
import struct

from oracle import libcrypto_ref as R

INITIAL_SALT_V1 = bytes.fromhex("38762cf7f55934b34d179ae6a4c80cadccbb7f0a")        # RFC 9001 5.2


def hkdf_extract(salt, ikm, hname="sha256"):
    return hmac.new(salt, ikm, hname).digest()


def hkdf_expand_label(secret, label, length, hname="sha256"):
    """RFC 8446 7.1 with an empty context; HKDF-Expand is RFC 5869 2.3"""
    full = b"tls13 " + label
    info = struct.pack(">HB", length, len(full)) + full + b"\0"
    out, t, i = b"", b"", 1
    while len(out) < length:
        t = hmac.new(secret, t + info + bytes([i]), hname).digest()
        out += t
        i += 1
    return out[:length]


def initial_keys(dcid, who):
    """RFC 9001 5.2: (key, iv, hp) of the client's or the server's Initial packets, from the client's first Destination Connection ID"""
    initial = hkdf_extract(INITIAL_SALT_V1, dcid)
    secret = hkdf_expand_label(initial, b"client in" if who == "client" else b"server in", 32)
    return packet_keys(secret, 16)


def packet_keys(secret, key_len, hname="sha256"):
    """RFC 9001 5.1: what becomes what -- `quic key` the AEAD key, `quic iv` its 12-byte IV, `quic hp` the header-protection key"""
    return (hkdf_expand_label(secret, b"quic key", key_len, hname), hkdf_expand_label(secret, b"quic iv", 12, hname), hkdf_expand_label(secret, b"quic hp", key_len, hname))


_lc = None


def _load():
    global _lc
    if _lc is None:
        L = ctypes.CDLL(ctypes.util.find_library("crypto") or "libcrypto.so.3")
        vp = ctypes.c_void_p
        L.EVP_CIPHER_CTX_new.restype = vp
        L.EVP_CIPHER_CTX_free.argtypes = [vp]
        for nm in ("EVP_aes_128_ecb", "EVP_aes_192_ecb", "EVP_aes_256_ecb"):
            getattr(L, nm).restype = vp
        L.EVP_EncryptInit_ex.argtypes = [vp, vp, vp, ctypes.c_char_p, ctypes.c_char_p]
        L.EVP_CIPHER_CTX_set_padding.argtypes = [vp, ctypes.c_int]
        L.EVP_EncryptUpdate.argtypes = [vp, ctypes.c_char_p, ctypes.POINTER(ctypes.c_int), ctypes.c_char_p, ctypes.c_int]
        _lc = L
    return _lc


def aes_ecb(key, block):
    """one block of AES-128 / AES-192 / AES-256 under libcrypto"""
    assert len(block) == 16 and len(key) in (16, 24, 32)
    L = _load()
    ctx = L.EVP_CIPHER_CTX_new()
    try:
        assert L.EVP_EncryptInit_ex(ctx, {16: L.EVP_aes_128_ecb, 24: L.EVP_aes_192_ecb, 32: L.EVP_aes_256_ecb}[len(key)](), None, key, None) == 1
        assert L.EVP_CIPHER_CTX_set_padding(ctx, 0) == 1
        out = ctypes.create_string_buffer(32)
        n = ctypes.c_int(0)
        assert L.EVP_EncryptUpdate(ctx, out, ctypes.byref(n), block, 16) == 1 and n.value == 16
        return out.raw[:16]
    finally:
        L.EVP_CIPHER_CTX_free(ctx)


def nonce_of(iv, pn):
    return bytes(a ^ b for a, b in zip(iv, bytes(4) + struct.pack(">Q", pn)))


def hp_mask(hp, packet, pn_off):
    """RFC 9001 5.4.2: the sample is the 16 bytes that start four bytes behind the start of the packet-number field"""
    sample = packet[pn_off + 4:pn_off + 20]
    assert len(sample) == 16
    return aes_ecb(hp, sample)


def apply_mask(packet, pn_off, pn_len, mask):
    """RFC 9001 5.4.1 on a packet whose pn_len is known (protect: from the unprotected first byte; unprotect: after the first byte is unmasked)"""
    out = bytearray(packet)
    out[0] ^= mask[0] & (0x0F if out[0] & 0x80 else 0x1F)
    for i in range(pn_len):
        out[pn_off + i] ^= mask[1 + i]
    return bytes(out)


def protect(key, iv, hp, pn, pn_off, packet):
    """packet = unprotected header (truncated packet number written) | plaintext | 16 placeholder bytes -> the packet on the wire"""
    pn_len = (packet[0] & 3) + 1
    h = pn_off + pn_len
    ct, tag = R.encrypt(key, nonce_of(iv, pn), packet[:h], packet[h:-16])
    sealed = packet[:h] + bytes(ct) + bytes(tag)
    return apply_mask(sealed, pn_off, pn_len, hp_mask(hp, sealed, pn_off))


def decode_pn(expected, truncated, nbits):
    """RFC 9000 A.3, DecodePacketNumber, as written"""
    win = 1 << nbits
    hwin = win // 2
    mask = win - 1
    cand = (expected & ~mask) | truncated
    if cand <= expected - hwin and cand < (1 << 62) - win:
        return cand + win
    if cand > expected + hwin and cand >= win:
        return cand - win
    return cand


def unprotect(key, iv, hp, expected_pn, pn_off, packet):
    """the packet on the wire -> (unprotected header | plaintext | tag, full packet number, authentic)"""
    mask = hp_mask(hp, packet, pn_off)
    first = packet[0] ^ (mask[0] & (0x0F if packet[0] & 0x80 else 0x1F))
    pn_len = (first & 3) + 1
    clear = bytearray(packet)
    clear[0] = first
    for i in range(pn_len):
        clear[pn_off + i] ^= mask[1 + i]
    h = pn_off + pn_len
    pn = decode_pn(expected_pn, int.from_bytes(clear[pn_off:h], "big"), 8 * pn_len)
    pt, ok = R.decrypt(key, nonce_of(iv, pn & (2 ** 64 - 1)), bytes(clear[:h]), packet[h:-16], packet[-16:])
    return bytes(clear[:h]) + bytes(pt) + packet[-16:], pn, bool(ok)
