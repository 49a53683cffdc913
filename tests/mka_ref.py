"""What tests/test_mka_cpu.py and tests/test_gpu_mka.py share: MACsec's MKA key hierarchy (IEEE 802.1X-2010 6.2, 9.3, 9.8) in plain Python over libcrypto -- it is the
library's reference and does not import it.
    PRF    = AES-CMAC (RFC 4493; SP 800-38B), written here over libcrypto's single-block AES_encrypt
    KDF    = first Length bits of PRF(Key, 0x01 | Label | 0x00 | Context | be16(Length)) | PRF(Key, 0x02 | ...) | ...          (the counter one byte, Length in bits)
    KEK    = KDF(CAK, "IEEE8021 KEK", Keyid, 8 * len(CAK)),   Keyid = the CKN's first 16 bytes, zero-padded on the right where it is shorter
    SAK    = KDF(CAK, "IEEE8021 SAK", KS-nonce | MI-value list | be32(KN), 8 * key_len)
    wrap   = RFC 3394 with the default initial value: libcrypto's AES_wrap_key / AES_unwrap_key
tests/golden/mka_vectors.json pins the CMAC to RFC 4493's four AES-128 examples and SP 800-38B's AES-256 examples, and cmac_libcrypto (libcrypto's own CMAC_*) stands
beside it; the wrap is pinned to RFC 3394 4.1 and 4.6.  THE KDF ITSELF HAS NO PUBLISHED VECTOR AT HAND: it rests on 802.1X's formula as written above
(tests/COVERAGE_mka.md)."""
import ctypes
import ctypes.util
import struct

from util import golden

LABEL_KEK, LABEL_SAK = b"IEEE8021 KEK", b"IEEE8021 SAK"
CTX_MAX = 2048
_lc = None


def _load():
    global _lc
    if _lc is None:
        L = ctypes.CDLL(ctypes.util.find_library("crypto") or "libcrypto.so.3")
        vp, cp, ci, sz = ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int, ctypes.c_size_t
        L.AES_set_encrypt_key.argtypes = L.AES_set_decrypt_key.argtypes = [cp, ci, vp]
        L.AES_encrypt.argtypes = L.AES_decrypt.argtypes = [cp, vp, vp]
        L.AES_encrypt.restype = L.AES_decrypt.restype = None
        L.AES_wrap_key.argtypes = L.AES_unwrap_key.argtypes = [vp, cp, vp, cp, ctypes.c_uint]
        L.CMAC_CTX_new.restype = vp
        L.CMAC_CTX_free.argtypes = [vp]
        L.CMAC_CTX_free.restype = None
        L.EVP_aes_128_cbc.restype = L.EVP_aes_256_cbc.restype = vp
        L.CMAC_Init.argtypes = [vp, cp, sz, vp, vp]
        L.CMAC_Update.argtypes = [vp, cp, sz]
        L.CMAC_Final.argtypes = [vp, vp, ctypes.POINTER(sz)]
        _lc = L
    return _lc


class _Key:
    """libcrypto's AES_KEY (at most 244 bytes) for one direction"""

    def __init__(self, key, decrypt=False):
        assert len(key) in (16, 32)
        self.L, self.buf = _load(), ctypes.create_string_buffer(256)
        assert (self.L.AES_set_decrypt_key if decrypt else self.L.AES_set_encrypt_key)(bytes(key), 8 * len(key), self.buf) == 0

    def block(self, b, decrypt=False):
        out = ctypes.create_string_buffer(16)
        (self.L.AES_decrypt if decrypt else self.L.AES_encrypt)(bytes(b), out, self.buf)
        return out.raw


def aes_decrypt(key, block):
    """one block through libcrypto's inverse cipher"""
    assert len(block) == 16
    return _Key(key, True).block(block, True)


def _dbl(b):
    v = int.from_bytes(b, "big") << 1
    return ((v & ((1 << 128) - 1)) ^ (0x87 if v >> 128 else 0)).to_bytes(16, "big")


def _xor(a, b):
    return bytes(x ^ y for x, y in zip(a, b))


def cmac(key, msg, _k=None):
    """RFC 4493 2.4 over single-block AES"""
    k = _k or _Key(key)
    k1 = _dbl(k.block(bytes(16)))
    k2 = _dbl(k1)
    msg = bytes(msg)
    n = max(1, -(-len(msg) // 16))
    last = msg[16 * (n - 1):]
    last = _xor(last, k1) if len(last) == 16 else _xor(last + b"\x80" + bytes(15 - len(last)), k2)
    x = bytes(16)
    for i in range(n - 1):
        x = k.block(_xor(x, msg[16 * i:16 * i + 16]))
    return k.block(_xor(x, last))


def cmac_libcrypto(key, msg):
    """libcrypto's own CMAC"""
    L = _load()
    ctx = L.CMAC_CTX_new()
    try:
        assert L.CMAC_Init(ctx, bytes(key), len(key), (L.EVP_aes_128_cbc if len(key) == 16 else L.EVP_aes_256_cbc)(), None) == 1
        if msg:
            assert L.CMAC_Update(ctx, bytes(msg), len(msg)) == 1
        out, n = ctypes.create_string_buffer(16), ctypes.c_size_t(0)
        assert L.CMAC_Final(ctx, out, ctypes.byref(n)) == 1 and n.value == 16
        return out.raw
    finally:
        L.CMAC_CTX_free(ctx)


def kdf(key, label, context, bits):
    assert bits % 8 == 0 and 0 < bits < 1 << 16
    k, out, i = _Key(key), b"", 1
    while 8 * len(out) < bits:
        out += cmac(key, bytes([i]) + label + b"\x00" + bytes(context) + struct.pack(">H", bits), k)
        i += 1
    return out[:bits // 8]


def keyid(ckn):
    assert 1 <= len(ckn) <= 32
    return bytes(ckn)[:16].ljust(16, b"\0")


def kek(cak, ckn):
    return kdf(cak, LABEL_KEK, keyid(ckn), 8 * len(cak))


def sak_context(ks_nonce, mis, kn):
    """KS-nonce | MI-value list | be32(KN): the nonce of the SAK's length, every member identifier 12 bytes"""
    assert all(len(mi) == 12 for mi in mis)
    return bytes(ks_nonce) + b"".join(bytes(mi) for mi in mis) + struct.pack(">I", kn)


def sak(cak, context, key_len):
    assert 1 <= len(context) <= CTX_MAX and key_len in (16, 32)
    return kdf(cak, LABEL_SAK, context, 8 * key_len)


def wrap(kek_, key):
    """RFC 3394 2.2.1, the default initial value"""
    out = ctypes.create_string_buffer(len(key) + 8)
    assert _load().AES_wrap_key(_Key(kek_).buf, None, out, bytes(key), len(key)) == len(key) + 8
    return out.raw


def unwrap(kek_, wrapped):
    """RFC 3394 2.2.2 -> the key, or None where the integrity check fails"""
    out = ctypes.create_string_buffer(len(wrapped) - 8)
    n = _load().AES_unwrap_key(_Key(kek_, True).buf, None, out, bytes(wrapped), len(wrapped))
    return out.raw if n == len(wrapped) - 8 else None


def wrapped_sak(cak, ckn, context, key_len):
    """what a key server sends: the SAK under the KEK"""
    return wrap(kek(cak, ckn), sak(cak, context, key_len))


def vectors():
    return golden("mka_vectors.json")
