"""What tests/test_srtp_kdf_cpu.py and tests/test_gpu_srtp_kdf.py share: SRTP's key derivation (RFC 3711 4.3.1; RFC 6188 for AES-192 / AES-256 master keys; the labels
RFC 7714 11 uses) in plain Python over libcrypto's AES (quic_fixture.aes_ecb) -- it is the library's reference and does not import it.
    x      = master_salt XOR (0^56 | label | be48(r)), 14 bytes; r = index DIV key_derivation_rate
    output = E_mk(x | be16(0)) | E_mk(x | be16(1)) | ..., truncated
tests/golden/srtp_kdf_rfc.json pins it to RFC 3711 B.3 (AES-128), RFC 6188 7.2 (AES-192) and RFC 6188 7.1 (AES-256): r = 0, labels 0x00 and 0x02.  No published vector
with r != 0 or with the SRTCP labels 0x03 / 0x05 is at hand: those rest on the formula."""
import srtp_fixture as S
from quic_fixture import aes_ecb
from util import golden

LABEL_KEY = {S.RTP: 0x00, S.RTCP: 0x03}
LABEL_SALT = {S.RTP: 0x02, S.RTCP: 0x05}
R_END = 1 << 48


def pad_salt(salt):
    """a master salt as the PRF takes it: 14 bytes, an AEAD profile's 12 with two zero bytes appended (times 2^16)"""
    assert len(salt) in (12, 14)
    return bytes(salt).ljust(14, b"\0")


def prf(master_key, master_salt, label, r, n):
    """the first n bytes of the key-derivation PRF's output"""
    assert len(master_key) in (16, 24, 32) and 0 <= label < 256 and 0 <= r < R_END
    x = int.from_bytes(pad_salt(master_salt), "big") ^ (label << 48) ^ r
    out = b""
    for j in range((n + 15) // 16):
        out += aes_ecb(bytes(master_key), x.to_bytes(14, "big") + j.to_bytes(2, "big"))
    return out[:n]


def session(kind, master_key, master_salt, r=0):
    """-> (session key of the master key's size, the session salt's first 12 bytes: what a key-table slot holds)"""
    return prf(master_key, master_salt, LABEL_KEY[kind], r, len(master_key)), prf(master_key, master_salt, LABEL_SALT[kind], r, 12)


def vectors():
    """tests/golden/srtp_kdf_rfc.json -> [(name, master key, master salt, session key, session salt of 14 bytes)]"""
    return [(v["name"],) + tuple(bytes.fromhex(v[k]) for k in ("master_key", "master_salt", "session_key", "session_salt")) for v in golden("srtp_kdf_rfc.json")["vectors"]]
