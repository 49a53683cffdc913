"""What tests/test_srtp_cpu.py and tests/test_gpu_srtp.py share: SRTP and SRTCP packet protection under RFC 7714's AEAD_AES_128_GCM / AEAD_AES_256_GCM in plain Python
over libcrypto (oracle.libcrypto_ref), written from RFC 7714 and RFC 3711 and from nothing else -- it is the GPU's reference and does not import the library.
SRTP (RFC 7714 8, 9; RFC 3711 3.1): rtp_hdr | payload | tag[16] | mki.  The header is 12 bytes, 4 per CSRC, and with the X bit an extension of 4 bytes and 4 times its
16-bit length field.  AAD = the header; nonce = salt XOR (00 00 | SSRC | ROC | SEQ).
SRTCP (RFC 7714 9.2 - 10; RFC 3711 3.4): rtcp_hdr[8] | payload | tag[16] | W[4] | mki, W = E | 31-bit index.  Nonce = salt XOR (00 00 | SSRC | 00 00 | 0, index).  E set:
AAD = the header | W, the payload is encrypted; E clear: AAD = everything in front of the tag | W, nothing is encrypted.
The MKI is passed through and is not authenticated.  tests/golden/srtp_rfc7714.json pins the fixture to RFC 7714's test vectors (sections 16 and 17); SRTCP with E
clear has no vector there and rests on the formulas."""
import struct

from oracle import libcrypto_ref as R

from util import golden

RTP, RTCP = 1, 2


def rtp_hdr_len(pkt):
    """the RTP header's length as the packet says it: CSRC count, X bit, the extension's own length field"""
    hdr = 12 + 4 * (pkt[0] & 15)
    if pkt[0] & 0x10:
        hdr += 4 + 4 * int.from_bytes(pkt[hdr + 2:hdr + 4], "big")
    return hdr


def rtp_header(cc, ext_words, seq, ts, ssrc, fill, pt=96, marker=0, padding=0):
    """V = 2 | P | X | CC, M | PT, sequence number, timestamp, SSRC, cc CSRCs, and with ext_words not None an extension of that many words -- CSRCs, the extension's
    profile bytes and its words taken from `fill`"""
    x = ext_words is not None
    h = bytes([0x80 | (0x20 if padding else 0) | (0x10 if x else 0) | cc, (marker << 7) | pt]) + struct.pack(">HII", seq, ts, ssrc) + fill[:4 * cc]
    if x:
        h += fill[60:62] + struct.pack(">H", ext_words) + fill[64:64 + 4 * ext_words]
    return h


def nonce_rtp(salt, pkt, roc):
    return bytes(a ^ b for a, b in zip(salt, bytes(2) + pkt[8:12] + struct.pack(">I", roc) + pkt[2:4]))


def nonce_rtcp(salt, pkt, w):
    return bytes(a ^ b for a, b in zip(salt, bytes(2) + pkt[4:8] + bytes(2) + struct.pack(">I", w & 0x7FFFFFFF)))


def _rtcp_parts(pkt, mki_len):
    """-> (where the tag starts, W)"""
    t = len(pkt) - mki_len - 20
    return t, int.from_bytes(pkt[t + 16:t + 20], "big")


def protect_rtp(key, salt, roc, pkt, mki_len=0):
    """pkt = header | plaintext | 16 placeholder bytes | mki -> the packet on the wire"""
    h, t = rtp_hdr_len(pkt), len(pkt) - mki_len - 16
    ct, tag = R.encrypt(key, nonce_rtp(salt, pkt, roc), pkt[:h], pkt[h:t])
    return pkt[:h] + bytes(ct) + bytes(tag) + pkt[t + 16:]


def unprotect_rtp(key, salt, roc, pkt, mki_len=0):
    """-> (header | plaintext | the tag as it came | mki, authentic)"""
    h, t = rtp_hdr_len(pkt), len(pkt) - mki_len - 16
    pt, ok = R.decrypt(key, nonce_rtp(salt, pkt, roc), pkt[:h], pkt[h:t], pkt[t:t + 16])
    return pkt[:h] + bytes(pt) + pkt[t:], bool(ok)


def protect_rtcp(key, salt, pkt, mki_len=0):
    """pkt = header[8] | plaintext | 16 placeholder bytes | W | mki, W as the sender wrote it -> the packet on the wire"""
    t, w = _rtcp_parts(pkt, mki_len)
    if w >> 31:
        ct, tag = R.encrypt(key, nonce_rtcp(salt, pkt, w), pkt[:8] + pkt[t + 16:t + 20], pkt[8:t])
        return pkt[:8] + bytes(ct) + bytes(tag) + pkt[t + 16:]
    _, tag = R.encrypt(key, nonce_rtcp(salt, pkt, w), pkt[:t] + pkt[t + 16:t + 20], b"")
    return pkt[:t] + bytes(tag) + pkt[t + 16:]


def unprotect_rtcp(key, salt, pkt, mki_len=0):
    """-> (header | plaintext | the tag as it came | W | mki, authentic)"""
    t, w = _rtcp_parts(pkt, mki_len)
    if w >> 31:
        pt, ok = R.decrypt(key, nonce_rtcp(salt, pkt, w), pkt[:8] + pkt[t + 16:t + 20], pkt[8:t], pkt[t:t + 16])
        return pkt[:8] + bytes(pt) + pkt[t:], bool(ok)
    _, ok = R.decrypt(key, nonce_rtcp(salt, pkt, w), pkt[:t] + pkt[t + 16:t + 20], b"", pkt[t:t + 16])
    return pkt, bool(ok)


def protect(kind, key, salt, roc, pkt, mki_len=0):
    return protect_rtp(key, salt, roc, pkt, mki_len) if kind == RTP else protect_rtcp(key, salt, pkt, mki_len)


def unprotect(kind, key, salt, roc, pkt, mki_len=0):
    return unprotect_rtp(key, salt, roc, pkt, mki_len) if kind == RTP else unprotect_rtcp(key, salt, pkt, mki_len)


def vectors():
    """tests/golden/srtp_rfc7714.json -> [(name, kind, key, salt, roc, plain packet with placeholder tag, nonce, wire packet)]"""
    out = []
    for v in golden("srtp_rfc7714.json")["vectors"]:
        kind = RTP if v["kind"] == "rtp" else RTCP
        wire = bytes.fromhex(v["wire"])
        plain = bytes.fromhex(v["packet"]) + b"\xAA" * 16 + (bytes.fromhex(v["w"]) if kind == RTCP else b"")
        out.append((v["name"], kind, bytes.fromhex(v["key"]), bytes.fromhex(v["salt"]), v.get("roc", 0), plain, bytes.fromhex(v["nonce"]), wire))
    return out
