"""What tests/test_ssh_cpu.py and tests/test_gpu_ssh.py share: SSH's AES-GCM packet protection (RFC 5647 7.1 - 7.3; OpenSSH PROTOCOL 1.6) and its key derivation
(RFC 4253 7.2) written from the RFCs' formulas in plain Python -- the nonce and the AAD of a packet here, the AEAD itself by libcrypto (kt_common.evp_by_slot, the
fixture the other wire tests use), the hash by hashlib.  No published AES-GCM SSH packet vector and no KDF vector is at hand: this rests on the formulas
(tests/COVERAGE_ssh.md)."""
import hashlib
import struct

from util import splitmix_bytes

HASH = {32: hashlib.sha256, 48: hashlib.sha384, 64: hashlib.sha512}
MASK64 = (1 << 64) - 1


# ---------------------------------------------------------------- packets
def nonce_of(iv, seq):
    """RFC 5647 7.1: fixed[4] | invocation_counter[8], the counter a big-endian integer incremented once per packet, modulo 2^64; the fixed field stays"""
    assert len(iv) == 12
    return iv[:4] + struct.pack(">Q", (struct.unpack(">Q", iv[4:])[0] + seq) & MASK64)


def nonce_xor(iv, seq):
    """what TLS 1.3 would make of the same inputs: the tests hold the two apart"""
    return bytes(a ^ b for a, b in zip(iv, bytes(4) + struct.pack(">Q", seq)))


def packet(body):
    """a plaintext packet around `body` (padding_length | payload | padding, a whole number of cipher blocks): the length field written, the tag's bytes placeholders"""
    return struct.pack(">I", len(body)) + body + b"\xAA" * 16


def make_packets(seed, bodies):
    blob = splitmix_bytes(seed, sum(bodies))
    out, at = [], 0
    for b in bodies:
        out.append(packet(blob[at:at + b]))
        at += b
    return out


def split(pkt):
    """-> (aad, body): the four length bytes in the clear, and what lies between them and the tag"""
    return pkt[:4], pkt[4:-16]


def refused(pkt):
    """RFC 5647 7.2 / 7.3 by length alone, then the field: shorter than one cipher block of body, a body that is no whole number of blocks, a length field that
    says something else"""
    body = len(pkt) - 20
    return len(pkt) < 36 or body % 16 != 0 or struct.unpack(">I", pkt[:4])[0] != body


def ref_encrypt(evp, key_len, keys, ivs, slots, seqs, pkts, nonce=nonce_of):
    from kt_common import evp_by_slot
    return evp_by_slot(evp, key_len, keys, slots, [(nonce(ivs[s], q),) + split(p) for s, q, p in zip(slots, seqs, pkts)], pkts, 16)


# ---------------------------------------------------------------- RFC 4253 7.2
def mpint(x):
    """RFC 4251 5: K as the DH and ECDH exchanges put it into the hash"""
    b = x.to_bytes((x.bit_length() + 8) // 8, "big") if x else b""
    return struct.pack(">I", len(b)) + b


def kdf(hash_len, secret, session_id, letter, n):
    """HASH(K | H | letter | session_id), its first n bytes; secret = K_enc | H.  n <= hash_len: the extension K2 = HASH(K | H | K1) is never needed here"""
    assert n <= hash_len and len(session_id) == hash_len and len(letter) == 1
    return HASH[hash_len](secret + letter + session_id).digest()[:n]


def derive(hash_len, secret, session_id, key_len):
    """-> ((key, iv) client to server, (key, iv) server to client)"""
    return ((kdf(hash_len, secret, session_id, b"C", key_len), kdf(hash_len, secret, session_id, b"A", 12)),
            (kdf(hash_len, secret, session_id, b"D", key_len), kdf(hash_len, secret, session_id, b"B", 12)))
