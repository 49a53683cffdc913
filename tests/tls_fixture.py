"""What tests/test_tls_cpu.py and tests/test_gpu_tls.py share: tests/golden/tls_records.json (records of a real TLS stack, tests/golden/gen_tls_records.py), the key
derivations of RFC 8446 section 7.3 and RFC 5246 section 6.3 written with hmac and hashlib, and nonce and AAD of a record by the formulas of RFC 8446 5.2 / 5.3 and
RFC 5288 3 / RFC 5246 6.2.3.3 in plain Python."""
import base64
import hashlib
import hmac
import struct

from util import golden, splitmix_bytes

TLS13, TLS12 = 1, 2
HDR = {TLS13: 5, TLS12: 13}           # the bytes in front of the payload: the record header, and TLS 1.2's explicit nonce


def hkdf_expand_label(hname, secret, label, length):
    """RFC 8446 7.1 with an empty context; HKDF-Expand is RFC 5869 2.3"""
    full = b"tls13 " + label
    info = struct.pack(">HB", length, len(full)) + full + b"\0"
    out, t, i = b"", b"", 1
    while len(out) < length:
        t = hmac.new(secret, t + info + bytes([i]), hname).digest()
        out += t
        i += 1
    return out[:length]


def prf12(hname, secret, label, seed, length):
    """RFC 5246 5: P_hash(secret, label + seed)"""
    seed = label + seed
    out, a = b"", seed
    while len(out) < length:
        a = hmac.new(secret, a, hname).digest()
        out += hmac.new(secret, a + seed, hname).digest()
    return out[:length]


def derive(conn, who):
    """-> (write key, 12-byte slot IV) of one direction ("client" / "server"); TLS 1.2's write IV is four bytes, the slot's other eight are not used"""
    kl, hname = conn["key_len"], conn["hash"]
    if conn["version"] == "1.3":
        secret = bytes.fromhex(conn["dirs"][who]["traffic_secret"])
        return hkdf_expand_label(hname, secret, b"key", kl), hkdf_expand_label(hname, secret, b"iv", 12)
    block = prf12(hname, bytes.fromhex(conn["master_secret"]), b"key expansion", bytes.fromhex(conn["server_random"]) + bytes.fromhex(conn["client_random"]), 2 * kl + 8)
    i = 0 if who == "client" else 1                       # client_write_key | server_write_key | client_write_IV | server_write_IV (an AEAD suite has no MAC keys)
    return block[i * kl:(i + 1) * kl], block[2 * kl + 4 * i:2 * kl + 4 * i + 4] + bytes(8)


def nonce_of(ver, iv, seq, rec):
    if ver == TLS13:
        return bytes(a ^ b for a, b in zip(iv, bytes(4) + struct.pack(">Q", seq)))
    return iv[:4] + rec[5:13]


def aad_of(ver, seq, rec):
    if ver == TLS13:
        return rec[:5]
    return struct.pack(">Q", seq) + rec[:3] + struct.pack(">H", len(rec) - 29)


def version_of(conn):
    return TLS13 if conn["version"] == "1.3" else TLS12


def directions():
    """every (connection, direction) of the fixture: (conn, who, ver, key, iv, [(seq, wire record, plaintext as the record layer encrypted it)])"""
    out = []
    for conn in golden("tls_records.json")["connections"]:
        ver = version_of(conn)
        for who in ("client", "server"):
            key, iv = derive(conn, who)
            recs = []
            for r in conn["dirs"][who]["records"]:
                pt = splitmix_bytes(r["seed"], r["len"]) + (b"\x17" if ver == TLS13 else b"")          # TLSInnerPlaintext: content | type, no padding
                recs.append((r["seq"], base64.b64decode(r["wire"]), pt))
            out.append((conn, who, ver, key, iv, recs))
    return out
