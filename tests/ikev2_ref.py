"""IKEv2's prf+ and the ESP AES-GCM cut of KEYMAT in plain Python over hmac: the reference of tests/test_prfplus_cpu.py and tests/test_gpu_prfplus.py.

It rests on RFC 7296's formula alone (2.13: prf+(K, S) = T1 | T2 | ..., T1 = prf(K, S | 0x01), Tn = prf(K, T(n-1) | S | n)); the cut is RFC 7296 2.17 (the
initiator-to-responder SA first) and RFC 4106 8.1 (the key, then its four salt bytes).  No published prf+ vector stands behind it: tests/COVERAGE_prfplus.md."""
import hashlib
import hmac

HASH = {32: hashlib.sha256, 48: hashlib.sha384, 64: hashlib.sha512}
I2R, R2I = 0, 1


def prf_plus(hash_len, key, seed, n):
    """the first n bytes of prf+(key, seed) under HMAC-SHA-256 / -384 / -512 by hash_len"""
    out, t, ctr = b"", b"", 1
    while len(out) < n:
        assert ctr < 256
        t = hmac.new(key, t + seed + bytes([ctr]), HASH[hash_len]).digest()
        out, ctr = out + t, ctr + 1
    return out[:n]


def child_sa(hash_len, sk_d, seed, key_len):
    """KEYMAT of one Child SA -> ((key_i2r, salt_i2r), (key_r2i, salt_r2i))"""
    km = prf_plus(hash_len, sk_d, seed, 2 * (key_len + 4))
    return tuple((km[d * (key_len + 4):d * (key_len + 4) + key_len], km[d * (key_len + 4) + key_len:(d + 1) * (key_len + 4)]) for d in (I2R, R2I))
