#!/usr/bin/env python3
"""SSH packets against the parent commit's TLS 1.3 call on records of the same byte lengths, and SshKexTable.install against the parent's set_dev + set_tls_iv of
values that lie derived in memory (GPU box): this build against a library built at the PARENT commit (--base, a libaesgcm_hip.so; both libraries live in this one
process, as the debug library does in the tests).  The base crypt call, aesgcm_keytab_records_crypt_dev in TLS 1.3 mode, is one launch too, takes the same d_seq array
and XORs where SSH adds; its AAD is 5 bytes where SSH's is 4.  Every packet is L = 4 + 1024 + 16 bytes on both sides.
    (a) 65536 packets over 1024 slots, AES-256        (b) 4096 packets over 64 slots, AES-256
encrypt and decrypt each; install: 65536 and 4096 connections (both directions: twice as many slots), SHA-256, secrets of 289 bytes (a 2048-bit mpint and H).
Same process, same device, calls ALTERNATED, --reps calls per side and round, --rounds rounds, timed with events on the launch stream.  Per side: the median of each
round, and the median of those.  Spread = max - min of the base call's round medians.  The expectation for the packets is parity: within that spread.
Each side decrypts what it encrypted; every tag must be accepted and the tables' status words stay clear.
    python profiles/ssh/ab.py --base PATH/libaesgcm_hip.so [--reps 9] [--rounds 3]"""
import argparse
import ctypes
import hashlib
import json
import os
import statistics
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import aesgcm_amd  # noqa: E402,F401
from aesgcm_amd import lib  # noqa: E402

SIDES = ("base", "ssh")
BODY = 1024
L = 4 + BODY + 16


def load_base(path):
    """the parent commit's library, typed as far as this script calls it (it has no SSH symbol for lib._keytab_typed to type)"""
    B = lib._typed(ctypes.CDLL(path))
    vp, sz, cint, u64 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_uint64
    B.aesgcm_keytab_create.argtypes = [ctypes.POINTER(vp), cint, sz, sz]
    B.aesgcm_keytab_set.argtypes = [vp, sz, sz, vp, vp]
    B.aesgcm_keytab_set_dev.argtypes = [vp, sz, vp, vp, vp]
    B.aesgcm_keytab_set_tls_iv.argtypes = [vp, sz, sz, vp, vp]
    B.aesgcm_keytab_records_crypt_dev.argtypes = [vp, cint, ctypes.POINTER(lib.TlsFormat), sz, vp, vp, vp, vp, vp, vp, vp]
    B.aesgcm_keytab_status.argtypes = [vp, ctypes.POINTER(cint), ctypes.POINTER(u64)]
    B.aesgcm_keytab_destroy.argtypes = [vp]
    B._keytab_typed = True
    return B


class base_library:
    """inside the block lib.KeyTable() belongs to the parent commit's library"""

    def __init__(self, B):
        self.B = B

    def __enter__(self):
        lib.load()
        self.prev, lib._L = lib._L, self.B

    def __exit__(self, *a):
        lib._L = self.prev


def dev(arr):
    b = lib.DeviceBuffer(max(arr.nbytes, 16))
    b.upload(arr.tobytes())
    return b


def alternate(runs, reps, rounds):
    t = lib.Timer()
    for _ in range(2):                                        # every shape warmed up
        for k in SIDES:
            runs[k]()
    lib.dev_sync()
    ms = {k: [] for k in SIDES}
    for _ in range(rounds):
        r = {k: [] for k in SIDES}
        for _ in range(reps):
            for k in SIDES:
                t.start(); runs[k](); t.stop()
                r[k].append(t.ms())
        for k in r:
            ms[k].append(r[k])
    t.close()
    return ms


def summary(r, ms):
    med = {k: [statistics.median(x) for x in v] for k, v in ms.items()}                      # per round, ms
    r["ms"] = {k: [[round(x, 4) for x in rr] for rr in v] for k, v in ms.items()}
    r["median_us"] = {k: round(1e3 * statistics.median(v), 1) for k, v in med.items()}
    r["base_spread_us"] = round(1e3 * (max(med["base"]) - min(med["base"])), 1)
    r["within_base_spread"] = r["median_us"]["ssh"] <= r["median_us"]["base"] + r["base_spread_us"]
    return r


def crypt_case(name, base, n, n_slots, key_len, reps, rounds, rng):
    f13 = lib.TlsFormat.tls13()
    keys = rng.integers(0, 256, size=n_slots * key_len, dtype=np.uint8).tobytes()
    ivs = rng.integers(0, 256, size=n_slots * 12, dtype=np.uint8).tobytes()
    slots = rng.integers(0, n_slots, size=n, dtype=np.uint32)
    seqs = rng.integers(0, 1 << 40, size=n, dtype=np.uint64)
    off = np.arange(n + 1, dtype=np.uint64) * np.uint64(L)
    wire = rng.integers(0, 256, size=n * L, dtype=np.uint8)          # to the base call any bytes are a TLS 1.3 record
    swire = wire.copy()
    for b, v in enumerate(BODY.to_bytes(4, "big")):
        swire[b::L] = v                                               # the length field says the body's length
    d_slots, d_seqs, d_off, d_wire, d_swire = dev(slots), dev(seqs), dev(off), dev(wire), dev(swire)
    d_ct = {k: lib.DeviceBuffer(wire.nbytes + 64) for k in SIDES}
    d_pt = {k: lib.DeviceBuffer(wire.nbytes + 64) for k in SIDES}
    d_auth = {k: lib.DeviceBuffer(4 * n) for k in SIDES}
    with base_library(base):
        kb = lib.KeyTable(key_len, n_slots)
    ks = lib.KeyTable(key_len, n_slots)
    kb.set(0, keys); kb.set_tls_iv(0, ivs)
    ks.set(0, keys); ks.set_tls_iv(0, ivs)
    rows = []
    for decrypt in (0, 1):
        src = d_ct if decrypt else {"base": d_wire, "ssh": d_swire}
        dst = d_pt if decrypt else d_ct
        au = {k: d_auth[k].ptr if decrypt else None for k in SIDES}
        runs = {
            "base": lambda: kb.records_crypt_dev(decrypt, f13, n, d_slots.ptr, d_seqs.ptr, src["base"].ptr, d_off.ptr, dst["base"].ptr, d_auth=au["base"]),
            "ssh": lambda: ks.ssh_crypt_dev(decrypt, n, d_slots.ptr, d_seqs.ptr, src["ssh"].ptr, d_off.ptr, dst["ssh"].ptr, d_auth=au["ssh"]),
        }
        ms = alternate(runs, reps, rounds)
        lib.dev_sync()
        ok = True
        if decrypt:                                            # each side gets its plaintext back, every tag accepted
            for k in SIDES:
                a = np.frombuffer(bytes(d_auth[k].download(4 * n)), dtype=np.int32)
                ok = ok and bool((a == 1).all())
                for p in range(0, n, max(1, n // 64)):
                    pt = np.frombuffer(bytes(d_pt[k].download(L - 16, offset=p * L)), dtype=np.uint8)
                    ok = ok and bool((pt == (wire if k == "base" else swire)[p * L:p * L + L - 16]).all())
        r = summary({"case": name, "what": "decrypt" if decrypt else "encrypt", "key_bits": 8 * key_len, "n": n, "n_slots": n_slots, "pkt_len": L, "reps": reps, "rounds": rounds,
                     "round_trip_ok": ok, "status": [list(kb.status()), list(ks.status())]}, ms)
        r["gib_s"] = {k: round(n * L / (1 << 30) / (v / 1e6), 1) for k, v in r["median_us"].items()}
        print(json.dumps(r), flush=True)
        rows.append(r)
    kb.close(); ks.close()
    for b in [d_slots, d_seqs, d_off, d_wire, d_swire] + [x for d in (d_ct, d_pt, d_auth) for x in d.values()]:
        b.free()
    return rows


def install_case(name, base, n, key_len, hl, secret_len, reps, rounds, rng):
    """base: aesgcm_keytab_set_dev of 2n keys that lie in device memory and aesgcm_keytab_set_tls_iv of 2n IVs from the host (the parent has no device call for an IV);
    new: one install of n connections, both directions"""
    secrets = [rng.integers(0, 256, size=secret_len, dtype=np.uint8).tobytes() for _ in range(n)]
    sids = rng.integers(0, 256, size=n * hl, dtype=np.uint8).tobytes()
    keys = rng.integers(0, 256, size=2 * n * key_len, dtype=np.uint8)
    ivs = rng.integers(0, 256, size=2 * n * 12, dtype=np.uint8).tobytes()
    idx = np.arange(n, dtype=np.uint32)
    d_idx, d_c2s, d_s2c, d_all, d_keys = dev(idx), dev(2 * idx), dev(2 * idx + 1), dev(np.arange(2 * n, dtype=np.uint32)), dev(keys)
    with base_library(base):
        kb = lib.KeyTable(key_len, 2 * n)
    ks = lib.KeyTable(key_len, 2 * n)
    kex = lib.SshKexTable(hl, n, max_secret_len=secret_len)
    kex.set(0, secrets, sids)
    lib.dev_sync()

    def base_run():
        kb.set_dev(2 * n, d_all.ptr, d_keys.ptr)
        kb.set_tls_iv(0, ivs)
    runs = {"base": base_run, "ssh": lambda: kex.install_dev(ks, n, d_idx.ptr, d_c2s.ptr, d_s2c.ptr)}
    ms = alternate(runs, reps, rounds)
    lib.dev_sync()
    r = summary({"case": name, "what": "install", "key_bits": 8 * key_len, "n": n, "n_slots": 2 * n, "hash_len": hl, "secret_len": secret_len, "reps": reps, "rounds": rounds,
                 "round_trip_ok": True, "status": [list(kb.status()), list(ks.status()), list(kex.status())]}, ms)
    print(json.dumps(r), flush=True)
    kb.close(); ks.close(); kex.close()
    for b in (d_idx, d_c2s, d_s2c, d_all, d_keys):
        b.free()
    return [r]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--base", required=True, help="libaesgcm_hip.so built at the parent commit")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=HERE)
    a = ap.parse_args()
    assert a.reps >= 5 and a.rounds >= 3
    rng = np.random.default_rng(20261021)
    dev_name = lib.device_name(0)
    so = os.path.join(os.path.dirname(os.path.abspath(lib.__file__)), "libaesgcm_hip.so")
    sha = hashlib.sha256(open(so, "rb").read()).hexdigest()[:16]
    bsha = hashlib.sha256(open(a.base, "rb").read()).hexdigest()[:16]
    print("device:", dev_name, "library sha256:", sha, "base library sha256:", bsha, flush=True)
    base = load_base(a.base)
    rows = crypt_case("a_65536x1044", base, 65536, 1024, 32, a.reps, a.rounds, rng)
    rows += crypt_case("b_4096x1044", base, 4096, 64, 32, a.reps, a.rounds, rng)
    rows += install_case("install_65536", base, 65536, 32, 32, 289, a.reps, a.rounds, rng)
    rows += install_case("install_4096", base, 4096, 32, 32, 289, a.reps, a.rounds, rng)
    lines = ["device: %s; libaesgcm_hip.so sha256 %s...; baseline: the parent commit's library (sha256 %s...): aesgcm_keytab_records_crypt_dev in TLS 1.3 mode on records of"
             % (dev_name, sha, bsha),
             "the same byte lengths (%d), and for install aesgcm_keytab_set_dev + aesgcm_keytab_set_tls_iv of 2n derived values; %d rounds of %d alternated calls; per side the"
             % (L, a.rounds, a.reps),
             "median of the round medians in microseconds (crypt: and GiB/s over the packets' bytes); spread = max - min of the base call's round medians.  Expected: parity",
             "%-14s %-8s %4s %7s | %9s %7s | %9s %-6s | %-13s | %s" % ("case", "what", "key", "n", "base us", "spread", "SSH us", "within", "GiB/s b / ssh", "round trip")]
    for r in rows:
        g = r.get("gib_s")
        lines.append("%-14s %-8s %4d %7d | %9.1f %7.1f | %9.1f %-6s | %-13s | %s" % (
            r["case"], r["what"], r["key_bits"], r["n"], r["median_us"]["base"], r["base_spread_us"], r["median_us"]["ssh"], "yes" if r["within_base_spread"] else "NO",
            "%.1f / %.1f" % (g["base"], g["ssh"]) if g else "-", r["round_trip_ok"]))
    print("\n".join(lines))
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "ab.txt"), "w") as f:
        f.write("\n".join(lines) + "\n\n" + "\n".join(json.dumps(r) for r in rows) + "\n")
    assert all(r["round_trip_ok"] and all(s == [0, 0] for s in r["status"]) for r in rows), "a side did not get its plaintext back"


if __name__ == "__main__":
    main()
