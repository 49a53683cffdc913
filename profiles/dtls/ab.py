#!/usr/bin/env python3
"""DTLS records against the parent commit's calls on records of the same byte lengths (GPU box): aesgcm_keytab_dtls_crypt_dev of this build against a library built at
the PARENT commit (--base, a libaesgcm_hip.so; both libraries live in this one process, as the debug library does in the tests).  DTLS 1.2 against the parent's
aesgcm_keytab_records_crypt_dev in TLS 1.2 mode (one launch each; 21 against 13 bytes in front of the payload), DTLS 1.3 against the parent's aesgcm_keytab_quic_crypt_dev
(two launches each; a unified header with an 8-byte connection ID, a 2-byte sequence number and no length field is 11 bytes, as the short QUIC header with pn_off 9 and
pn_len 2).  Every record is L bytes on both sides and ends in 16 bytes of tag.
    (a) 65536 records of 1350 bytes over 1024 AEAD slots (and 16 sn / hp slots), AES-256        (b) 4096 records of 1350 bytes over 64 slots, AES-256
encrypt and decrypt each.  Same process, same device, calls ALTERNATED, --reps calls per side and round, --rounds rounds, timed with events on the launch stream.  Per
side: the median of each round, and the median of those.  Spread = max - min of the base call's round medians.  The expectation is parity: within that spread.
Each side decrypts what it encrypted; every tag must be accepted, every number decoded, and the tables' status words stay clear.
    python profiles/dtls/ab.py --base PATH/libaesgcm_hip.so [--reps 9] [--rounds 3] [--once]"""
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

SIDES = ("base", "dtls")
PN_OFF, PN_LEN = 9, 2


def load_base(path):
    """the parent commit's library, typed as far as this script calls it (it has no DTLS symbol for lib._keytab_typed to type)"""
    L = lib._typed(ctypes.CDLL(path))
    vp, sz, cint, u64 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_uint64
    L.aesgcm_keytab_create.argtypes = [ctypes.POINTER(vp), cint, sz, sz]
    L.aesgcm_keytab_set.argtypes = [vp, sz, sz, vp, vp]
    L.aesgcm_keytab_set_tls_iv.argtypes = [vp, sz, sz, vp, vp]
    L.aesgcm_keytab_records_crypt_dev.argtypes = [vp, cint, ctypes.POINTER(lib.TlsFormat), sz, vp, vp, vp, vp, vp, vp, vp]
    L.aesgcm_keytab_quic_crypt_dev.argtypes = [vp, cint, sz, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.aesgcm_keytab_status.argtypes = [vp, ctypes.POINTER(cint), ctypes.POINTER(u64)]
    L.aesgcm_keytab_destroy.argtypes = [vp]
    L._keytab_typed = True
    return L


class base_library:
    """inside the block lib.KeyTable() belongs to the parent commit's library"""

    def __init__(self, L):
        self.L = L

    def __enter__(self):
        lib.load()
        self.prev, lib._L = lib._L, self.L

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


def case(name, ver, base, n, n_slots, key_len, L, reps, rounds, rng, once):
    n_hp = 16
    v13 = ver == lib.DTLS_13
    f12, fd = lib.TlsFormat.tls12(), lib.DtlsFormat(ver, 0)
    keys = rng.integers(0, 256, size=(n_slots + n_hp) * key_len, dtype=np.uint8).tobytes()
    ivs = rng.integers(0, 256, size=n_slots * 12, dtype=np.uint8).tobytes()
    slots = rng.integers(0, n_slots, size=n, dtype=np.uint32)
    hps = (n_slots + rng.integers(0, n_hp, size=n)).astype(np.uint32)
    pns = rng.integers(0, 1 << 62, size=n, dtype=np.uint64)
    off = np.arange(n + 1, dtype=np.uint64) * np.uint64(L)
    wire = rng.integers(0, 256, size=n * L, dtype=np.uint8)
    wire[0::L] = 0x40 | (PN_LEN - 1)                                  # a short QUIC header with a two-byte packet number,
    wire[PN_OFF::L] = ((pns >> np.uint64(8)) & np.uint64(0xFF)).astype(np.uint8)    # truncated and written by the caller
    wire[PN_OFF + 1::L] = (pns & np.uint64(0xFF)).astype(np.uint8)
    dwire = wire.copy()
    dwire[0::L] = 0x20 | 0x10 | 0x08 | 0x01                           # the same bytes as a DTLS 1.3 record: C and S set, no length field, epoch 1
    d_slots, d_hps, d_pns, d_off, d_wire, d_dwire = dev(slots), dev(hps), dev(pns), dev(off), dev(wire), dev(dwire)
    d_pn_off = dev(np.full(n, PN_OFF, dtype=np.uint32))
    d_pn_out = lib.DeviceBuffer(8 * n)
    d_ct = {k: lib.DeviceBuffer(wire.nbytes + 64) for k in SIDES}
    d_pt = {k: lib.DeviceBuffer(wire.nbytes + 64) for k in SIDES}
    d_auth = {k: lib.DeviceBuffer(4 * n) for k in SIDES}
    with base_library(base):
        kb = lib.KeyTable(key_len, n_slots + n_hp)
    kq = lib.KeyTable(key_len, n_slots + n_hp)
    kb.set(0, keys); kb.set_tls_iv(0, ivs)
    kq.set(0, keys); kq.set_tls_iv(0, ivs)
    rows = []
    for decrypt in (0, 1):
        src = d_ct if decrypt else {"base": d_wire, "dtls": d_dwire if v13 else d_wire}
        dst = d_pt if decrypt else d_ct
        au = {k: d_auth[k].ptr if decrypt else None for k in SIDES}
        if v13:
            runs = {
                "base": lambda: kb.quic_crypt_dev(decrypt, n, d_slots.ptr, d_hps.ptr, d_pns.ptr, d_pn_off.ptr, src["base"].ptr, d_off.ptr, dst["base"].ptr,
                                                  d_pn_out=d_pn_out.ptr if decrypt else None, d_auth=au["base"]),
                "dtls": lambda: kq.dtls_crypt_dev(decrypt, fd, n, d_slots.ptr, src["dtls"].ptr, d_off.ptr, dst["dtls"].ptr, d_sn_slots=d_hps.ptr, d_seq=d_pns.ptr,
                                                  d_sn_off=d_pn_off.ptr, d_seq_out=d_pn_out.ptr if decrypt else None, d_auth=au["dtls"]),
            }
        else:
            runs = {
                "base": lambda: kb.records_crypt_dev(decrypt, f12, n, d_slots.ptr, d_pns.ptr, src["base"].ptr, d_off.ptr, dst["base"].ptr, d_auth=au["base"]),
                "dtls": lambda: kq.dtls_crypt_dev(decrypt, fd, n, d_slots.ptr, src["dtls"].ptr, d_off.ptr, dst["dtls"].ptr, d_auth=au["dtls"]),
            }
        if once:
            for k in SIDES:
                runs[k]()
            lib.dev_sync()
            continue
        ms = alternate(runs, reps, rounds)
        lib.dev_sync()
        ok = True
        if decrypt:                                            # each side gets its plaintext back, every tag accepted, every number decoded
            for k in SIDES:
                a = np.frombuffer(bytes(d_auth[k].download(4 * n)), dtype=np.int32)
                ok = ok and bool((a == 1).all())
                for p in range(0, n, max(1, n // 64)):
                    pt = np.frombuffer(bytes(d_pt[k].download(L - 16, offset=p * L)), dtype=np.uint8)
                    ok = ok and bool((pt == (dwire if v13 and k == "dtls" else wire)[p * L:(p + 1) * L - 16]).all())
            if v13:
                ok = ok and bool((np.frombuffer(bytes(d_pn_out.download(8 * n)), dtype=np.uint64) == pns).all())
        gib = n * (L - 16) / (1 << 30)
        rate = {k: [gib / (statistics.median(r) / 1e3) for r in v] for k, v in ms.items()}      # GiB/s, per round
        med_ms = {k: statistics.median(statistics.median(r) for r in v) for k, v in ms.items()}
        r = {"case": name, "version": "1.3" if v13 else "1.2", "op": "decrypt" if decrypt else "encrypt", "key_bits": 8 * key_len, "n_pkts": n, "n_slots": n_slots, "pkt_len": L,
             "reps": reps, "rounds": rounds, "ms": {k: [[round(x, 4) for x in rr] for rr in v] for k, v in ms.items()},
             "round_medians_gib_s": {k: [round(x, 1) for x in v] for k, v in rate.items()},
             "round_trip_ok": ok, "status": [list(kb.status()), list(kq.status())]}
        r["gib_s"] = {k: round(statistics.median(v), 1) for k, v in rate.items()}
        r["median_us"] = {k: round(1e3 * v, 1) for k, v in med_ms.items()}
        r["base_spread_gib_s"] = round(max(rate["base"]) - min(rate["base"]), 1)
        r["within_base_spread"] = r["gib_s"]["dtls"] >= r["gib_s"]["base"] - r["base_spread_gib_s"]
        print(json.dumps(r), flush=True)
        rows.append(r)
    kb.close(); kq.close()
    for b in [d_slots, d_hps, d_pns, d_off, d_wire, d_dwire, d_pn_off, d_pn_out] + [x for d in (d_ct, d_pt, d_auth) for x in d.values()]:
        b.free()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--base", required=True, help="libaesgcm_hip.so built at the parent commit")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--once", action="store_true", help="every call once and no file: for a kernel trace")
    ap.add_argument("--out", default=HERE)
    a = ap.parse_args()
    assert a.reps >= 5 and a.rounds >= 3
    rng = np.random.default_rng(20261017)
    dev_name = lib.device_name(0)
    so = os.path.join(os.path.dirname(os.path.abspath(lib.__file__)), "libaesgcm_hip.so")
    sha = hashlib.sha256(open(so, "rb").read()).hexdigest()[:16]
    bsha = hashlib.sha256(open(a.base, "rb").read()).hexdigest()[:16]
    print("device:", dev_name, "library sha256:", sha, "base library sha256:", bsha, flush=True)
    base = load_base(a.base)
    rows = []
    for ver in (lib.DTLS_12, lib.DTLS_13):
        rows += case("a_65536x1350", ver, base, 65536, 1024, 32, 1350, a.reps, a.rounds, rng, a.once)
        rows += case("b_4096x1350", ver, base, 4096, 64, 32, 1350, a.reps, a.rounds, rng, a.once)
    if a.once:
        return
    lines = ["device: %s; libaesgcm_hip.so sha256 %s...; baseline: the parent commit's library (sha256 %s...): aesgcm_keytab_records_crypt_dev (TLS 1.2) for DTLS 1.2,"
             % (dev_name, sha, bsha),
             "aesgcm_keytab_quic_crypt_dev for DTLS 1.3, on records of the same byte lengths; %d rounds of %d alternated calls; GiB/s over the bytes in front of the tag; per side"
             % (a.rounds, a.reps),
             "the median of the round medians (and that call's time in microseconds); spread = max - min of the base call's round medians.  Expected: parity, within the spread",
             "%-14s %-4s %-8s %4s %7s | %9s %7s %8s | %9s %8s %-6s | %s" % ("case", "ver", "op", "key", "records", "base", "spread", "us", "DTLS", "us", "within", "round trip")]
    for r in rows:
        lines.append("%-14s %-4s %-8s %4d %7d | %9.1f %7.1f %8.1f | %9.1f %8.1f %-6s | %s" % (
            r["case"], r["version"], r["op"], r["key_bits"], r["n_pkts"], r["gib_s"]["base"], r["base_spread_gib_s"], r["median_us"]["base"], r["gib_s"]["dtls"], r["median_us"]["dtls"],
            "yes" if r["within_base_spread"] else "NO", r["round_trip_ok"]))
    print("\n".join(lines))
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "ab.txt"), "w") as f:
        f.write("\n".join(lines) + "\n\n" + "\n".join(json.dumps(r) for r in rows) + "\n")
    assert all(r["round_trip_ok"] and r["status"] == [[0, 0], [0, 0]] for r in rows), "a side did not get its plaintext back"


if __name__ == "__main__":
    main()
