#!/usr/bin/env python3
"""SRTP and SRTCP packets against the parent commit's DTLS 1.2 call on packets of the same byte lengths (GPU box): aesgcm_keytab_srtp_crypt_dev of this build against a
library built at the PARENT commit (--base, a libaesgcm_hip.so; both libraries live in this one process, as the debug library does in the tests).  The base call,
aesgcm_keytab_dtls_crypt_dev in DTLS 1.2 mode, is one launch too and also builds its one AAD block in registers.  SRTP: a bare RTP header of 12 bytes, a rollover counter per
packet; SRTCP: E set in every packet, so the AAD is the one block header | W.  Every packet is L bytes on both sides.
    (a) 65536 packets of 1200 bytes over 1024 slots, AES-256        (b) 4096 packets of 1200 bytes over 64 slots, AES-256
encrypt and decrypt each.  Same process, same device, calls ALTERNATED, --reps calls per side and round, --rounds rounds, timed with events on the launch stream.  Per
side: the median of each round, and the median of those.  Spread = max - min of the base call's round medians.  The expectation is parity: within that spread.
Each side decrypts what it encrypted; every tag must be accepted and the tables' status words stay clear.
    python profiles/srtp/ab.py --base PATH/libaesgcm_hip.so [--reps 9] [--rounds 3] [--once]"""
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

SIDES = ("base", "srtp")


def load_base(path):
    """the parent commit's library, typed as far as this script calls it (it has no SRTP symbol for lib._keytab_typed to type)"""
    L = lib._typed(ctypes.CDLL(path))
    vp, sz, cint, u64 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_uint64
    L.aesgcm_keytab_create.argtypes = [ctypes.POINTER(vp), cint, sz, sz]
    L.aesgcm_keytab_set.argtypes = [vp, sz, sz, vp, vp]
    L.aesgcm_keytab_set_tls_iv.argtypes = [vp, sz, sz, vp, vp]
    L.aesgcm_keytab_dtls_crypt_dev.argtypes = [vp, cint, ctypes.POINTER(lib.DtlsFormat), sz, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
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


def case(name, kind, base, n, n_slots, key_len, L, reps, rounds, rng, once):
    rtp = kind == lib.SRTP_RTP
    f12, fs = lib.DtlsFormat.dtls12(), lib.SrtpFormat(kind, 0)
    front, back = (12, 16) if rtp else (8, 20)                        # the bytes in front of the payload and behind it
    keys = rng.integers(0, 256, size=n_slots * key_len, dtype=np.uint8).tobytes()
    salts = rng.integers(0, 256, size=n_slots * 12, dtype=np.uint8).tobytes()
    slots = rng.integers(0, n_slots, size=n, dtype=np.uint32)
    rocs = rng.integers(0, 1 << 32, size=n, dtype=np.uint32)
    off = np.arange(n + 1, dtype=np.uint64) * np.uint64(L)
    wire = rng.integers(0, 256, size=n * L, dtype=np.uint8)          # to the base call any bytes are a DTLS 1.2 record
    swire = wire.copy()
    swire[0::L] = 0x80                                                # version 2, no CSRC, no extension (SRTCP: no padding, count 0)
    if not rtp:
        swire[L - 4::L] |= 0x80                                       # W: E set
    d_slots, d_rocs, d_off, d_wire, d_swire = dev(slots), dev(rocs), dev(off), dev(wire), dev(swire)
    d_ct = {k: lib.DeviceBuffer(wire.nbytes + 64) for k in SIDES}
    d_pt = {k: lib.DeviceBuffer(wire.nbytes + 64) for k in SIDES}
    d_auth = {k: lib.DeviceBuffer(4 * n) for k in SIDES}
    with base_library(base):
        kb = lib.KeyTable(key_len, n_slots)
    ks = lib.KeyTable(key_len, n_slots)
    kb.set(0, keys); kb.set_tls_iv(0, salts)
    ks.set(0, keys); ks.set_tls_iv(0, salts)
    rows = []
    for decrypt in (0, 1):
        src = d_ct if decrypt else {"base": d_wire, "srtp": d_swire}
        dst = d_pt if decrypt else d_ct
        au = {k: d_auth[k].ptr if decrypt else None for k in SIDES}
        runs = {
            "base": lambda: kb.dtls_crypt_dev(decrypt, f12, n, d_slots.ptr, src["base"].ptr, d_off.ptr, dst["base"].ptr, d_auth=au["base"]),
            "srtp": lambda: ks.srtp_crypt_dev(decrypt, fs, n, d_slots.ptr, src["srtp"].ptr, d_off.ptr, dst["srtp"].ptr, d_roc=d_rocs.ptr if rtp else None, d_auth=au["srtp"]),
        }
        if once:
            for k in SIDES:
                runs[k]()
            lib.dev_sync()
            continue
        ms = alternate(runs, reps, rounds)
        lib.dev_sync()
        ok = True
        if decrypt:                                            # each side gets its plaintext back, every tag accepted
            for k in SIDES:
                a = np.frombuffer(bytes(d_auth[k].download(4 * n)), dtype=np.int32)
                ok = ok and bool((a == 1).all())
                keep = L - 16 if k == "base" else L - back
                for p in range(0, n, max(1, n // 64)):
                    pt = np.frombuffer(bytes(d_pt[k].download(keep, offset=p * L)), dtype=np.uint8)
                    ok = ok and bool((pt == (wire if k == "base" else swire)[p * L:p * L + keep]).all())
        gib = n * L / (1 << 30)
        rate = {k: [gib / (statistics.median(r) / 1e3) for r in v] for k, v in ms.items()}      # GiB/s of packet bytes, per round
        med_ms = {k: statistics.median(statistics.median(r) for r in v) for k, v in ms.items()}
        r = {"case": name, "kind": "SRTP" if rtp else "SRTCP", "op": "decrypt" if decrypt else "encrypt", "key_bits": 8 * key_len, "n_pkts": n, "n_slots": n_slots, "pkt_len": L,
             "payload": {"base": L - 37, "srtp": L - front - back},
             "reps": reps, "rounds": rounds, "ms": {k: [[round(x, 4) for x in rr] for rr in v] for k, v in ms.items()},
             "round_medians_gib_s": {k: [round(x, 1) for x in v] for k, v in rate.items()},
             "round_trip_ok": ok, "status": [list(kb.status()), list(ks.status())]}
        r["gib_s"] = {k: round(statistics.median(v), 1) for k, v in rate.items()}
        r["median_us"] = {k: round(1e3 * v, 1) for k, v in med_ms.items()}
        r["base_spread_gib_s"] = round(max(rate["base"]) - min(rate["base"]), 1)
        r["within_base_spread"] = r["gib_s"]["srtp"] >= r["gib_s"]["base"] - r["base_spread_gib_s"]
        print(json.dumps(r), flush=True)
        rows.append(r)
    kb.close(); ks.close()
    for b in [d_slots, d_rocs, d_off, d_wire, d_swire] + [x for d in (d_ct, d_pt, d_auth) for x in d.values()]:
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
    rng = np.random.default_rng(20261018)
    dev_name = lib.device_name(0)
    so = os.path.join(os.path.dirname(os.path.abspath(lib.__file__)), "libaesgcm_hip.so")
    sha = hashlib.sha256(open(so, "rb").read()).hexdigest()[:16]
    bsha = hashlib.sha256(open(a.base, "rb").read()).hexdigest()[:16]
    print("device:", dev_name, "library sha256:", sha, "base library sha256:", bsha, flush=True)
    base = load_base(a.base)
    rows = []
    for kind in (lib.SRTP_RTP, lib.SRTP_RTCP):
        rows += case("a_65536x1200", kind, base, 65536, 1024, 32, 1200, a.reps, a.rounds, rng, a.once)
        rows += case("b_4096x1200", kind, base, 4096, 64, 32, 1200, a.reps, a.rounds, rng, a.once)
    if a.once:
        return
    lines = ["device: %s; libaesgcm_hip.so sha256 %s...; baseline: the parent commit's library (sha256 %s...): aesgcm_keytab_dtls_crypt_dev in DTLS 1.2 mode, on packets of"
             % (dev_name, sha, bsha),
             "the same byte lengths (SRTCP: E set); %d rounds of %d alternated calls; GiB/s over the packets' bytes; per side the median of the round medians (and that call's"
             % (a.rounds, a.reps),
             "time in microseconds); spread = max - min of the base call's round medians.  Expected: parity, within the spread",
             "%-14s %-5s %-8s %4s %7s | %9s %7s %8s | %9s %8s %-6s | %s" % ("case", "kind", "op", "key", "packets", "base", "spread", "us", "SRTP", "us", "within", "round trip")]
    for r in rows:
        lines.append("%-14s %-5s %-8s %4d %7d | %9.1f %7.1f %8.1f | %9.1f %8.1f %-6s | %s" % (
            r["case"], r["kind"], r["op"], r["key_bits"], r["n_pkts"], r["gib_s"]["base"], r["base_spread_gib_s"], r["median_us"]["base"], r["gib_s"]["srtp"], r["median_us"]["srtp"],
            "yes" if r["within_base_spread"] else "NO", r["round_trip_ok"]))
    print("\n".join(lines))
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "ab.txt"), "w") as f:
        f.write("\n".join(lines) + "\n\n" + "\n".join(json.dumps(r) for r in rows) + "\n")
    assert all(r["round_trip_ok"] and r["status"] == [[0, 0], [0, 0]] for r in rows), "a side did not get its plaintext back"


if __name__ == "__main__":
    main()
