#!/usr/bin/env python3
"""TLS records against wire frames with 64-bit numbers on frames of the same byte lengths (GPU box): aesgcm_keytab_records_crypt_dev, TLS 1.3 and TLS 1.2, against
aesgcm_keytab_frames_crypt_x_dev with MACsec XPN.  The XPN call's kernels are the parent commit's, instruction for instruction (the assembly listing of k_kt_wirex is
byte-identical before and after the change that added k_kt_tls), so this build's XPN call is the baseline.  The same offsets serve all three sides: a frame of L bytes is
an XPN frame with a 28-byte header, a TLS 1.3 record with 5 bytes in front of its payload, a TLS 1.2 record with 13; every side ends in 16 bytes of tag.
    (a) 65536 frames of 5 + 16385 + 16 bytes, AES-256, 1024 slots        (b) 4096 frames of 5 + 1400 + 16 bytes, AES-256, 64 slots          encrypt and decrypt each
Same process, same device, calls ALTERNATED, --reps calls per side and round (>= 5), --rounds rounds (>= 3), timed with events on the launch stream.  Per side: the median
of each round, and the median of those.  Allowed shortfall: the base call's own spread, max - min of its round medians in this run.  Each side decrypts what it encrypted;
every tag must be accepted and the table's status word stay clear.
    python profiles/tls_ab.py [--reps 9] [--rounds 3] [--out profiles/tls]"""
import argparse
import hashlib
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import aesgcm_amd  # noqa: E402,F401
from aesgcm_amd import lib  # noqa: E402

SIDES = ("base", "tls13", "tls12")
FRONT = {"base": 28, "tls13": 5, "tls12": 13}


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


def case(name, n, n_slots, key_len, payload, reps, rounds, rng):
    L = 5 + payload + 16
    xf, f13, f12 = lib.WireFormatX.macsec_xpn(), lib.TlsFormat.tls13(), lib.TlsFormat.tls12()
    keys = rng.integers(0, 256, size=n_slots * key_len, dtype=np.uint8).tobytes()
    slots = rng.integers(0, n_slots, size=n, dtype=np.uint32)
    seqs = rng.integers(0, 1 << 63, size=n, dtype=np.uint64)
    his = (seqs >> np.uint64(32)).astype(np.uint32)
    woff = np.arange(n + 1, dtype=np.uint64) * np.uint64(L)
    wire = rng.integers(0, 256, size=n * L, dtype=np.uint8)
    d_slots, d_seqs, d_his, d_woff, d_wire = dev(slots), dev(seqs), dev(his), dev(woff), dev(wire)
    d_ct = {k: lib.DeviceBuffer(wire.nbytes + 64) for k in SIDES}
    d_pt = {k: lib.DeviceBuffer(wire.nbytes + 64) for k in SIDES}
    d_auth = {k: lib.DeviceBuffer(4 * n) for k in SIDES}
    # a slot is a MACsec association or a TLS connection direction: one table per kind, the same keys
    kx, kt = lib.KeyTable(key_len, n_slots), lib.KeyTable(key_len, n_slots)
    kx.set(0, keys); kt.set(0, keys)
    kx.set_xpn(0, rng.integers(0, 256, size=n_slots * 12, dtype=np.uint8).tobytes(), rng.integers(0, 256, size=n_slots * 4, dtype=np.uint8).tobytes())
    kt.set_tls_iv(0, rng.integers(0, 256, size=n_slots * 12, dtype=np.uint8).tobytes())
    rows = []
    for decrypt in (0, 1):
        src = d_ct if decrypt else {k: d_wire for k in SIDES}
        dst = d_pt if decrypt else d_ct
        au = {k: d_auth[k].ptr if decrypt else None for k in SIDES}
        runs = {
            "base": lambda: kx.frames_crypt_x_dev(decrypt, xf, n, d_slots.ptr, d_his.ptr, src["base"].ptr, d_woff.ptr, dst["base"].ptr, d_auth=au["base"]),
            "tls13": lambda: kt.records_crypt_dev(decrypt, f13, n, d_slots.ptr, d_seqs.ptr, src["tls13"].ptr, d_woff.ptr, dst["tls13"].ptr, d_auth=au["tls13"]),
            "tls12": lambda: kt.records_crypt_dev(decrypt, f12, n, d_slots.ptr, d_seqs.ptr, src["tls12"].ptr, d_woff.ptr, dst["tls12"].ptr, d_auth=au["tls12"]),
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
                    ok = ok and bool((pt == wire[p * L:(p + 1) * L - 16]).all())
        gib = n * (L - 16) / (1 << 30)
        rate = {k: [gib / (statistics.median(r) / 1e3) for r in v] for k, v in ms.items()}      # GiB/s, per round
        r = {"case": name, "op": "decrypt" if decrypt else "encrypt", "key_bits": 8 * key_len, "n_frames": n, "n_slots": n_slots, "frame_len": L,
             "reps": reps, "rounds": rounds, "ms": {k: [[round(x, 4) for x in rr] for rr in v] for k, v in ms.items()},
             "round_medians_gib_s": {k: [round(x, 1) for x in v] for k, v in rate.items()},
             "round_trip_ok": ok, "status": [list(kx.status()), list(kt.status())]}
        r["gib_s"] = {k: round(statistics.median(v), 1) for k, v in rate.items()}
        r["base_spread_gib_s"] = round(max(rate["base"]) - min(rate["base"]), 1)
        r["within_base_spread"] = {k: r["gib_s"][k] >= r["gib_s"]["base"] - r["base_spread_gib_s"] for k in SIDES[1:]}
        print(json.dumps(r), flush=True)
        rows.append(r)
    kx.close(); kt.close()
    for b in [d_slots, d_seqs, d_his, d_woff, d_wire] + [x for d in (d_ct, d_pt, d_auth) for x in d.values()]:
        b.free()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "tls"))
    a = ap.parse_args()
    assert a.reps >= 5 and a.rounds >= 3
    rng = np.random.default_rng(20261017)
    dev_name = lib.device_name(0)
    so = os.path.join(os.path.dirname(os.path.abspath(lib.__file__)), "libaesgcm_hip.so")
    sha = hashlib.sha256(open(so, "rb").read()).hexdigest()[:16]
    print("device:", dev_name, "library sha256:", sha, flush=True)
    rows = case("a_65536x16385", 65536, 1024, 32, 16385, a.reps, a.rounds, rng)
    rows += case("b_4096x1400", 4096, 64, 32, 1400, a.reps, a.rounds, rng)
    lines = ["device: %s; libaesgcm_hip.so sha256 %s...; baseline: aesgcm_keytab_frames_crypt_x_dev (MACsec XPN) of this build on frames of the same byte lengths;"
             % (dev_name, sha),
             "%d rounds of %d alternated calls; GiB/s over the bytes in front of the tag; per side the median of the round medians; spread = max - min of the base call's"
             % (a.rounds, a.reps),
             "round medians",
             "%-15s %-8s %7s | %9s %7s | %9s %-6s | %9s %-6s | %s" % ("case", "op", "frames", "base XPN", "spread", "TLS 1.3", "within", "TLS 1.2", "within", "round trip")]
    for r in rows:
        w = r["within_base_spread"]
        lines.append("%-15s %-8s %7d | %9.1f %7.1f | %9.1f %-6s | %9.1f %-6s | %s" % (
            r["case"], r["op"], r["n_frames"], r["gib_s"]["base"], r["base_spread_gib_s"], r["gib_s"]["tls13"], "yes" if w["tls13"] else "NO",
            r["gib_s"]["tls12"], "yes" if w["tls12"] else "NO", r["round_trip_ok"]))
    print("\n".join(lines))
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "ab.txt"), "w") as f:
        f.write("\n".join(lines) + "\n\n" + "\n".join(json.dumps(r) for r in rows) + "\n")
    assert all(r["round_trip_ok"] and r["status"] == [[0, 0], [0, 0]] for r in rows), "a side did not get its plaintext back"


if __name__ == "__main__":
    main()
