#!/usr/bin/env python3
"""IKEv2's prf+ on the device: what an install costs beside the parent commit's set calls (GPU box).  The base side is the PARENT commit's library (--base, a
libaesgcm_hip.so built there; both libraries live in this one process, as in profiles/prf12/ab.py) doing what a caller does today AFTER the host has derived
everything: aesgcm_keytab_set_dev of n device keys twice (the i2r slots, the r2i slots) plus aesgcm_keytab_set_salt of n salts twice.  That side derives nothing.
The other side is this build's aesgcm_prfplus_install_dev of n entries, both directions, from n SK_d records and n byte-packed seeds on the device.
    (a) install against the base, n = 65 536 and n = 4096, AES-128 / SHA-256, AES-256 / SHA-384 and AES-256 / SHA-512, 64-byte seeds (Ni | Nr of 32 bytes each)
    (b) one run with 320-byte seeds (a 256-byte g^ir in front of the nonces), AES-256 / SHA-384 at n = 65 536
    (c) the host's derivation of the same n KEYMATs with Python's hmac on one core -- for scale only, timed once on min(n, 1024) entries and scaled
Same process, same device, calls ALTERNATED, --reps calls per side and round, --rounds rounds, timed with events on the launch stream.  Per side: the median of each
round, and the median of those.  Spread = max - min of the base side's round medians.
    python profiles/prfplus/ab.py --base PATH/libaesgcm_hip.so [--reps 9] [--rounds 3]"""
import argparse
import ctypes
import hashlib
import hmac
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import aesgcm_amd  # noqa: E402,F401
from aesgcm_amd import lib  # noqa: E402

SIDES = ("base", "install")


def load_base(path):
    """the parent commit's library, typed as far as this script calls it"""
    L = lib._typed(ctypes.CDLL(path))
    vp, sz, cint, u64 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_uint64
    L.aesgcm_keytab_create.argtypes = [ctypes.POINTER(vp), cint, sz, sz]
    L.aesgcm_keytab_set_dev.argtypes = [vp, sz, vp, vp, vp]
    L.aesgcm_keytab_set_salt.argtypes = [vp, sz, sz, vp, vp]
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


def prf_plus(hname, key, seed, length):
    out, t, ctr = b"", b"", 1
    while len(out) < length:
        t = hmac.new(key, t + seed + bytes([ctr]), hname).digest()
        out, ctr = out + t, ctr + 1
    return out[:length]


def case(name, base, n, key_len, hash_len, seed_len, reps, rounds, rng):
    hname = {32: "sha256", 48: "sha384", 64: "sha512"}[hash_len]
    sk = rng.integers(0, 256, n * hash_len, dtype=np.uint8)
    seeds = rng.integers(0, 256, n * seed_len + 1, dtype=np.uint8)               # byte-packed behind one odd byte: no seed starts on a word
    keys = rng.integers(0, 256, 2 * n * key_len, dtype=np.uint8)                 # what the host would have derived: values do not matter to the time
    salts = rng.integers(0, 256, 2 * n * 8, dtype=np.uint8)
    idx = np.arange(n, dtype=np.uint32)
    off = (np.arange(n + 1, dtype=np.uint64) * seed_len + 1).astype(np.uint32)
    bufs = {"keys": dev(keys), "idx": dev(idx), "r2i": dev(idx + np.uint32(n)), "seed": dev(seeds), "off": dev(off)}
    with base_library(base):
        bkt = lib.KeyTable(key_len, 2 * n)
    kt, it = lib.KeyTable(key_len, 2 * n), lib.IkeSaTable(hash_len, n)
    it.set(0, sk.tobytes())
    sb = salts.tobytes()
    s0, s1 = sb[:8 * n], sb[8 * n:]
    r2i_keys = bufs["keys"].ptr + n * key_len

    def run_base():
        base.aesgcm_keytab_set_dev(bkt._h, n, bufs["idx"].ptr, bufs["keys"].ptr, None)
        base.aesgcm_keytab_set_dev(bkt._h, n, bufs["r2i"].ptr, r2i_keys, None)
        base.aesgcm_keytab_set_salt(bkt._h, 0, n, s0, None)
        base.aesgcm_keytab_set_salt(bkt._h, n, n, s1, None)

    runs = {"base": run_base, "install": lambda: it.install_dev(kt, n, bufs["idx"].ptr, bufs["seed"].ptr, bufs["off"].ptr, bufs["idx"].ptr, bufs["r2i"].ptr)}
    ms = alternate(runs, reps, rounds)
    lib.dev_sync()
    status = [list(bkt.status()), list(kt.status()), list(it.status())]
    # (c) the host's derivation, one core
    m = min(n, 1024)
    rows = [(sk[hash_len * i:hash_len * i + hash_len].tobytes(), seeds[1 + seed_len * i:1 + seed_len * (i + 1)].tobytes()) for i in range(m)]
    t0 = time.perf_counter()
    for key, seed in rows:
        prf_plus(hname, key, seed, 2 * key_len + 8)
    host_us = 1e6 * (time.perf_counter() - t0) * n / m
    for b in bufs.values():
        b.free()
    it.close(); kt.close(); bkt.close()
    med = {k: [statistics.median(r) for r in v] for k, v in ms.items()}
    us = {k: 1e3 * statistics.median(v) for k, v in med.items()}
    return {"case": name, "n": n, "key_len": key_len, "hash_len": hash_len, "seed_len": seed_len, "round_medians_us": {k: [round(1e3 * x, 1) for x in v] for k, v in med.items()},
            "median_us": {k: round(v, 1) for k, v in us.items()}, "base_spread_us": round(1e3 * (max(med["base"]) - min(med["base"])), 1),
            "host_hmac_us": round(host_us, 1), "status": status}


def clock_line():
    try:
        out = subprocess.run(["rocm-smi", "--showclocks", "-d", "0"], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True, timeout=30).stdout
        got = [" ".join(ln.split()) for ln in out.splitlines() if "sclk" in ln or "mclk" in ln]
        return "; ".join(got) or "clocks: not reported"
    except Exception as e:                                                       # noqa: BLE001
        return "clocks: not read (%s)" % type(e).__name__


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--base", required=True, help="libaesgcm_hip.so built at the parent commit")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=HERE)
    a = ap.parse_args()
    assert a.reps >= 5 and a.rounds >= 3
    rng = np.random.default_rng(20261020)
    dev_name = lib.device_name(0)
    so = os.path.join(os.path.dirname(os.path.abspath(lib.__file__)), "libaesgcm_hip.so")
    sha = hashlib.sha256(open(so, "rb").read()).hexdigest()[:16]
    bsha = hashlib.sha256(open(a.base, "rb").read()).hexdigest()[:16]
    clocks = clock_line()
    print("device:", dev_name, "|", clocks, "| library sha256:", sha, "base library sha256:", bsha, flush=True)
    base = load_base(a.base)
    rows = [case("%s_%d_%d_%d" % ("b" if sl != 64 else "a", n, 8 * kl, 8 * hl), base, n, kl, hl, sl, a.reps, a.rounds, rng)
            for n, kl, hl, sl in ((65536, 16, 32, 64), (65536, 32, 48, 64), (65536, 32, 64, 64), (4096, 16, 32, 64), (4096, 32, 48, 64), (4096, 32, 64, 64), (65536, 32, 48, 320))]
    lines = ["device: %s; %s; libaesgcm_hip.so sha256 %s...; baseline: the parent commit's library (sha256 %s...): aesgcm_keytab_set_dev x 2 + aesgcm_keytab_set_salt x 2" % (dev_name, clocks, sha, bsha),
             "of n keys / salts per direction that lie derived in device / host memory; against aesgcm_prfplus_install_dev (both directions) of n SK_d records and n byte-packed seeds;",
             "%d rounds of %d alternated calls; microseconds per call, per side the median of the round medians; spread = max - min of the base side's round medians; host hmac = Python on one core, for scale" % (a.rounds, a.reps),
             "%-18s %6s %4s %4s %5s | %9s %7s | %9s %8s | %11s" % ("case", "n", "key", "hash", "seed", "base set", "spread", "install", "diff", "host hmac")]
    for r in rows:
        d = r["median_us"]["install"] - r["median_us"]["base"]
        lines.append("%-18s %6d %4d %4d %5d | %9.1f %7.1f | %9.1f %+8.1f | %11.1f" % (
            r["case"], r["n"], r["key_len"], r["hash_len"], r["seed_len"], r["median_us"]["base"], r["base_spread_us"], r["median_us"]["install"], d, r["host_hmac_us"]))
        lines.append("    install - base = %+.1f us: %s" % (d, "within the base spread" if abs(d) <= r["base_spread_us"] else
                                                             ("SLOWER than the base's set calls by more than the base spread -- a finding" if d > 0 else "faster by more than the base spread")))
    print("\n".join(lines))
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "ab.txt"), "w") as f:
        f.write("\n".join(lines) + "\n\n" + "\n".join(json.dumps(r) for r in rows) + "\n")
    assert all(r["status"] == [[0, 0]] * 3 for r in rows), "a call was refused"


if __name__ == "__main__":
    main()
