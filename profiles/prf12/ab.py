#!/usr/bin/env python3
"""The TLS 1.2 PRF on the device: what an install costs beside the parent commit's set calls (GPU box).  The base side is the PARENT commit's library (--base, a
libaesgcm_hip.so built there; both libraries live in this one process, as in profiles/kdf/ab.py) doing what a caller does today AFTER the host has derived
everything: aesgcm_keytab_set_dev of n device keys twice (the client's slots, the server's) plus aesgcm_keytab_set_tls_iv of n IVs twice.  That side derives nothing.
The other side is this build's aesgcm_prf12_install_dev of n entries, both directions, from n master-secret records on the device.
    (a) install against the base, n = 65 536 and n = 4096, AES-256 / SHA-384 and AES-128 / SHA-256
    (b) aesgcm_prf12_export_srtp_dev alone, both directions, the same n, into an SRTP master table of the same key size
    (c) the host's derivation of the same n key blocks with Python's hmac on one core -- for scale only, timed once on min(n, 1024) entries and scaled
Same process, same device, calls ALTERNATED, --reps calls per side and round, --rounds rounds, timed with events on the launch stream.  Per side: the median of each
round, and the median of those.  Spread = max - min of the base side's round medians.
    python profiles/prf12/ab.py --base PATH/libaesgcm_hip.so [--reps 9] [--rounds 3]"""
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

SIDES = ("base", "install", "export")


def load_base(path):
    """the parent commit's library, typed as far as this script calls it"""
    L = lib._typed(ctypes.CDLL(path))
    vp, sz, cint, u64 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_uint64
    L.aesgcm_keytab_create.argtypes = [ctypes.POINTER(vp), cint, sz, sz]
    L.aesgcm_keytab_set_dev.argtypes = [vp, sz, vp, vp, vp]
    L.aesgcm_keytab_set_tls_iv.argtypes = [vp, sz, sz, vp, vp]
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


def p_hash(hname, secret, seed, length):
    out, a = b"", seed
    while len(out) < length:
        a = hmac.new(secret, a, hname).digest()
        out += hmac.new(secret, a + seed, hname).digest()
    return out[:length]


def case(name, base, n, key_len, hash_len, reps, rounds, rng):
    hname = {32: "sha256", 48: "sha384"}[hash_len]
    masters = rng.integers(0, 256, n * 48, dtype=np.uint8)
    crs, srs = rng.integers(0, 256, n * 32, dtype=np.uint8), rng.integers(0, 256, n * 32, dtype=np.uint8)
    keys = rng.integers(0, 256, 2 * n * key_len, dtype=np.uint8)                 # what the host would have derived: values do not matter to the time
    ivs = rng.integers(0, 256, 2 * n * 12, dtype=np.uint8)
    idx = np.arange(n, dtype=np.uint32)
    bufs = {"keys": dev(keys), "idx": dev(idx), "srv": dev(idx + np.uint32(n))}
    with base_library(base):
        bkt = lib.KeyTable(key_len, 2 * n)
    kt, mt, mk = lib.KeyTable(key_len, 2 * n), lib.MasterSecretTable(hash_len, n), lib.MasterKeyTable(key_len, 2 * n)
    mt.set(0, masters.tobytes(), crs.tobytes(), srs.tobytes())
    ivb = ivs.tobytes()
    civ, siv = ivb[:12 * n], ivb[12 * n:]
    srv_keys = bufs["keys"].ptr + n * key_len

    def run_base():
        base.aesgcm_keytab_set_dev(bkt._h, n, bufs["idx"].ptr, bufs["keys"].ptr, None)
        base.aesgcm_keytab_set_dev(bkt._h, n, bufs["srv"].ptr, srv_keys, None)
        base.aesgcm_keytab_set_tls_iv(bkt._h, 0, n, civ, None)
        base.aesgcm_keytab_set_tls_iv(bkt._h, n, n, siv, None)

    runs = {"base": run_base, "install": lambda: mt.install_dev(kt, n, bufs["idx"].ptr, bufs["idx"].ptr, bufs["srv"].ptr),
            "export": lambda: mt.export_srtp_dev(mk, n, bufs["idx"].ptr, bufs["idx"].ptr, bufs["srv"].ptr)}
    ms = alternate(runs, reps, rounds)
    lib.dev_sync()
    status = [list(bkt.status()), list(kt.status()), list(mt.status()), list(mk.status())]
    # (c) the host's derivation, one core
    m = min(n, 1024)
    rows = [(masters[48 * i:48 * i + 48].tobytes(), b"key expansion" + srs[32 * i:32 * i + 32].tobytes() + crs[32 * i:32 * i + 32].tobytes()) for i in range(m)]
    t0 = time.perf_counter()
    for sec, seed in rows:
        p_hash(hname, sec, seed, 2 * key_len + 8)
    host_us = 1e6 * (time.perf_counter() - t0) * n / m
    for b in bufs.values():
        b.free()
    mk.close(); mt.close(); kt.close(); bkt.close()
    med = {k: [statistics.median(r) for r in v] for k, v in ms.items()}
    us = {k: 1e3 * statistics.median(v) for k, v in med.items()}
    return {"case": name, "n": n, "key_len": key_len, "hash_len": hash_len, "round_medians_us": {k: [round(1e3 * x, 1) for x in v] for k, v in med.items()},
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
    rows = [case("a_65536_256_384", base, 65536, 32, 48, a.reps, a.rounds, rng), case("a_65536_128_256", base, 65536, 16, 32, a.reps, a.rounds, rng),
            case("a_4096_256_384", base, 4096, 32, 48, a.reps, a.rounds, rng), case("a_4096_128_256", base, 4096, 16, 32, a.reps, a.rounds, rng)]
    lines = ["device: %s; %s; libaesgcm_hip.so sha256 %s...; baseline: the parent commit's library (sha256 %s...): aesgcm_keytab_set_dev x 2 + aesgcm_keytab_set_tls_iv x 2" % (dev_name, clocks, sha, bsha),
             "of n keys / IVs per direction that lie derived in device / host memory; against aesgcm_prf12_install_dev (both directions) of n master-secret records; export = aesgcm_prf12_export_srtp_dev alone;",
             "%d rounds of %d alternated calls; microseconds per call, per side the median of the round medians; spread = max - min of the base side's round medians; host hmac = Python on one core, for scale" % (a.rounds, a.reps),
             "%-16s %6s %4s %4s | %9s %7s | %9s %8s | %9s | %11s" % ("case", "n", "key", "hash", "base set", "spread", "install", "diff", "export", "host hmac")]
    for r in rows:
        d = r["median_us"]["install"] - r["median_us"]["base"]
        lines.append("%-16s %6d %4d %4d | %9.1f %7.1f | %9.1f %+8.1f | %9.1f | %11.1f" % (
            r["case"], r["n"], r["key_len"], r["hash_len"], r["median_us"]["base"], r["base_spread_us"], r["median_us"]["install"], d, r["median_us"]["export"], r["host_hmac_us"]))
        lines.append("    install - base = %+.1f us: %s" % (d, "within the base spread" if abs(d) <= r["base_spread_us"] else
                                                             ("SLOWER than the base's set calls by more than the base spread -- a finding" if d > 0 else "faster by more than the base spread")))
    print("\n".join(lines))
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "ab.txt"), "w") as f:
        f.write("\n".join(lines) + "\n\n" + "\n".join(json.dumps(r) for r in rows) + "\n")
    assert all(r["status"] == [[0, 0]] * 4 for r in rows), "a call was refused"


if __name__ == "__main__":
    main()
