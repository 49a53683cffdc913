#!/usr/bin/env python3
"""MACsec's MKA on the device: what install and unwrap cost beside the parent commit's set call (GPU box).  The base side is the PARENT commit's library (--base, a
libaesgcm_hip.so built there; both libraries live in this one process, as in profiles/prfplus/ab.py) doing what a caller does today AFTER the host has derived or
unwrapped everything: aesgcm_keytab_set_dev of the same n SAKs lying derived in device memory.  That side derives nothing.  The other sides are this build's
aesgcm_mka_install_dev of n entries without and with wrapped output, from n CAK records and n byte-packed contexts on the device (KS-nonce | 3 MIs | KN: key_len + 40
bytes, behind one odd byte), and aesgcm_mka_unwrap_dev of the n wrapped SAKs that install made.
    n = 65 536 and n = 4096, AES-128 CAK + SAK and AES-256 CAK + SAK
Same process, same device, calls ALTERNATED, --reps calls per side and round, --rounds rounds, timed with events on the launch stream.  Per side: the median of each
round, and the median of those.  Spread = max - min of the base side's round medians.
    python profiles/mka/ab.py --base PATH/libaesgcm_hip.so [--reps 9] [--rounds 3]"""
import argparse
import ctypes
import hashlib
import json
import os
import statistics
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import aesgcm_amd  # noqa: E402,F401
from aesgcm_amd import lib  # noqa: E402

SIDES = ("base", "install", "install_wrap", "unwrap")


def load_base(path):
    """the parent commit's library, typed as far as this script calls it"""
    L = lib._typed(ctypes.CDLL(path))
    vp, sz, cint, u64 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_uint64
    L.aesgcm_keytab_create.argtypes = [ctypes.POINTER(vp), cint, sz, sz]
    L.aesgcm_keytab_set_dev.argtypes = [vp, sz, vp, vp, vp]
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


def case(name, base, n, key_len, reps, rounds, rng):
    ctx_len, w = key_len + 40, key_len + 8
    caks = rng.integers(0, 256, n * key_len, dtype=np.uint8)
    ctxs = rng.integers(0, 256, n * ctx_len + 1, dtype=np.uint8)                 # byte-packed behind one odd byte: no context starts on a word
    keys = rng.integers(0, 256, n * key_len, dtype=np.uint8)                     # what the host would have derived: values do not matter to the time
    idx = np.arange(n, dtype=np.uint32)
    off = (np.arange(n + 1, dtype=np.uint64) * ctx_len + 1).astype(np.uint32)
    bufs = {"keys": dev(keys), "idx": dev(idx), "ctx": dev(ctxs), "off": dev(off), "wrapped": dev(np.zeros(n * w, dtype=np.uint8)), "verdict": dev(np.zeros(n, dtype=np.uint8))}
    with base_library(base):
        bkt = lib.KeyTable(key_len, n)
    kt, rx, ct = lib.KeyTable(key_len, n), lib.KeyTable(key_len, n), lib.CakTable(key_len, n)
    cb = caks.tobytes()
    ct.set(0, cb, [cb[key_len * i:key_len * i + 16] for i in range(n)])
    p = {k: b.ptr for k, b in bufs.items()}
    runs = {"base": lambda: base.aesgcm_keytab_set_dev(bkt._h, n, p["idx"], p["keys"], None),
            "install": lambda: ct.install_dev(kt, n, p["idx"], p["ctx"], p["off"], p["idx"], None),
            "install_wrap": lambda: ct.install_dev(kt, n, p["idx"], p["ctx"], p["off"], p["idx"], p["wrapped"]),
            "unwrap": lambda: ct.unwrap_dev(rx, n, p["idx"], p["wrapped"], p["idx"], p["verdict"])}
    runs["install_wrap"]()                                                       # the wrapped SAKs that unwrap takes
    lib.dev_sync()
    ms = alternate(runs, reps, rounds)
    lib.dev_sync()
    status = [list(bkt.status()), list(kt.status()), list(rx.status()), list(ct.status())]
    verdicts_ok = bytes(bufs["verdict"].download(n)) == bytes(n)
    for b in bufs.values():
        b.free()
    ct.close(); kt.close(); rx.close(); bkt.close()
    med = {k: [statistics.median(r) for r in v] for k, v in ms.items()}
    us = {k: 1e3 * statistics.median(v) for k, v in med.items()}
    return {"case": name, "n": n, "key_len": key_len, "ctx_len": ctx_len, "round_medians_us": {k: [round(1e3 * x, 1) for x in v] for k, v in med.items()},
            "median_us": {k: round(v, 1) for k, v in us.items()}, "base_spread_us": round(1e3 * (max(med["base"]) - min(med["base"])), 1), "status": status,
            "verdicts_ok": verdicts_ok}


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
    rng = np.random.default_rng(20261021)
    dev_name = lib.device_name(0)
    so = os.path.join(os.path.dirname(os.path.abspath(lib.__file__)), "libaesgcm_hip.so")
    sha = hashlib.sha256(open(so, "rb").read()).hexdigest()[:16]
    bsha = hashlib.sha256(open(a.base, "rb").read()).hexdigest()[:16]
    clocks = clock_line()
    print("device:", dev_name, "|", clocks, "| library sha256:", sha, "base library sha256:", bsha, flush=True)
    base = load_base(a.base)
    rows = [case("mka_%d_%d" % (n, 8 * kl), base, n, kl, a.reps, a.rounds, rng) for n, kl in ((65536, 16), (65536, 32), (4096, 16), (4096, 32))]
    lines = ["device: %s; %s; libaesgcm_hip.so sha256 %s...; baseline: the parent commit's library (sha256 %s...): aesgcm_keytab_set_dev of n SAKs that lie derived in" % (dev_name, clocks, sha, bsha),
             "device memory; against aesgcm_mka_install_dev without and with wrapped output (n CAK records, n byte-packed contexts of key_len + 40 bytes) and aesgcm_mka_unwrap_dev;",
             "%d rounds of %d alternated calls; microseconds per call, per side the median of the round medians; spread = max - min of the base side's round medians" % (a.rounds, a.reps),
             "%-14s %6s %4s | %9s %7s | %9s %8s | %12s %8s | %9s %8s" % ("case", "n", "key", "base set", "spread", "install", "diff", "install+wrap", "diff", "unwrap", "diff")]
    for r in rows:
        m = r["median_us"]
        d = {k: m[k] - m["base"] for k in SIDES[1:]}
        lines.append("%-14s %6d %4d | %9.1f %7.1f | %9.1f %+8.1f | %12.1f %+8.1f | %9.1f %+8.1f" % (
            r["case"], r["n"], r["key_len"], m["base"], r["base_spread_us"], m["install"], d["install"], m["install_wrap"], d["install_wrap"], m["unwrap"], d["unwrap"]))
        for k in SIDES[1:]:
            lines.append("    %s - base = %+.1f us: %s" % (k, d[k], "within the base spread" if abs(d[k]) <= r["base_spread_us"] else
                                                          ("SLOWER than the base's set call by more than the base spread -- a finding" if d[k] > 0 else "faster by more than the base spread")))
    print("\n".join(lines))
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "ab.txt"), "w") as f:
        f.write("\n".join(lines) + "\n\n" + "\n".join(json.dumps(r) for r in rows) + "\n")
    assert all(r["status"] == [[0, 0]] * 4 and r["verdicts_ok"] for r in rows), "a call was refused"


if __name__ == "__main__":
    main()
