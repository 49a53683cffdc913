#!/usr/bin/env python3
"""SRTP's on-device key derivation: what an install costs beside the parent commit's set calls (GPU box).  The base side is the PARENT commit's library (--base, a
libaesgcm_hip.so built there; both libraries live in this one process, as in profiles/kdf/ab.py) doing what it does AFTER the host has derived everything:
aesgcm_keytab_set_dev of n session keys that lie in device memory plus aesgcm_keytab_set_tls_iv of n session salts.  The other side is this build's
aesgcm_srtp_kdf_install_dev of n entries (session key + session salt, kind SRTP, a d_r array) from n master keys on the device.  The base side derives nothing, so
parity is not the bar: the table says what the derivation costs.
    (a) install against the base, n = 65 536 and n = 4096, AES-256 and AES-128
    (b) the host's derivation of the same n (key, salt) in Python over libcrypto's AES-ECB on one core -- for scale only, timed once on min(n, 4096) entries and scaled
Same process, same device, calls ALTERNATED, --reps calls per side and round, --rounds rounds, timed with events on the launch stream.  Per side: the median of each
round, and the median of those.  Spread = max - min of the base side's round medians.
    python profiles/srtp_kdf/ab.py --base PATH/libaesgcm_hip.so [--reps 9] [--rounds 3]"""
import argparse
import ctypes
import ctypes.util
import hashlib
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


class HostAes:
    """AES-ECB of one block by libcrypto, for the host's derivation (scale only)"""

    def __init__(self):
        L = self.L = ctypes.CDLL(ctypes.util.find_library("crypto") or "libcrypto.so.3")
        vp = ctypes.c_void_p
        L.EVP_CIPHER_CTX_new.restype = vp
        L.EVP_CIPHER_CTX_free.argtypes = [vp]
        for nm in ("EVP_aes_128_ecb", "EVP_aes_256_ecb"):
            getattr(L, nm).restype = vp
        L.EVP_EncryptInit_ex.argtypes = [vp, vp, vp, ctypes.c_char_p, ctypes.c_char_p]
        L.EVP_CIPHER_CTX_set_padding.argtypes = [vp, ctypes.c_int]
        L.EVP_EncryptUpdate.argtypes = [vp, ctypes.c_char_p, ctypes.POINTER(ctypes.c_int), ctypes.c_char_p, ctypes.c_int]

    def derive(self, mk, ms, r):
        """RFC 3711 4.3.1: (SRTP session key, session salt) of one master: one key setup, two or three blocks"""
        L = self.L
        ctx = L.EVP_CIPHER_CTX_new()
        L.EVP_EncryptInit_ex(ctx, (L.EVP_aes_128_ecb if len(mk) == 16 else L.EVP_aes_256_ecb)(), None, mk, None)
        L.EVP_CIPHER_CTX_set_padding(ctx, 0)
        out, n = ctypes.create_string_buffer(32), ctypes.c_int(0)
        x = int.from_bytes(ms, "big")

        def block(label, j):
            L.EVP_EncryptUpdate(ctx, out, ctypes.byref(n), (x ^ (label << 48) ^ r).to_bytes(14, "big") + j.to_bytes(2, "big"), 16)
            return out.raw[:16]
        key = block(0, 0) + (block(0, 1) if len(mk) == 32 else b"")
        salt = block(2, 0)[:12]
        L.EVP_CIPHER_CTX_free(ctx)
        return key, salt


def case(name, base, n, key_len, reps, rounds, rng, host):
    masters = rng.integers(0, 256, n * key_len, dtype=np.uint8)
    msalts = rng.integers(0, 256, n * 14, dtype=np.uint8)
    keys = rng.integers(0, 256, n * key_len, dtype=np.uint8)                     # what the host would have derived: values do not matter to the time
    salts = rng.integers(0, 256, n * 12, dtype=np.uint8)
    idx = np.arange(n, dtype=np.uint32)
    rs = rng.integers(0, 1 << 48, n, dtype=np.uint64)
    bufs = {"keys": dev(keys), "idx": dev(idx), "r": dev(rs)}
    with base_library(base):
        bkt = lib.KeyTable(key_len, n)
    kt, mt = lib.KeyTable(key_len, n), lib.MasterKeyTable(key_len, n)
    mt.set(0, masters.tobytes(), msalts.tobytes())
    sb = salts.tobytes()

    def run_base():
        base.aesgcm_keytab_set_dev(bkt._h, n, bufs["idx"].ptr, bufs["keys"].ptr, None)
        base.aesgcm_keytab_set_tls_iv(bkt._h, 0, n, sb, None)

    runs = {"base": run_base, "install": lambda: mt.install_dev(lib.SRTP_RTP, kt, n, bufs["idx"].ptr, bufs["idx"].ptr, bufs["r"].ptr)}
    ms = alternate(runs, reps, rounds)
    lib.dev_sync()
    status = [list(bkt.status()), list(kt.status()), list(mt.status())]
    # (b) the host's derivation, one core
    m = min(n, 4096)
    mk = [masters[i * key_len:(i + 1) * key_len].tobytes() for i in range(m)]
    sl = [msalts[i * 14:(i + 1) * 14].tobytes() for i in range(m)]
    t0 = time.perf_counter()
    for i in range(m):
        host.derive(mk[i], sl[i], int(rs[i]))
    host_us = 1e6 * (time.perf_counter() - t0) * n / m
    for b in bufs.values():
        b.free()
    mt.close(); kt.close(); bkt.close()
    med = {k: [statistics.median(r) for r in v] for k, v in ms.items()}
    us = {k: 1e3 * statistics.median(v) for k, v in med.items()}
    return {"case": name, "n": n, "key_len": key_len, "round_medians_us": {k: [round(1e3 * x, 1) for x in v] for k, v in med.items()},
            "median_us": {k: round(v, 1) for k, v in us.items()}, "base_spread_us": round(1e3 * (max(med["base"]) - min(med["base"])), 1),
            "host_python_us": round(host_us, 1), "status": status}


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
    base, host = load_base(a.base), HostAes()
    rows = [case("a_65536_256", base, 65536, 32, a.reps, a.rounds, rng, host), case("a_65536_128", base, 65536, 16, a.reps, a.rounds, rng, host),
            case("a_4096_256", base, 4096, 32, a.reps, a.rounds, rng, host), case("a_4096_128", base, 4096, 16, a.reps, a.rounds, rng, host)]
    lines = ["device: %s; %s; libaesgcm_hip.so sha256 %s...; baseline: the parent commit's library (sha256 %s...): aesgcm_keytab_set_dev + aesgcm_keytab_set_tls_iv" % (dev_name, clocks, sha, bsha),
             "of n session keys / salts that lie derived in device / host memory; against aesgcm_srtp_kdf_install_dev (key + salt, kind SRTP, with d_r) of n masters; %d rounds of %d alternated calls;" % (a.rounds, a.reps),
             "microseconds per call, per side the median of the round medians; spread = max - min of the base side's round medians; host = Python over libcrypto's AES-ECB on one core, for scale",
             "%-12s %6s %4s | %9s %7s | %9s %8s | %11s" % ("case", "n", "key", "base set", "spread", "install", "diff", "host")]
    for r in rows:
        d = r["median_us"]["install"] - r["median_us"]["base"]
        lines.append("%-12s %6d %4d | %9.1f %7.1f | %9.1f %+8.1f | %11.1f" % (
            r["case"], r["n"], r["key_len"], r["median_us"]["base"], r["base_spread_us"], r["median_us"]["install"], d, r["host_python_us"]))
        lines.append("    install - base = %+.1f us: %s" % (d, "within the base spread" if abs(d) <= r["base_spread_us"] else
                                                             ("SLOWER than the base's set calls by more than the base spread -- a finding" if d > 0 else "faster by more than the base spread")))
    print("\n".join(lines))
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "ab.txt"), "w") as f:
        f.write("\n".join(lines) + "\n\n" + "\n".join(json.dumps(r) for r in rows) + "\n")
    assert all(r["status"] == [[0, 0], [0, 0], [0, 0]] for r in rows), "a call was refused"


if __name__ == "__main__":
    main()
