#!/usr/bin/env python3
"""Send counters: what assign adds to an encrypt call (GPU box).  The base side is the PARENT commit's XPN encrypt call alone (--base, a libaesgcm_hip.so built there;
both libraries live in this one process, as in profiles/rxwin/ab.py): aesgcm_keytab_frames_crypt_x_dev with d_hi given and the SecTAG's PN already in the frames.  The
other side is this build's send loop on the same frames: aesgcm_txnum_assign_dev (MACsec XPN: the number, d_hi, the PN's lower half into the SecTAG, d_slots) + the
same encrypt call -- seven launches for one (64 counters or one: one sort pass).
    (a) 4096 MACsec-shaped frames (64 .. 1514 payload bytes, byte-packed) on 64 counters      (b) the same 4096 frames all on ONE counter
    (c) 2^20 such frames on 64 counters                                                        (d) the 2^20 frames all on ONE counter
AES-256, 64 slots.  By construction (a) = (b) and (c) = (d): no atomic, no step whose cost depends on how many packets share a counter.  The counters are set back
before every timed call, outside the timed region.  Same process, same device, calls ALTERNATED, --reps calls per side and round, --rounds rounds, timed with events
on the launch stream.  Per side: the median of each round, and the median of those.  Spread = max - min of the base call's round medians.
    python profiles/txnum/ab.py --base PATH/libaesgcm_hip.so [--reps 9] [--rounds 3]"""
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

SIDES = ("base", "txnum")


def load_base(path):
    """the parent commit's library, typed as far as this script calls it"""
    L = lib._typed(ctypes.CDLL(path))
    vp, sz, cint, u64 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_uint64
    L.aesgcm_keytab_create.argtypes = [ctypes.POINTER(vp), cint, sz, sz]
    L.aesgcm_keytab_set.argtypes = [vp, sz, sz, vp, vp]
    L.aesgcm_keytab_set_salt.argtypes = [vp, sz, sz, vp, vp]
    L.aesgcm_keytab_set_xpn.argtypes = [vp, sz, sz, vp, vp, vp]
    L.aesgcm_keytab_frames_crypt_x_dev.argtypes = [vp, cint, ctypes.POINTER(lib.WireFormatX), sz, vp, vp, vp, vp, vp, vp, vp]
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


def alternate(runs, before, reps, rounds):
    t = lib.Timer()
    for _ in range(2):                                        # every shape warmed up
        for k in SIDES:
            before[k](); runs[k]()
    lib.dev_sync()
    ms = {k: [] for k in SIDES}
    for _ in range(rounds):
        r = {k: [] for k in SIDES}
        for _ in range(reps):
            for k in SIDES:
                before[k]()
                t.start(); runs[k](); t.stop()
                r[k].append(t.ms())
        for k in r:
            ms[k].append(r[k])
    t.close()
    return ms


def case(name, base, n, n_ctrs, reps, rounds, rng):
    key_len, n_slots = 32, 64
    xf, tf = lib.WireFormatX.macsec_xpn(), lib.TxFormat.macsec_xpn()
    keys = rng.integers(0, 256, size=n_slots * key_len, dtype=np.uint8).tobytes()
    salts = rng.integers(0, 256, size=n_slots * 8, dtype=np.uint8).tobytes()
    xsalts = rng.integers(0, 256, size=n_slots * 12, dtype=np.uint8).tobytes()
    sscis = rng.integers(0, 256, size=n_slots * 4, dtype=np.uint8).tobytes()
    slots = rng.integers(0, n_slots, size=n, dtype=np.uint32)
    ctrs = (slots % n_ctrs).astype(np.uint32)
    lens = rng.integers(64, 1515, size=n, dtype=np.int64) + 28 + 16        # SecTAG with SCI behind DA SA, 16 bytes of ICV
    off = np.zeros(n + 1, dtype=np.uint64)
    off[1:] = np.cumsum(lens).astype(np.uint64)
    # counter c's k-th frame (in array order) gets start_c + k; every counter crosses 2^32 inside the call
    count = np.bincount(ctrs, minlength=n_ctrs)
    start = (1 << 32) - count // 2
    rank = np.zeros(n, dtype=np.int64)
    for c in range(n_ctrs):
        idx = np.nonzero(ctrs == c)[0]
        rank[idx] = np.arange(len(idx), dtype=np.int64)
    nums = (start[ctrs] + rank).astype(np.uint64)
    plain = rng.integers(0, 256, size=int(off[-1]), dtype=np.uint8)
    numbered = plain.copy()                                                # the base side's frames: the PN's lower half already in the SecTAG
    first = off[:-1].astype(np.int64)
    for k in range(4):
        numbered[first + 16 + k] = ((nums >> np.uint64(8 * (3 - k))) & np.uint64(0xFF)).astype(np.uint8)
    his = (nums >> np.uint64(32)).astype(np.uint32)
    d_slots_in, d_ctr, d_off, d_his, d_numbered = dev(slots), dev(ctrs), dev(off), dev(his), dev(numbered)
    nb = plain.nbytes + 64
    d_work = dev(plain)                                                    # the send loop numbers these in place (the same bytes every time), then encrypts out of place
    d_out = {k: lib.DeviceBuffer(nb) for k in SIDES}
    d_slots, d_num, d_hi = dev(slots), lib.DeviceBuffer(8 * n), lib.DeviceBuffer(4 * n)
    with base_library(base):
        kb = lib.KeyTable(key_len, n_slots)
    ks = lib.KeyTable(key_len, n_slots)
    for k in (kb, ks):
        k.set(0, keys); k.set_salt(0, salts); k.set_xpn(0, xsalts, sscis)
    tc = lib.TxCounters(n_ctrs, n)
    nexts, limits = [int(s) for s in start], [2 ** 64 - 1] * n_ctrs
    lib.dev_sync()

    def send():
        tc.assign_dev(tf, n, d_ctr.ptr, d_work.ptr, d_off.ptr, d_num.ptr, d_hi.ptr, d_slots.ptr)
        ks.frames_crypt_x_dev(0, xf, n, d_slots.ptr, d_hi.ptr, d_work.ptr, d_off.ptr, d_out["txnum"].ptr)
    runs = {"base": lambda: kb.frames_crypt_x_dev(0, xf, n, d_slots_in.ptr, d_his.ptr, d_numbered.ptr, d_off.ptr, d_out["base"].ptr), "txnum": send}
    before = {"base": lambda: None, "txnum": lambda: tc.set(0, nexts, limits)}
    ms = alternate(runs, before, reps, rounds)
    lib.dev_sync()
    # what must hold: the numbers are start_c + rank in array order; both sides leave the same frames; nothing was refused; every counter moved by its count
    got_num = np.frombuffer(bytes(d_num.download(8 * n)), dtype=np.uint64)
    got_hi = np.frombuffer(bytes(d_hi.download(4 * n)), dtype=np.uint32)
    out = {k: hashlib.sha256(bytes(d_out[k].download(plain.nbytes))).hexdigest() for k in SIDES}
    ok = bool((got_num == nums).all() and (got_hi == his).all() and out["base"] == out["txnum"])
    ok = ok and tc.get()[0] == [int(s) + int(c) for s, c in zip(start, count)] and bytes(d_slots.download(4 * n)) == slots.tobytes()
    med = {k: [statistics.median(r) for r in v] for k, v in ms.items()}
    us = {k: 1e3 * statistics.median(v) for k, v in med.items()}
    r = {"case": name, "n_frames": n, "n_ctrs": n_ctrs, "key_bits": 8 * key_len, "bytes": int(off[-1]), "reps": reps, "rounds": rounds,
         "ms": {k: [[round(x, 4) for x in rr] for rr in v] for k, v in ms.items()}, "round_medians_us": {k: [round(1e3 * x, 1) for x in v] for k, v in med.items()},
         "median_us": {k: round(v, 1) for k, v in us.items()}, "base_spread_us": round(1e3 * (max(med["base"]) - min(med["base"])), 1),
         "added_us": round(us["txnum"] - us["base"], 1), "added_share_of_encrypt": round((us["txnum"] - us["base"]) / us["base"], 4),
         "checks_ok": ok, "status": [list(kb.status()), list(ks.status()), list(tc.status())]}
    print(json.dumps(r), flush=True)
    kb.close(); ks.close(); tc.close()
    for b in [d_slots_in, d_ctr, d_off, d_his, d_numbered, d_work, d_slots, d_num, d_hi] + list(d_out.values()):
        b.free()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--base", required=True, help="libaesgcm_hip.so built at the parent commit")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=HERE)
    a = ap.parse_args()
    assert a.reps >= 5 and a.rounds >= 3
    rng = np.random.default_rng(20261019)
    dev_name = lib.device_name(0)
    so = os.path.join(os.path.dirname(os.path.abspath(lib.__file__)), "libaesgcm_hip.so")
    sha = hashlib.sha256(open(so, "rb").read()).hexdigest()[:16]
    bsha = hashlib.sha256(open(a.base, "rb").read()).hexdigest()[:16]
    print("device:", dev_name, "library sha256:", sha, "base library sha256:", bsha, flush=True)
    base = load_base(a.base)
    rows = [case("a_4096_on_64", base, 4096, 64, a.reps, a.rounds, rng), case("b_4096_on_1", base, 4096, 1, a.reps, a.rounds, rng),
            case("c_2^20_on_64", base, 1 << 20, 64, a.reps, a.rounds, rng), case("d_2^20_on_1", base, 1 << 20, 1, a.reps, a.rounds, rng)]
    lines = ["device: %s; libaesgcm_hip.so sha256 %s...; baseline: the parent commit's library (sha256 %s...): aesgcm_keytab_frames_crypt_x_dev, XPN encrypt, alone; against"
             % (dev_name, sha, bsha),
             "assign (MACsec XPN) + the same encrypt call of this build on the same frames (AES-256, 64 slots, byte-packed, 64 .. 1514 payload bytes); %d rounds of %d alternated calls;" % (a.rounds, a.reps),
             "microseconds per call, per side the median of the round medians; spread = max - min of the base call's round medians; added = send loop - encrypt alone",
             "%-14s %8s %5s | %9s %7s | %9s | %8s %7s | %s" % ("case", "frames", "ctrs", "encrypt", "spread", "send", "added", "share", "checks")]
    for r in rows:
        lines.append("%-14s %8d %5d | %9.1f %7.1f | %9.1f | %8.1f %6.1f%% | %s" % (
            r["case"], r["n_frames"], r["n_ctrs"], r["median_us"]["base"], r["base_spread_us"], r["median_us"]["txnum"], r["added_us"], 100 * r["added_share_of_encrypt"], r["checks_ok"]))
    for small, big in ((rows[0], rows[1]), (rows[2], rows[3])):
        diff, spread = big["median_us"]["txnum"] - small["median_us"]["txnum"], max(small["base_spread_us"], big["base_spread_us"])
        lines.append("%d frames: ONE counter - 64 counters = %+.1f us (the larger base spread: %.1f us): %s" % (
            small["n_frames"], diff, spread, "within the base spread" if abs(diff) <= spread else "MORE than the base spread -- a finding"))
    print("\n".join(lines))
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "ab.txt"), "w") as f:
        f.write("\n".join(lines) + "\n\n" + "\n".join(json.dumps(r) for r in rows) + "\n")
    assert all(r["checks_ok"] and r["status"] == [[0, 0], [0, 0], [0, 0]] for r in rows), "a check failed"


if __name__ == "__main__":
    main()
