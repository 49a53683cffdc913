#!/usr/bin/env python3
"""Receive windows: what recover + commit add to a decrypt call (GPU box).  The base side is the PARENT commit's ESN decrypt call alone (--base, a libaesgcm_hip.so built
there; both libraries live in this one process, as in profiles/srtp/ab.py): aesgcm_keytab_frames_crypt_x_dev with d_hi given.  The other side is this build's receive
loop on the same frames: aesgcm_rxwin_recover_dev (LOWEST: d_hi from the windows) + the same decrypt call + aesgcm_rxwin_commit_dev -- five launches for one.
    (a) 2^20 MACsec-shaped frames (64 .. 1514 payload bytes, byte-packed) on 64 windows     (b) 4096 such frames on 64 windows
    (c) the worst case for the atomics: the 2^20 frames all on ONE window
AES-256, ESP with ESN, 64 slots, windows of 4096 bits.  Every window's numbers run upwards across 2^32 in frame order with a little reordering, so in (a) and (c) a call
spans more than the window and its oldest frames are OLD -- the commit's work per frame is the same.  The windows are set back before every timed call, outside the timed
region, so every repetition accepts afresh.  Same process, same device, calls ALTERNATED, --reps calls per side and round, --rounds rounds, timed with events on the launch
stream.  Per side: the median of each round, and the median of those.  Spread = max - min of the base call's round medians.
    python profiles/rxwin/ab.py --base PATH/libaesgcm_hip.so [--reps 9] [--rounds 3]"""
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

SIDES = ("base", "rxwin")
W = 4096


def load_base(path):
    """the parent commit's library, typed as far as this script calls it"""
    L = lib._typed(ctypes.CDLL(path))
    vp, sz, cint, u64 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_uint64
    L.aesgcm_keytab_create.argtypes = [ctypes.POINTER(vp), cint, sz, sz]
    L.aesgcm_keytab_set.argtypes = [vp, sz, sz, vp, vp]
    L.aesgcm_keytab_set_salt.argtypes = [vp, sz, sz, vp, vp]
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


def case(name, base, n, n_wins, reps, rounds, rng):
    key_len, n_slots = 32, 64
    xf, rf = lib.WireFormatX.esp_esn(16), lib.RxFormat.esp_esn()
    keys = rng.integers(0, 256, size=n_slots * key_len, dtype=np.uint8).tobytes()
    salts = rng.integers(0, 256, size=n_slots * 8, dtype=np.uint8).tobytes()
    slots = rng.integers(0, n_slots, size=n, dtype=np.uint32)
    wins = (slots % n_wins).astype(np.uint32)
    lens = rng.integers(64, 1515, size=n, dtype=np.int64) + 32            # 16 bytes of ESP header and IV field, 16 of ICV
    off = np.zeros(n + 1, dtype=np.uint64)
    off[1:] = np.cumsum(lens).astype(np.uint64)
    # window w's k-th frame carries number start_w + k, neighbours swapped here and there; every window crosses 2^32 inside the call
    count = np.bincount(wins, minlength=n_wins)
    start = (1 << 32) - count // 2
    rank = np.zeros(n, dtype=np.int64)
    for w in range(n_wins):
        idx = np.nonzero(wins == w)[0]
        r = np.arange(len(idx), dtype=np.int64)
        sw = np.nonzero(rng.integers(0, 4, size=len(idx) // 2) == 0)[0] * 2
        r[sw], r[sw + 1] = r[sw + 1].copy(), r[sw].copy()
        rank[idx] = r
    nums = (start[wins] + rank).astype(np.uint64)
    wire = rng.integers(0, 256, size=int(off[-1]), dtype=np.uint8)
    first = off[:-1].astype(np.int64)
    for k in range(4):
        wire[first + 4 + k] = ((nums >> np.uint64(8 * (3 - k))) & np.uint64(0xFF)).astype(np.uint8)
    his = (nums >> np.uint64(32)).astype(np.uint32)
    d_slots, d_wins, d_off, d_his, d_plain = dev(slots), dev(wins), dev(off), dev(his), dev(wire)
    nb = wire.nbytes + 64
    d_ct = lib.DeviceBuffer(nb)
    d_pt = {k: lib.DeviceBuffer(nb) for k in SIDES}
    d_auth = {k: lib.DeviceBuffer(4 * n) for k in SIDES}
    d_num, d_hi, d_accept, d_why = lib.DeviceBuffer(8 * n), lib.DeviceBuffer(4 * n), lib.DeviceBuffer(4 * n), lib.DeviceBuffer(4 * n)
    with base_library(base):
        kb = lib.KeyTable(key_len, n_slots)
    ks = lib.KeyTable(key_len, n_slots)
    kb.set(0, keys); kb.set_salt(0, salts)
    ks.set(0, keys); ks.set_salt(0, salts)
    rw = lib.RxWindows(n_wins, W)
    nexts = [int(s) for s in start]
    ks.frames_crypt_x_dev(0, xf, n, d_slots.ptr, d_his.ptr, d_plain.ptr, d_off.ptr, d_ct.ptr)
    lib.dev_sync()

    def receive():
        rw.recover_dev(rf, n, d_wins.ptr, d_ct.ptr, d_off.ptr, d_num.ptr, d_hi.ptr)
        ks.frames_crypt_x_dev(1, xf, n, d_slots.ptr, d_hi.ptr, d_ct.ptr, d_off.ptr, d_pt["rxwin"].ptr, d_auth=d_auth["rxwin"].ptr)
        rw.commit_dev(n, d_wins.ptr, d_num.ptr, d_auth["rxwin"].ptr, d_accept.ptr, d_why.ptr)
    runs = {"base": lambda: kb.frames_crypt_x_dev(1, xf, n, d_slots.ptr, d_his.ptr, d_ct.ptr, d_off.ptr, d_pt["base"].ptr, d_auth=d_auth["base"].ptr), "rxwin": receive}
    before = {"base": lambda: None, "rxwin": lambda: rw.set(0, nexts)}
    ms = alternate(runs, before, reps, rounds)
    lib.dev_sync()
    auth = {k: np.frombuffer(bytes(d_auth[k].download(4 * n)), dtype=np.int32) for k in SIDES}
    why = np.frombuffer(bytes(d_why.download(4 * n)), dtype=np.int32)
    accept = np.frombuffer(bytes(d_accept.download(4 * n)), dtype=np.int32)
    got_num = np.frombuffer(bytes(d_num.download(8 * n)), dtype=np.uint64)
    # what must hold: every tag verifies on both sides; the recovered numbers are the senders'; a frame is accepted unless it lies more than W below its window's largest
    top = np.zeros(n_wins, dtype=np.uint64)
    np.maximum.at(top, wins, nums)
    old = (top[wins] - nums) >= np.uint64(W)
    ok = bool((auth["base"] == 1).all() and (auth["rxwin"] == 1).all() and (got_num == nums).all() and (why[old] == 2).all() and (why[~old] == 1).all()
              and (accept == (why == 1)).all())
    got_next = rw.get()[0]
    ok = ok and got_next == [int(t) + 1 for t in top]
    med = {k: [statistics.median(r) for r in v] for k, v in ms.items()}
    us = {k: 1e3 * statistics.median(v) for k, v in med.items()}
    r = {"case": name, "n_frames": n, "n_wins": n_wins, "window": W, "key_bits": 8 * key_len, "bytes": int(off[-1]), "reps": reps, "rounds": rounds,
         "ms": {k: [[round(x, 4) for x in rr] for rr in v] for k, v in ms.items()}, "round_medians_us": {k: [round(1e3 * x, 1) for x in v] for k, v in med.items()},
         "median_us": {k: round(v, 1) for k, v in us.items()}, "base_spread_us": round(1e3 * (max(med["base"]) - min(med["base"])), 1),
         "added_us": round(us["rxwin"] - us["base"], 1), "added_share_of_decrypt": round((us["rxwin"] - us["base"]) / us["base"], 4),
         "accepted": int((why == 1).sum()), "old": int((why == 2).sum()), "checks_ok": ok, "status": [list(kb.status()), list(ks.status()), list(rw.status())]}
    print(json.dumps(r), flush=True)
    kb.close(); ks.close(); rw.close()
    for b in [d_slots, d_wins, d_off, d_his, d_plain, d_ct, d_num, d_hi, d_accept, d_why] + [x for d in (d_pt, d_auth) for x in d.values()]:
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
    rows = [case("a_2^20_on_64", base, 1 << 20, 64, a.reps, a.rounds, rng), case("b_4096_on_64", base, 4096, 64, a.reps, a.rounds, rng),
            case("c_2^20_on_1", base, 1 << 20, 1, a.reps, a.rounds, rng)]
    lines = ["device: %s; libaesgcm_hip.so sha256 %s...; baseline: the parent commit's library (sha256 %s...): aesgcm_keytab_frames_crypt_x_dev, ESN decrypt, alone; against"
             % (dev_name, sha, bsha),
             "recover (LOWEST) + the same decrypt call + commit of this build on the same frames (AES-256, 64 slots, windows of %d bits); %d rounds of %d alternated calls;" % (W, a.rounds, a.reps),
             "microseconds per call, per side the median of the round medians; spread = max - min of the base call's round medians; added = receive loop - decrypt alone",
             "%-14s %8s %5s | %9s %7s | %9s | %8s %7s | %9s %8s | %s" % ("case", "frames", "wins", "decrypt", "spread", "receive", "added", "share", "accepted", "old", "checks")]
    for r in rows:
        lines.append("%-14s %8d %5d | %9.1f %7.1f | %9.1f | %8.1f %6.1f%% | %9d %8d | %s" % (
            r["case"], r["n_frames"], r["n_wins"], r["median_us"]["base"], r["base_spread_us"], r["median_us"]["rxwin"], r["added_us"], 100 * r["added_share_of_decrypt"],
            r["accepted"], r["old"], r["checks_ok"]))
    print("\n".join(lines))
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "ab.txt"), "w") as f:
        f.write("\n".join(lines) + "\n\n" + "\n".join(json.dumps(r) for r in rows) + "\n")
    assert all(r["checks_ok"] and r["status"] == [[0, 0], [0, 0], [0, 0]] for r in rows), "a check failed"


if __name__ == "__main__":
    main()
