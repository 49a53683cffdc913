#!/usr/bin/env python3
"""Wire frames with 64-bit numbers against the base wire-format call on the same frames (GPU box): aesgcm_keytab_frames_crypt_x_dev with MACsec XPN against
aesgcm_keytab_frames_crypt_dev with the classic MACsec format, and with ESP ESN against the classic ESP format.  The extended call moves the same frame bytes plus four
bytes per frame (d_hi); the base call's kernels are the parent commit's, instruction for instruction (their assembly listings are byte-identical), so it is the baseline.
    (b) 2^20 frames of 64 .. 1514 payload bytes, AES-256, 64 slots, byte-packed      (c) 4096 such frames (a small call)          encrypt and decrypt each
Same process, same device, calls ALTERNATED, --reps calls per side and round (>= 5), --rounds rounds (>= 3), timed with events on the launch stream.  Per side: the median
of each round, and the median of those.  Allowed shortfall: the base call's own spread, max - min of its round medians in this run.  Each side decrypts what it encrypted;
every ICV must be accepted and the table's status word stay clear.
    python profiles/wirex_ab.py [--reps 9] [--rounds 3] [--out profiles/wirex]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import aesgcm_amd  # noqa: E402,F401
from aesgcm_amd import lib  # noqa: E402


def dev(arr):
    b = lib.DeviceBuffer(max(arr.nbytes, 16))
    b.upload(arr.tobytes())
    return b


def alternate(run_base, run_x, reps, rounds):
    t = lib.Timer()
    run_base(); run_x(); run_base(); run_x()                  # every shape warmed up
    lib.dev_sync()
    ms = {"base": [], "x": []}
    for _ in range(rounds):
        r = {"base": [], "x": []}
        for _ in range(reps):
            for k, fn in (("base", run_base), ("x", run_x)):
                t.start(); fn(); t.stop()
                r[k].append(t.ms())
        for k in r:
            ms[k].append(r[k])
    t.close()
    return ms


def case(name, mode, n, n_slots, key_len, lens, reps, rounds, rng):
    if mode == "xpn":
        base, xf = lib.WireFormat.macsec(), lib.WireFormatX.macsec_xpn()
    else:
        base, xf = lib.WireFormat.esp(16), lib.WireFormatX.esp_esn(16)
    hdr, icv = base.hdr_len, base.tag_len
    keys = rng.integers(0, 256, size=n_slots * key_len, dtype=np.uint8).tobytes()
    slots = rng.integers(0, n_slots, size=n, dtype=np.uint32)
    his = rng.integers(0, 1 << 32, size=n, dtype=np.uint32)
    woff = np.zeros(n + 1, dtype=np.uint64); woff[1:] = np.cumsum(lens + np.uint64(hdr + icv), dtype=np.uint64)
    wire = rng.integers(0, 256, size=int(woff[n]), dtype=np.uint8)
    d_slots, d_his, d_woff, d_wire = dev(slots), dev(his), dev(woff), dev(wire)
    d_ct = {k: lib.DeviceBuffer(wire.nbytes + 64) for k in ("base", "x")}
    d_pt = {k: lib.DeviceBuffer(wire.nbytes + 64) for k in ("base", "x")}
    d_auth = {k: lib.DeviceBuffer(4 * n) for k in ("base", "x")}
    kt = lib.KeyTable(key_len, n_slots)
    kt.set(0, keys)
    kt.set_salt(0, rng.integers(0, 256, size=n_slots * 8, dtype=np.uint8).tobytes())
    kt.set_xpn(0, rng.integers(0, 256, size=n_slots * 12, dtype=np.uint8).tobytes(), rng.integers(0, 256, size=n_slots * 4, dtype=np.uint8).tobytes())
    frame_bytes = int(woff[n]) - icv * n                       # header + payload: what both sides authenticate and (the payload) encrypt
    rows = []
    for decrypt in (0, 1):
        if not decrypt:
            run_b = lambda: kt.frames_crypt_dev(False, base, n, d_slots.ptr, d_wire.ptr, d_woff.ptr, d_ct["base"].ptr)  # noqa: E731
            run_x = lambda: kt.frames_crypt_x_dev(False, xf, n, d_slots.ptr, d_his.ptr, d_wire.ptr, d_woff.ptr, d_ct["x"].ptr)  # noqa: E731
        else:
            run_b = lambda: kt.frames_crypt_dev(True, base, n, d_slots.ptr, d_ct["base"].ptr, d_woff.ptr, d_pt["base"].ptr, d_auth=d_auth["base"].ptr)  # noqa: E731
            run_x = lambda: kt.frames_crypt_x_dev(True, xf, n, d_slots.ptr, d_his.ptr, d_ct["x"].ptr, d_woff.ptr, d_pt["x"].ptr, d_auth=d_auth["x"].ptr)  # noqa: E731
        ms = alternate(run_b, run_x, reps, rounds)
        lib.dev_sync()
        ok = True
        if decrypt:                                            # each side gets its plaintext back, every ICV accepted
            for k in ("base", "x"):
                a = np.frombuffer(bytes(d_auth[k].download(4 * n)), dtype=np.int32)
                pt = np.frombuffer(bytes(d_pt[k].download(wire.nbytes)), dtype=np.uint8)
                ok = ok and bool((a == 1).all())
                wl = woff.tolist()
                for p in range(0, n, max(1, n // 4096)):
                    ok = ok and bool((pt[wl[p]:wl[p + 1] - icv] == wire[wl[p]:wl[p + 1] - icv]).all())
        gib = frame_bytes / (1 << 30)
        med = {k: [statistics.median(r) for r in v] for k, v in ms.items()}                     # ms, per round
        rate = {k: [gib / (m / 1e3) for m in v] for k, v in med.items()}                        # GiB/s, per round
        r = {"case": name, "mode": mode, "op": "decrypt" if decrypt else "encrypt", "key_bits": 8 * key_len, "n_frames": n, "n_slots": n_slots,
             "frame_bytes": frame_bytes, "reps": reps, "rounds": rounds,
             "base_ms": [[round(x, 4) for x in rr] for rr in ms["base"]], "x_ms": [[round(x, 4) for x in rr] for rr in ms["x"]],
             "base_round_medians_gib_s": [round(x, 1) for x in rate["base"]], "x_round_medians_gib_s": [round(x, 1) for x in rate["x"]],
             "round_trip_ok": ok, "status": list(kt.status())}
        r["base_gib_s"], r["x_gib_s"] = round(statistics.median(rate["base"]), 1), round(statistics.median(rate["x"]), 1)
        r["base_spread_gib_s"] = round(max(rate["base"]) - min(rate["base"]), 1)
        r["within_base_spread"] = r["x_gib_s"] >= r["base_gib_s"] - r["base_spread_gib_s"]
        print(json.dumps(r), flush=True)
        rows.append(r)
    kt.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "wirex"))
    ap.add_argument("--frames", type=int, default=1 << 20)
    a = ap.parse_args()
    assert a.reps >= 5 and a.rounds >= 3
    rng = np.random.default_rng(20261017)
    dev_name = lib.device_name(0)
    print("device:", dev_name, flush=True)
    lens = rng.integers(64, 1515, size=a.frames).astype(np.uint64)
    rows = []
    for mode in ("xpn", "esn"):
        rows += case("b_%s_%d" % (mode, a.frames), mode, a.frames, 64, 32, lens, a.reps, a.rounds, rng)
        rows += case("c_%s_4096" % mode, mode, 4096, 64, 32, lens[:4096], a.reps, a.rounds, rng)
    lines = ["device: %s; baseline: aesgcm_keytab_frames_crypt_dev of this build (classic MACsec / ESP format, the same frames); %d rounds of %d alternated calls;"
             % (dev_name, a.rounds, a.reps),
             "GiB/s over header + payload bytes; per side the median of the round medians; spread = max - min of the base call's round medians",
             "%-16s %-8s %9s | %10s %8s | %10s | %-13s %s" % ("case", "op", "frames", "base", "spread", "extended", "within spread", "round trip")]
    for r in rows:
        lines.append("%-16s %-8s %9d | %10.1f %8.1f | %10.1f | %-13s %s" % (
            r["case"], r["op"], r["n_frames"], r["base_gib_s"], r["base_spread_gib_s"], r["x_gib_s"], "yes" if r["within_base_spread"] else "NO", r["round_trip_ok"]))
    print("\n".join(lines))
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "ab.txt"), "w") as f:
        f.write("\n".join(lines) + "\n\n" + "\n".join(json.dumps(r) for r in rows) + "\n")
    assert all(r["round_trip_ok"] and r["status"] == [0, 0] for r in rows), "a side did not get its plaintext back"


if __name__ == "__main__":
    main()
