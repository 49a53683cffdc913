#!/usr/bin/env python3
"""Key tables against the batch entry points on the same packets (GPU box): aesgcm_keytab_crypt_dev with a slot per packet against aesgcm_batch_crypt_dev /
aesgcm_batch_crypt_var_dev given the gathered keys keys[slot[p]] -- the same kernel loop, with and without the per-packet key schedule, H = E_K(0) and squaring chain.
    (a) 2^20 x 4 KiB, AES-128, 1024 slots (cfg5's shape)
    (b) 2^20 MACsec frames of 64 .. 1514 bytes + 28 bytes of AAD, AES-256, 64 slots, byte-packed
    (c) 4096 such frames (a small call)
    and the cost of `set` for 65 536 slots of each key size.
Best of --reps launches each, timed with HIP events on the launch stream; the two paths' outputs are compared once per case.  One JSON line per case, then a table.
    python profiles/keytab_ab.py [--reps 20] [--out DIR]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import aesgcm_amd  # noqa: E402,F401
from aesgcm_amd import lib  # noqa: E402


def timed(fn, reps):
    t = lib.Timer()
    best = 1e30
    fn()
    lib.dev_sync()
    for _ in range(reps):
        t.start(); fn(); t.stop()
        best = min(best, t.ms())
    t.close()
    return best


def dev(arr):
    b = lib.DeviceBuffer(max(arr.nbytes, 16))
    b.upload(arr.tobytes())
    return b


def case(name, key_len, n, n_slots, lens, aad_len, var, reps, rng):
    keys = rng.integers(0, 256, size=(n_slots, key_len), dtype=np.uint8)
    slots = rng.integers(0, n_slots, size=n, dtype=np.uint32)
    gathered = np.ascontiguousarray(keys[slots])
    d_slots, d_keys = dev(slots), dev(gathered)
    d_ivs = lib.DeviceBuffer(12 * n); d_ivs.fill_splitmix64(2)
    data_bytes = int(lens.sum()) if var else n * int(lens)
    d_in = lib.DeviceBuffer(data_bytes + 64); d_in.fill_splitmix64(3)
    d_o1, d_o2 = lib.DeviceBuffer(data_bytes + 64), lib.DeviceBuffer(data_bytes + 64)
    d_t1, d_t2 = lib.DeviceBuffer(16 * n), lib.DeviceBuffer(16 * n)
    d_aad = lib.DeviceBuffer(max(aad_len * n, 16)); d_aad.fill_splitmix64(4)
    if var:
        doff = np.zeros(n + 1, dtype=np.uint64); doff[1:] = np.cumsum(lens, dtype=np.uint64)
        aoff = np.arange(n + 1, dtype=np.uint64) * aad_len
        d_doff, d_aoff = dev(doff), dev(aoff)
    kt = lib.KeyTable(key_len, n_slots)
    kt.set(0, keys.tobytes())
    if var:
        run_kt = lambda: kt.crypt_dev(False, n, d_slots.ptr, d_ivs.ptr, d_in.ptr, d_doff.ptr, d_o1.ptr, d_t1.ptr, d_aad=d_aad.ptr, d_aad_off=d_aoff.ptr)  # noqa: E731
        run_b = lambda: lib.batch_crypt_var_dev(False, n, key_len, d_keys.ptr, d_ivs.ptr, d_in.ptr, d_doff.ptr, d_o2.ptr, d_t2.ptr,  # noqa: E731
                                                d_aad=d_aad.ptr, d_aad_off=d_aoff.ptr)
    else:
        run_kt = lambda: kt.crypt_dev(False, n, d_slots.ptr, d_ivs.ptr, d_in.ptr, None, d_o1.ptr, d_t1.ptr, pkt_len=int(lens))  # noqa: E731
        run_b = lambda: lib.batch_crypt_dev(False, n, key_len, d_keys.ptr, d_ivs.ptr, d_in.ptr, int(lens), d_o2.ptr, d_t2.ptr)  # noqa: E731
    ms_b = timed(run_b, reps)
    ms_kt = timed(run_kt, reps)
    lib.dev_sync()
    same = bytes(d_t1.download()) == bytes(d_t2.download()) and bytes(d_o1.download(data_bytes)) == bytes(d_o2.download(data_bytes))
    status = kt.status()
    kt.close()
    gib = (data_bytes + aad_len * n) / (1 << 30)
    r = {"case": name, "key_bits": 8 * key_len, "n_pkts": n, "n_slots": n_slots, "bytes": data_bytes, "aad_per_pkt": aad_len,
         "lanes_per_packet": lib.batch_shape(n, 0 if var else int(lens), var_len=var),
         "batch_ms": round(ms_b, 4), "keytab_ms": round(ms_kt, 4), "batch_gib_s": round(gib / (ms_b / 1e3), 1), "keytab_gib_s": round(gib / (ms_kt / 1e3), 1),
         "speedup": round(ms_b / ms_kt, 3), "bit_identical": same, "status": list(status)}
    print(json.dumps(r), flush=True)
    return r


def set_cost(key_len, n_slots, reps, rng):
    keys = rng.integers(0, 256, size=n_slots * key_len, dtype=np.uint8).tobytes()
    d_keys = lib.DeviceBuffer(len(keys)); d_keys.upload(keys)
    d_slots = dev(np.arange(n_slots, dtype=np.uint32))
    with lib.KeyTable(key_len, n_slots) as kt:
        ms_host = timed(lambda: kt.set(0, keys), reps)
        ms_dev = timed(lambda: kt.set_dev(n_slots, d_slots.ptr, d_keys.ptr), reps)
    r = {"case": "set", "key_bits": 8 * key_len, "n_slots": n_slots, "set_ms": round(ms_host, 4), "set_dev_ms": round(ms_dev, 4),
         "set_dev_ns_per_slot": round(ms_dev * 1e6 / n_slots, 2)}
    print(json.dumps(r), flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rng = np.random.default_rng(20261016)
    print("device:", lib.device_name(0), flush=True)
    frames = rng.integers(64, 1515, size=1 << 20).astype(np.uint64)
    rows = [case("a_cfg5_4KiB", 16, 1 << 20, 1024, np.uint64(4096), 0, False, a.reps, rng),
            case("b_macsec_2^20", 32, 1 << 20, 64, frames, 28, True, a.reps, rng),
            case("c_macsec_4096", 32, 4096, 64, frames[:4096], 28, True, a.reps, rng)]
    rows += [set_cost(kl, 65536, a.reps, rng) for kl in (16, 24, 32)]
    lines = ["%-16s %4s %9s %7s %8s %10s %10s %9s %9s %8s %s" % ("case", "bits", "n_pkts", "slots", "lanes", "batch ms", "keytab ms", "batch", "keytab", "x", "same")]
    for r in rows[:3]:
        lines.append("%-16s %4d %9d %7d %8d %10.3f %10.3f %9.1f %9.1f %8.3f %s" % (r["case"], r["key_bits"], r["n_pkts"], r["n_slots"], r["lanes_per_packet"],
                                                                                 r["batch_ms"], r["keytab_ms"], r["batch_gib_s"], r["keytab_gib_s"], r["speedup"], r["bit_identical"]))
    for r in rows[3:]:
        lines.append("set %d slots, AES-%d: host keys %.3f ms, device keys %.3f ms (%.2f ns per slot)" % (r["n_slots"], r["key_bits"], r["set_ms"], r["set_dev_ms"], r["set_dev_ns_per_slot"]))
    print("\n".join(lines))
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "keytab_ab.json"), "w") as f:
            json.dump({"device": lib.device_name(0), "reps": a.reps, "rows": rows}, f, indent=1)
        with open(os.path.join(a.out, "keytab_ab.txt"), "w") as f:
            f.write("\n".join(lines) + "\n")
    assert all(r["bit_identical"] and r["status"] == [0, 0] for r in rows[:3]), "keytab and batch outputs differ"


if __name__ == "__main__":
    main()
