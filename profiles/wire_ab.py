#!/usr/bin/env python3
"""Frames in wire format against the split form of the same frames (GPU box): aesgcm_keytab_frames_crypt_dev on one byte-packed buffer of MACsec frames
(28-byte header | payload | 16-byte ICV, the nonce from the slot's salt and the header) against aesgcm_keytab_crypt_dev on the five arrays a caller had to build before
(IVs, AAD + offsets, payload + offsets, tags) -- the same frame bytes, 20 bytes per frame less of side arrays.
    (b) 2^20 frames of 64 .. 1514 payload bytes, AES-256, 64 slots, byte-packed      (c) 4096 such frames (a small call)          encrypt and decrypt each
The baseline is the library given with --baseline-so (build the PARENT commit's csrc and pass its libaesgcm_hip.so); without it, this build's own
aesgcm_keytab_crypt_dev (whose kernels this change leaves as they were).  Same process, same device, calls ALTERNATED, --reps repetitions each (>= 5), timed with
events on the launch stream; median, min and max per side.  The outputs of the two sides are compared once per case.  Condition: the wire call's median rate is not below
the baseline's median by more than the baseline's own max - min.
    python profiles/wire_ab.py [--reps 9] [--out profiles/wire] [--baseline-so PATH]"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import aesgcm_amd  # noqa: E402,F401
from aesgcm_amd import lib  # noqa: E402

HDR, ICV = 28, 16


def dev(arr):
    b = lib.DeviceBuffer(max(arr.nbytes, 16))
    b.upload(arr.tobytes())
    return b


class Baseline:
    """aesgcm_keytab_crypt_dev of another build of the library (or of this one) on the split form"""

    def __init__(self, so, key_len, n_slots, keys):
        vp, sz, cint = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
        self.L = ctypes.CDLL(so) if so else lib._keytab_typed(lib.load())
        self.L.aesgcm_keytab_create.argtypes = [ctypes.POINTER(vp), cint, sz, sz]
        self.L.aesgcm_keytab_set.argtypes = [vp, sz, sz, vp, vp]
        self.L.aesgcm_keytab_crypt_dev.argtypes = [vp, cint, sz, vp, vp, vp, sz, vp, vp, sz, vp, vp, vp, vp, vp, vp]
        self.L.aesgcm_keytab_destroy.argtypes = [vp]
        t = vp()
        assert self.L.aesgcm_keytab_create(ctypes.byref(t), 0, key_len, n_slots) == 0
        self.t = t.value
        assert self.L.aesgcm_keytab_set(self.t, 0, n_slots, keys, None) == 0

    def crypt(self, decrypt, n, d_slots, d_ivs, d_aad, d_aoff, d_in, d_doff, d_out, d_tags, d_expect=None, d_auth=None):
        rc = self.L.aesgcm_keytab_crypt_dev(self.t, decrypt, n, d_slots, d_ivs, d_aad, 0, d_aoff, d_in, 0, d_doff, d_out, d_tags, d_expect, d_auth, None)
        assert rc == 0, rc

    def close(self):
        self.L.aesgcm_keytab_destroy(self.t)


def alternate(run_base, run_wire, reps):
    t = lib.Timer()
    run_base(); run_wire(); run_base(); run_wire()            # every shape warmed up
    lib.dev_sync()
    ms = {"base": [], "wire": []}
    for _ in range(reps):
        for k, fn in (("base", run_base), ("wire", run_wire)):
            t.start(); fn(); t.stop()
            ms[k].append(t.ms())
    t.close()
    return ms


def case(name, n, n_slots, key_len, lens, reps, rng, baseline_so):
    keys = rng.integers(0, 256, size=n_slots * key_len, dtype=np.uint8).tobytes()
    salts = rng.integers(0, 256, size=n_slots * 8, dtype=np.uint8).tobytes()
    slots = rng.integers(0, n_slots, size=n, dtype=np.uint32)
    woff = np.zeros(n + 1, dtype=np.uint64); woff[1:] = np.cumsum(lens + np.uint64(HDR + ICV), dtype=np.uint64)
    doff = np.zeros(n + 1, dtype=np.uint64); doff[1:] = np.cumsum(lens, dtype=np.uint64)
    aoff = np.arange(n + 1, dtype=np.uint64) * HDR
    wire = rng.integers(0, 256, size=int(woff[n]), dtype=np.uint8)
    # the split form of the same frames: header -> AAD array, salt || PN -> IV array, payload -> data array
    hdr_at = woff[:-1].astype(np.int64)[:, None] + np.arange(HDR, dtype=np.int64)[None, :]
    aad = wire[hdr_at]                                         # n x 28
    salt_arr = np.frombuffer(salts, dtype=np.uint8).reshape(n_slots, 8)
    ivs = np.concatenate([salt_arr[slots], aad[:, 16:20]], axis=1)
    data = np.empty(int(doff[n]), dtype=np.uint8)
    wl, dl = woff.tolist(), doff.tolist()
    for p in range(n):
        data[dl[p]:dl[p + 1]] = wire[wl[p] + HDR:wl[p + 1] - ICV]
    fmt = lib.WireFormat.macsec()
    d_slots, d_woff, d_doff, d_aoff = dev(slots), dev(woff), dev(doff), dev(aoff)
    d_wire, d_wct, d_wpt = dev(wire), lib.DeviceBuffer(wire.nbytes + 64), lib.DeviceBuffer(wire.nbytes + 64)
    d_data, d_ct, d_pt = dev(data), lib.DeviceBuffer(data.nbytes + 64), lib.DeviceBuffer(data.nbytes + 64)
    d_aad, d_ivs = dev(np.ascontiguousarray(aad)), dev(np.ascontiguousarray(ivs))
    d_tags, d_tags2 = lib.DeviceBuffer(16 * n), lib.DeviceBuffer(16 * n)
    d_auth_w, d_auth_b = lib.DeviceBuffer(4 * n), lib.DeviceBuffer(4 * n)
    kt = lib.KeyTable(key_len, n_slots)
    kt.set(0, keys); kt.set_salt(0, salts)
    base = Baseline(baseline_so, key_len, n_slots, keys)
    frame_bytes = int(doff[n]) + HDR * n                       # what both sides encrypt and authenticate
    rows = []
    for decrypt in (0, 1):
        if not decrypt:
            run_w = lambda: kt.frames_crypt_dev(False, fmt, n, d_slots.ptr, d_wire.ptr, d_woff.ptr, d_wct.ptr)  # noqa: E731
            run_b = lambda: base.crypt(0, n, d_slots.ptr, d_ivs.ptr, d_aad.ptr, d_aoff.ptr, d_data.ptr, d_doff.ptr, d_ct.ptr, d_tags.ptr)  # noqa: E731
        else:
            run_w = lambda: kt.frames_crypt_dev(True, fmt, n, d_slots.ptr, d_wct.ptr, d_woff.ptr, d_wpt.ptr, d_auth=d_auth_w.ptr)  # noqa: E731
            run_b = lambda: base.crypt(1, n, d_slots.ptr, d_ivs.ptr, d_aad.ptr, d_aoff.ptr, d_ct.ptr, d_doff.ptr, d_pt.ptr, d_tags2.ptr, d_tags.ptr, d_auth_b.ptr)  # noqa: E731
        ms = alternate(run_b, run_w, reps)
        lib.dev_sync()
        # the two sides once against each other: payload bytes and ICV of every frame
        w = np.frombuffer(bytes((d_wpt if decrypt else d_wct).download(wire.nbytes)), dtype=np.uint8)
        s = np.frombuffer(bytes((d_pt if decrypt else d_ct).download(data.nbytes)), dtype=np.uint8)
        tg = np.frombuffer(bytes(d_tags.download(16 * n)), dtype=np.uint8).reshape(n, 16)
        icv_at = (woff[1:].astype(np.int64) - ICV)[:, None] + np.arange(ICV, dtype=np.int64)[None, :]
        same = bool((w[icv_at] == tg).all()) and bool((w[hdr_at] == aad).all())
        for p in range(0, n, max(1, n // 4096)):               # payloads: a stride of frames (every frame of the small case)
            same = same and bool((w[wl[p] + HDR:wl[p + 1] - ICV] == s[dl[p]:dl[p + 1]]).all())
        if decrypt:
            aw = np.frombuffer(bytes(d_auth_w.download(4 * n)), dtype=np.int32)
            ab = np.frombuffer(bytes(d_auth_b.download(4 * n)), dtype=np.int32)
            same = same and bool((aw == 1).all()) and bool((ab == 1).all())
        gib = frame_bytes / (1 << 30)
        rate = {k: sorted(gib / (x / 1e3) for x in v) for k, v in ms.items()}
        r = {"case": name, "op": "decrypt" if decrypt else "encrypt", "key_bits": 8 * key_len, "n_frames": n, "n_slots": n_slots, "frame_bytes": frame_bytes,
             "reps": reps, "baseline": "parent build" if baseline_so else "this build's aesgcm_keytab_crypt_dev",
             "base_ms": [round(x, 4) for x in ms["base"]], "wire_ms": [round(x, 4) for x in ms["wire"]],
             "base_gib_s": {"median": round(statistics.median(rate["base"]), 1), "min": round(rate["base"][0], 1), "max": round(rate["base"][-1], 1)},
             "wire_gib_s": {"median": round(statistics.median(rate["wire"]), 1), "min": round(rate["wire"][0], 1), "max": round(rate["wire"][-1], 1)},
             "outputs_equal": same, "status": list(kt.status())}
        r["condition_met"] = r["wire_gib_s"]["median"] >= r["base_gib_s"]["median"] - (r["base_gib_s"]["max"] - r["base_gib_s"]["min"])
        print(json.dumps(r), flush=True)
        rows.append(r)
    kt.close(); base.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "wire"))
    ap.add_argument("--baseline-so", default=None)
    ap.add_argument("--frames", type=int, default=1 << 20)
    a = ap.parse_args()
    assert a.reps >= 5
    rng = np.random.default_rng(20261016)
    dev_name = lib.device_name(0)
    print("device:", dev_name, flush=True)
    lens = rng.integers(64, 1515, size=a.frames).astype(np.uint64)
    rows = case("b_macsec_%d" % a.frames, a.frames, 64, 32, lens, a.reps, rng, a.baseline_so)
    rows += case("c_macsec_4096", 4096, 64, 32, lens[:4096], a.reps, rng, a.baseline_so)
    lines = ["device: %s; baseline: %s; %d alternated repetitions; GiB/s over header + payload bytes" % (dev_name, rows[0]["baseline"], a.reps),
             "%-18s %-8s %9s | %28s | %28s | %s %s" % ("case", "op", "frames", "split form  median (min .. max)", "wire format median (min .. max)", "condition", "same")]
    for r in rows:
        b, w = r["base_gib_s"], r["wire_gib_s"]
        lines.append("%-18s %-8s %9d | %12.1f (%6.1f .. %6.1f) | %12.1f (%6.1f .. %6.1f) | %-9s %s" % (
            r["case"], r["op"], r["n_frames"], b["median"], b["min"], b["max"], w["median"], w["min"], w["max"], "met" if r["condition_met"] else "NOT met", r["outputs_equal"]))
    print("\n".join(lines))
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "ab.txt"), "w") as f:
        f.write("\n".join(lines) + "\n\n" + "\n".join(json.dumps(r) for r in rows) + "\n")
    assert all(r["outputs_equal"] and r["status"] == [0, 0] for r in rows), "the wire call and the split form differ"


if __name__ == "__main__":
    main()
