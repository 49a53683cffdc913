"""Walks every cell of the single-message grid (tests/msg_grid.py) over the fake runtime and holds the launch log of each call to what the cell's shape names:
that a shape FORCED by context options is the shape taken, without a GPU.  Per shape every message through aesgcm_encrypt_dev and aesgcm_decrypt_dev -- k_main
alone with static waves; k_main with dealt chunks (nq != 0); one dealt k_body launch with the k_main tail behind it, closed by k_combine, or by k_fold where the
range is one aligned body; a k_fold level present above 64 chunk items; one k_body launch of cyclic rows alone (cyc_close 1), with k_fold and k_combine behind it
(cyc_close 0), in the half shape (k_bodyh), and k_main where the AAD has more front rows than the launch has strands -- and what aesgcm_ctx_last_launch and
aesgcm_ctx_split answer; then the shards and streaming sessions of the GPU test under their forced options.  Nothing runs: every device buffer is 32 bytes.

    make -C tests/fake_hip -s libaesgcm_fake.so && AESGCM_LIB=tests/fake_hip/libaesgcm_fake.so python tests/fake_hip/msg_grid_drive.py

prints a line per shape and MSG GRID PLAN OK (tests/test_msg_grid_cpu.py)."""
import ctypes
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
os.environ.setdefault("AESGCM_LIB", os.path.join(HERE, "libaesgcm_fake.so"))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
import aesgcm_amd  # noqa: E402,F401
from aesgcm_amd import lib  # noqa: E402
import msg_grid as MG  # noqa: E402

lib.load()
F = ctypes.CDLL(os.environ["AESGCM_LIB"])
F.fake_log.restype = ctypes.c_size_t
F.fake_log.argtypes = [ctypes.c_char_p, ctypes.c_size_t]
F.fake_log_runtime(1)
KEY, IV = bytes(range(32)), bytes(range(1, 13))
bufs = [lib.DeviceBuffer(32) for _ in range(4)]
d_aad, d_in, d_out, d_partial = (b.ptr for b in bufs)

U = MG.units(lib)
assert U == MG.FAKE_UNITS, (U, MG.FAKE_UNITS)
assert (MG.LAUNCH_MAIN, MG.LAUNCH_CYCLIC, MG.LAUNCH_CYCLIC_HALF, MG.LAUNCH_DEALT) == (lib.LAUNCH_MAIN, lib.LAUNCH_CYCLIC, lib.LAUNCH_CYCLIC_HALF, lib.LAUNCH_DEALT)


def context(opts):
    c = lib.Context(KEY)
    for o, v in opts:
        c.set_option(o, v)
    return c


def launches(call):
    """the kernels the call launched: [(name, {field: value})]"""
    F.fake_reset()
    call()
    b = ctypes.create_string_buffer(1 << 16)
    assert F.fake_log(b, len(b)) <= len(b)
    out = []
    for line in b.value.decode().splitlines():
        w = line.split()
        if w and w[0].startswith("k_"):
            out.append((w[0], dict(x.split("=", 1) for x in w[2:] if "=" in x)))
    return out


def hold(log, e, what):
    """the launch log against MG.expected's answer"""
    names = [k for k, _ in log]
    bodies = [f for k, f in log if k == "k_body"]
    mains = [f for k, f in log if k == "k_main"]
    assert set(names) <= {"k_main", "k_body", "k_fold", "k_combine"}, (what, names)
    assert len(bodies) == int(e["body"]), (what, names)
    if e["body"]:
        b = bodies[0]
        assert (b.get("cyc") == "1") == e["cyc"] and (b.get("half") == "1") == e["half"], (what, b)
        if e["cyc"]:
            assert b["cw"] == str(U["W_half"] if e["half"] else U["W"]) and (b.get("fuse") == "1") == (e["last"] == "k_body"), (what, b)
            assert not mains, (what, names)                     # AAD, rows and the ragged end in the one launch
        else:
            assert "nq" in b or int(b["C"]) < 512, (what, b)     # dealt chunks
            at = names.index("k_body")
            assert ("k_main" in names[at + 1:]) == e["tail"], (what, names)
    else:
        assert len(mains) <= 1 and (mains or " 0+0 " in what), (what, names)          # (nothing to encrypt and nothing to hash: k_combine alone)
        assert all(("nq" in m and m["nq"] != "0") == e["main_dealt"] for m in mains), (what, mains)
        if e["main_dealt"]:
            assert int(mains[0]["C"]) + 1 > U["main_waves"], (what, mains)
    if e["fold"]:
        assert "k_fold" in names, (what, names)
    if e["last"] == "k_body":
        assert names == ["k_body"], (what, names)
    elif e["last"]:
        assert names[-1] == e["last"] and (e["last"] != "k_fold" or "k_combine" not in names), (what, names)
    elif names:
        assert names[-1] in ("k_main", "k_combine"), (what, names)


cells = 0
for s in MG.SHAPES:
    g = MG.grid(s.name, U)
    c = context(s.opts)
    seen = set()
    for i in range(g.n):
        L, a = g.lens[i], g.aads[i]
        e = MG.expected(s, L, a, U)
        what = "%s %r %d+%d" % (s.name, g.cells[i], L, a)
        for dec in (False, True):
            fn = c.decrypt_dev if dec else c.encrypt_dev
            log = launches(lambda: fn(IV, d_in, L, d_out, d_aad=d_aad + g.pos_aad[i] % 16 if a else None, aad_len=a))
            hold(log, e, what + (" dec" if dec else " enc"))
            assert c.last_launch() == e["launch"], (what, c.last_launch(), e["launch"])
            assert e["split"] is None or c.split(L) == e["split"], (what, c.split(L), e["split"])
        seen.add((e["launch"], e["last"], e["tail"]))
        cells += 1
    print("%-12s %3d messages, %5.1f MiB: %s" % (s.name, g.n, g.size_in / 2 ** 20, sorted(seen, key=str)))

# shards: every rank's range through k_body under the forced options, by dealt chunks or by cyclic rows
for how, opts in MG.SHARD_OPTS.items():
    c = context(opts)
    for ranks in (3, 5):
        for r, (first, ln) in enumerate(MG.shard_ranges(ranks, U)):
            for dec in (0, 1):
                log = launches(lambda: c.shard_crypt_dev(dec, IV, d_in, ln, d_out, first, MG.SHARD_LEN, d_partial, d_aad=d_aad if r == 0 else None, aad_len=MG.SHARD_AAD if r == 0 else 0))
                bodies = [f for k, f in log if k == "k_body"]
                assert len(bodies) == 1 and (bodies[0].get("cyc") == "1") == (how == "cyclic") and log[-1][0] == "k_combine", (how, ranks, r, log)
                assert c.split(ln, first)[1] > 0 and c.split(ln, first)[0] == (-first) % U["A"]
                cells += 1

# streaming chunks: a chunk takes what a shard of its size takes
for how, opts in MG.STREAM_OPTS.items():
    for sizes in MG.stream_sessions(U):
        for dec in (False, True):
            c = context(opts)
            c.stream_begin(IV, dec)
            c.stream_aad(bytes(MG.STREAM_AAD))
            first = 0
            for n in sizes:
                log = launches(lambda: c.stream_update_dev(d_in, n, d_out))
                bodies = [f for k, f in log if k == "k_body"]
                head = (-first) % U["A"]
                rows = max(n // 16 - head, 0) // U["R"]               # whole rows behind the chunk's head
                first += n // 16
                if how == "main" or rows < 4:
                    assert not bodies and [k for k, _ in log][0] == "k_main", (how, n, log)
                else:
                    assert len(bodies) == 1 and (bodies[0].get("cyc") == "1") == (how == "cyclic"), (how, n, log)
                cells += 1
            c.stream_final()
print("MSG GRID PLAN OK (%d calls' shapes held)" % cells)
