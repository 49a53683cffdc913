"""Prints what the host side decides for SINGLE MESSAGES, call by call, from the fake runtime's launch log (fakehip.cpp: fake_log, fake_log_runtime): whole messages
on device pointers (aesgcm_encrypt_dev / aesgcm_decrypt_dev), streaming sessions, shards, aesgcm_ghash, the keystream and ECB calls, the host-buffer and the
pipelined calls -- over a grid that stands on both sides of every threshold of the single-message planner (csrc/aesgcm_msgplan.h) and under the context options
that move them.  Nothing runs: every device buffer is 16 bytes, the fake device has 256 CUs.  Per call: a `==` line that names it, the log -- a line per launch (kernel,
stream, workgroups, the parameter struct's scalars, the context's own buffers by name, other pointers as 0 / 1), per hipMemsetAsync and per hipEventRecord -- an
`rc=` line when the call was refused, and `->` with what aesgcm_ctx_last_launch answers.

    make -C tests/fake_hip -s libaesgcm_fake.so && AESGCM_LIB=tests/fake_hip/libaesgcm_fake.so python tests/fake_hip/msg_drive.py > tests/golden/launch_plan_msg.txt

tests/test_fake_hip.py compares that with the fixture.  The fixture is taken from the commit BEFORE a change to the planner: equal logs are equal launches."""
import ctypes
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
os.environ.setdefault("AESGCM_LIB", os.path.join(HERE, "libaesgcm_fake.so"))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import aesgcm_amd  # noqa: E402,F401
from aesgcm_amd import lib  # noqa: E402

lib.load()
F = ctypes.CDLL(os.environ["AESGCM_LIB"])
F.fake_log.restype = ctypes.c_size_t
F.fake_log.argtypes = [ctypes.c_char_p, ctypes.c_size_t]
F.fake_name_stream.argtypes = [ctypes.c_void_p, ctypes.c_char_p]
F.fake_log_runtime(1)
KEYS = {16: bytes(range(16)), 32: bytes(range(32))}
IV = bytes(range(1, 13))
K, M, G = 1 << 10, 1 << 20, 1 << 30

bufs = [lib.DeviceBuffer(32) for _ in range(4)]
d_aad, d_in, d_out, d_partial = (b.ptr for b in bufs)
caller_ctx = lib.Context(KEYS[32])                                      # (as in plan_drive.py: a stream of the caller's)
caller = caller_ctx.stream()
F.fake_name_stream(caller, b"caller")


def context(key=32, opts=()):
    c = lib.Context(KEYS[key])
    F.fake_name_stream(c.stream(), b"own")
    for o, v in opts:
        c.set_option(o, v)
    return c


def show(title, call, ctx=None):
    F.fake_reset()
    print("== " + title)
    try:
        call()
    except lib.AesGcmError as e:
        print("rc=%d" % e.code)
    b = ctypes.create_string_buffer(1 << 16)
    assert F.fake_log(b, len(b)) <= len(b)
    sys.stdout.write(b.value.decode())
    if ctx is not None:
        print("-> %d" % ctx.last_launch())


def size(n):
    """a length as the fixture names it: the nearest unit below and what is left"""
    for u, s in ((G, "G"), (M, "M"), (K, "K")):
        if n >= u:
            return "%d%s%s" % (n // u, s, "+%d" % (n % u) if n % u else "")
    return str(n)


def crypt(n, aad=0, dec=0, key=32, opts=(), ctx=None, din=0, dout=0, st=True):
    """aesgcm_encrypt_dev / aesgcm_decrypt_dev"""
    c = ctx or context(key, opts)
    title = "crypt %s%s %s" % (size(n), " aad" if aad else "", "dec" if dec else "enc") + "".join(" %s=%d" % ov for ov in opts)
    title += (" key=%d" % key if key != 32 else "") + (" in+%d" % din if din else "") + (" out+%d" % dout if dout else "") + ("" if st else " own")
    s = caller if st else None
    if dec:
        show(title, lambda: c.decrypt_dev(IV, d_in + din, n, d_out + dout, d_aad=d_aad if aad else None, aad_len=aad, stream=s), c)
    else:
        show(title, lambda: c.encrypt_dev(IV, d_in + din, n, d_out + dout, d_aad=d_aad if aad else None, aad_len=aad, stream=s), c)
    return c


NOCYC = (("cyc_min", 0), ("cyc_max", 0))

print("# single messages (libaesgcm_fake.so).  Per launch: kernel, stream, the launcher's arguments (w = workgroups), p = the caller's pointers, the context's buffers by name")
print("# (parts / a / b + item, tag + word, q0 / q1, ptab + table), then the parameter struct's scalars under their own names; what is 0 is left out")
# the k_main path: nothing, one chunk (k_main's tail closes), a ragged end, more chunks; the 4 and 16 marks of k_combine's tables; 64 chunks and a k_fold level
for n in (0, 16, 1000, 2 * K, 2 * K + 1, 4 * K, 5 * K, 16 * K, 17 * K, 64 * K - 1):
    crypt(n, aad=20 if n in (0, 1000, 5 * K) else 0, dec=int(n in (16, 17 * K)))
crypt(0)
for n in (64 * K, 65 * K, 256 * K, 257 * K, 16 * M, 64 * M):            # ... with the cyclic rows switched off: 64 items, 33, 64, 257 (k_fold), static and dealt chunks
    crypt(n, opts=NOCYC, aad=20 if n == 257 * K else 0)
for n in (1000, 10000, 300 * K):                                        # the chunk-width override: spacings without tables
    crypt(n, opts=NOCYC + (("tw", 3),))
crypt(1000, key=16)
crypt(1000, aad=20, st=False)
# cyclic rows: both sides of cyc_min_fused, the ragged end and the pieces, the half shape and its limit, cyc_max_fused / cyc_max_pieces
for n, aad in ((64 * K, 0), (64 * K + 1000, 0), (64 * K, 20), (M + 16, 20), (80 * M - K, 0), (80 * M, 0), (G - K, 0), (G + 1000, 0), (G, 20), (1280 * M - K, 20)):
    crypt(n, aad=aad, dec=int(n == M + 16))
for h in (0, 1, 2):
    crypt(M, opts=(("cyc_half", h),))
crypt(80 * M - K, opts=(("cyc_half", 1),))
crypt(80 * M, opts=(("cyc_half", 1),))
crypt(M, key=16, dec=1)
for n in (M, 4 * M - K, 4 * M, 8 * M + 1000):                           # cyc_close 0: k_fold and k_combine behind the launch, from cyc_min
    crypt(n, opts=(("cyc_close", 0),), aad=20 if n == 4 * M else 0)
crypt(8 * M + 1000, opts=(("cyc_close", 0), ("cyc_half", 1)))
crypt(M, opts=(("cyc_prio", 0),))
# dealt chunks: the whole aligned body (k_fold closes: first level at 1 GiB, second at 16 GiB), fold_close 0, head / body / tail through the chaining value
for n, aad in ((G, 0), (16 * G, 0), (1280 * M, 20), (1280 * M + 1000, 20), (1280 * M + 1000, 0), (2 * G + 16, 0)):
    crypt(n, aad=aad, dec=int(n == 16 * G))
crypt(G, opts=(("fold_close", 0),))
crypt(16 * G, opts=(("fold_close", 0),))
crypt(G, key=16)
for n in (4 * M - K, 4 * M, 4 * M + 1000):                              # body_min, both sides
    crypt(n, opts=NOCYC + (("body_min", 4 * M),), aad=20 if n == 4 * M + 1000 else 0)
crypt(256 * M - K, opts=NOCYC)
crypt(256 * M, opts=NOCYC)
crypt(256 * M, opts=NOCYC + (("tw", 8),))
# the refusals: unaligned data on every path
for n in (1000, M, G, 1280 * M + 1000):
    crypt(n, din=1)
    crypt(n, dout=8)
# timing: the trace, the event pairs, the muted head and tail
for n, aad in ((1000, 0), (5 * K, 0), (M, 0), (G, 0), (1280 * M + 1000, 20)):
    c = context()
    c.timing_enable(True)
    crypt(n, aad=aad, ctx=c)
    crypt(n, aad=aad, ctx=c)
c = context()
caller_ctx.wait_fused(c)                                                # (the context records its event behind every fused launch from now on)
crypt(M, ctx=c)
crypt(1000, ctx=c)
crypt(1280 * M + 1000, aad=20, ctx=c)
# calls in a row on one context: the generation numbers, the toggle of the queue sets behind a dealt launch
c = context(opts=NOCYC)
for n in (64 * M, 64 * M, 1000, 64 * M, G, G):
    crypt(n, ctx=c)
c = context()
for n in (1000, M, 5 * K, G):
    crypt(n, ctx=c, dec=1)


def session(title, steps, opts=(), dec=False):
    """a streaming session: ("aad", bytes) / ("up", bytes) through the staging buffers, ("dev", n) on device pointers and the caller's stream, then the tag"""
    c = context(opts=opts)
    show("%s begin" % title, lambda: c.stream_begin(IV, dec))
    at = 0
    for what, x in steps:
        if what == "aad":
            show("%s aad %d" % (title, len(x)), lambda: c.stream_aad(x))
        elif what == "up":
            show("%s update %d at block %d" % (title, len(x), at), lambda: c.stream_update(x))
            at += len(x) // 16
        else:
            show("%s update_dev %s at block %d" % (title, size(x), at), lambda: c.stream_update_dev(d_in, x, d_out, stream=caller))
            at += x // 16
    show("%s final" % title, lambda: c.stream_final())


session("session", [("aad", bytes(20)), ("up", bytes(4096)), ("dev", 8 * M), ("dev", 8 * M + 16), ("dev", 2 * G), ("dev", 4 * M + 1000)])
session("session dec", [("dev", 16), ("dev", 2 * G), ("dev", 3 * M), ("up", bytes(100))], dec=True)
session("session cyc_min=0 cyc_max=0", [("dev", 8 * M + 16), ("dev", 8 * M)], opts=NOCYC)


def shard(n, first, total, aad=0, dec=0, opts=()):
    c = context(opts=opts)
    show("shard %s at block %d of %s%s %s" % (size(n), first, size(total), " aad" if aad else "", "dec" if dec else "enc") + "".join(" %s=%d" % ov for ov in opts),
         lambda: c.shard_crypt_dev(dec, IV, d_in, n, d_out, first, total, d_partial, d_aad=d_aad if aad else None, aad_len=aad, stream=caller))


shard(1000, 0, 1000, aad=20)
shard(4096, 256, 16 * K)
shard(8 * M, 0, 32 * M, aad=20)
shard(8 * M, 8 * M // 16, 32 * M, dec=1)
shard(8 * M + 1000, 3 * 8 * M // 16, 32 * M + 1000)
shard(4 * G, 0, 16 * G)
shard(4 * G, 4 * G // 16, 16 * G, dec=1)
shard(4 * G, 0, 16 * G, aad=20)
shard(4 * G + 16, 16 * G // 16, 32 * G)
shard(4 * G, 4 * G // 16 + 1, 16 * G)
shard(8 * M, 0, 32 * M, opts=NOCYC)

c = context()
for n in (0, 1000, 100000, M):
    show("ghash %d" % n, lambda: c.ghash(bytes(n)))
show("keystream_dev 64 blocks from 5", lambda: c.keystream_dev(IV, 5, 64, d_out, stream=caller))
show("keystream_dev 70000 blocks", lambda: c.keystream_dev(IV, 0, 70000, d_out))
show("keystream_dev out+8", lambda: c.keystream_dev(IV, 0, 4, d_out + 8))
show("ecb_encrypt 4 blocks", lambda: c.ecb_encrypt(bytes(64)))
show("ceiling_probe 1G", lambda: c.ceiling_probe(G))                    # (k_body alone over a virtual range, timed, and the k_fold levels behind it)
show("encrypt 1000 aad (host buffers)", lambda: c.encrypt(IV, bytes(20), bytes(1000)), c)
show("decrypt 70000 (host buffers)", lambda: c.decrypt(IV, b"", bytes(70000)), c)
show("encrypt_pipelined 3000 aad, chunks of 1024", lambda: c.encrypt_pipelined(IV, bytes(20), bytes(3000), chunk_bytes=1024))
show("decrypt_pipelined 200000, one chunk", lambda: c.decrypt_pipelined(IV, b"", bytes(200000)))
