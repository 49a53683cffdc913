"""Drives the host side of the library against the fake HIP runtime (fakehip.cpp) for STREAM ORDER and ERROR PATHS, through the ordinary ctypes binding:
  * a streaming session fed on a caller's stream (aesgcm_stream_update_dev): every later step -- final, update, update_dev on another stream, aad, export -- makes its
    stream wait for that chunk on the device before it enqueues anything, and export synchronises no device;
  * a routed packet call (offset arrays: the row launches fork to the context's side stream) whose k-th launch fails, for every k up to the first that is past its
    last launch: an error, the caller's stream ordered behind everything that reached the side stream, and the next call on the context clean;
  * a call of fixed-size records through k_pktl and one through k_pktg whose launch fails: the context's packet dispenser stands where it stood -- the next call's
    launch log (fake_log) is the one a context that never saw the failure writes;
  * a multi-launch aesgcm_stream_update_dev whose k-th launch fails: an error, and the session over (ESTATE) until it is begun again.
Run by tests/test_fake_hip.py with AESGCM_LIB pointing at the fake library."""
import ctypes
import os
import struct
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import aesgcm_amd  # noqa: E402,F401
from aesgcm_amd import lib  # noqa: E402

assert os.environ.get("AESGCM_LIB", "").endswith("libaesgcm_fake.so"), "run with AESGCM_LIB = the fake library"
lib.load()
F = ctypes.CDLL(os.environ["AESGCM_LIB"])
F.fake_launches.restype = F.fake_device_syncs.restype = ctypes.c_long
F.fake_fail_launch.argtypes = [ctypes.c_long]
F.fake_watch.argtypes = F.fake_ordered_behind_all.argtypes = [ctypes.c_void_p]
F.fake_log.restype = ctypes.c_size_t
F.fake_log.argtypes = [ctypes.c_char_p, ctypes.c_size_t]


def check(what):
    b = ctypes.create_string_buffer(1 << 16)
    n = F.fake_violations(b, len(b))
    assert n == 0, "%s: %d violations\n%s" % (what, n, b.value.decode())
    F.fake_reset()


def refused(call, code):
    try:
        call()
    except lib.AesGcmError as e:
        assert e.code == code, (e.code, code)
        return
    raise AssertionError("not refused")


MB = 1 << 20
key, iv = bytes(range(32)), bytes(12)
ctx = lib.Context(key)
s1, s2 = lib.Context(key).stream(), lib.Context(key).stream()      # callers' streams
d_in, d_out = lib.DeviceBuffer(40 * MB), lib.DeviceBuffer(40 * MB)

# ---- a session's steps after a chunk on a caller's stream
for name, after in (("final", lambda: ctx.stream_final()),
                    ("update", lambda: ctx.stream_update(bytes(100))),
                    ("update_dev on another stream", lambda: ctx.stream_update_dev(d_in.ptr + 1600, 5 * MB, d_out.ptr + 1600, stream=s2)),
                    ("update_dev on the context's stream", lambda: ctx.stream_update_dev(d_in.ptr + 1600, 100, d_out.ptr + 1600)),
                    ("export", lambda: ctx.stream_export())):
    F.fake_reset()
    ctx.stream_begin(iv)
    ctx.stream_aad(bytes(32))
    ctx.stream_update_dev(d_in.ptr, 1600, d_out.ptr, stream=s1)
    F.fake_watch(s1)
    after()
    assert name != "export" or F.fake_device_syncs() == 0, "export synchronised the device"
    check("a session's %s behind a chunk on a caller's stream" % name)
    if name != "final":
        ctx.stream_final()
# ... and an import into another context goes on where the export was taken
other = lib.Context(key)
ctx.stream_begin(iv)
ctx.stream_update_dev(d_in.ptr, 5 * MB, d_out.ptr, stream=s1)
blob = ctx.stream_export()
other.stream_import(blob)
F.fake_reset()
F.fake_watch(s1)
other.stream_update_dev(d_in.ptr + 5 * MB, 100, d_out.ptr + 5 * MB, stream=s2)
other.stream_final()
check("import after export")
ctx.stream_final()
F.fake_reset()

# ---- a routed packet call whose k-th launch fails
n = 3000
lens = [(i * 977) % 20000 for i in range(n)]
off = [0]
for x in lens:
    off.append(off[-1] + x)
d_big_in, d_big_out = lib.DeviceBuffer(off[-1] + 16), lib.DeviceBuffer(off[-1] + 16)
d_ivs, d_tags, d_auth = lib.DeviceBuffer(12 * n), lib.DeviceBuffer(16 * n), lib.DeviceBuffer(4 * n)
d_off = lib.DeviceBuffer(8 * (n + 1))
d_off.upload(struct.pack("<%dQ" % (n + 1), *off))
for caller in (None, s1):
    st = caller if caller is not None else ctx.stream()
    call = lambda: ctx.packets_crypt_dev(True, n, d_ivs.ptr, d_big_in.ptr, d_big_out.ptr, d_tags.ptr, d_data_off=d_off.ptr, d_expect_tags=d_tags.ptr,
                                         d_auth=d_auth.ptr, stream=caller)
    F.fake_reset()
    call()
    launches = F.fake_launches()
    assert launches >= 4, launches                                   # the sort, the plan, the packet kernels, the rows, the closing
    check("routed call")
    for k in range(1, launches + 2):
        F.fake_reset()
        F.fake_fail_launch(k)
        try:
            call()
        except lib.AesGcmError:
            assert k <= launches, k
            assert F.fake_ordered_behind_all(st), "launch %d of %d failed: the caller's stream returns unjoined" % (k, launches)
        else:
            assert k > launches, "launch %d of %d failed and the call returned OK" % (k, launches)
        check("routed call, launch %d of %d failing" % (k, launches))
        call()                                                       # the next call, nothing injected
        assert F.fake_ordered_behind_all(st)
        check("the call after launch %d failed" % k)

# ---- fixed-size records whose launch fails: the dispenser's base (cb in the log, left out while 0) is moved back
def logged(call):
    F.fake_reset()
    call()
    b = ctypes.create_string_buffer(1 << 12)
    assert F.fake_log(b, len(b)) <= len(b)
    return b.value.decode()


for kernel, n_pkts, pkt_len in (("k_pktl", 65536, 256), ("k_pktg", 4096, 1024)):
    fixed = lambda c: c.packets_crypt_dev(False, n_pkts, d_ivs.ptr, d_big_in.ptr, d_big_out.ptr, d_tags.ptr, pkt_len=pkt_len)
    fresh = lib.Context(key)
    want = [logged(lambda: fixed(fresh)) for _ in range(3)]          # what a context's first, second and third such call launch
    launches = F.fake_launches()
    assert launches == 1 and all(w.startswith(kernel + " ") for w in want) and " cb=" not in want[0] and " cb=" in want[1] and want[1] != want[2], want
    for k in range(1, launches + 2):
        c = lib.Context(key)
        assert logged(lambda: fixed(c)) == want[0]
        F.fake_reset()
        F.fake_fail_launch(k)
        if k <= launches:
            refused(lambda: fixed(c), lib.EHIP)
        else:
            fixed(c)
        check("%s call, launch %d of %d failing" % (kernel, k, launches))
        got = logged(lambda: fixed(c))                               # the next call: the context's second if the one between launched nothing
        assert got == want[1 if k <= launches else 2], "%s, launch %d of %d failed: the next call starts from another counter_base\n%swanted\n%s" % (kernel, k, launches, got, want[1])
F.fake_reset()

# ---- a multi-launch stream_update_dev whose k-th launch fails
for length in (5 * MB + 16 * 7 + 3, 32 * MB + 5):
    ctx.stream_begin(iv)
    ctx.stream_aad(bytes(13))
    F.fake_reset()
    ctx.stream_update_dev(d_in.ptr, length, d_out.ptr, stream=s1)
    launches = F.fake_launches()
    assert launches >= 2, launches
    ctx.stream_final()
    for k in range(1, launches + 1):
        ctx.stream_begin(iv)
        ctx.stream_aad(bytes(13))
        F.fake_reset()
        F.fake_fail_launch(k)
        refused(lambda: ctx.stream_update_dev(d_in.ptr, length, d_out.ptr, stream=s1), lib.EHIP)
        for step in (lambda: ctx.stream_update(bytes(16)), lambda: ctx.stream_update_dev(d_in.ptr, 16, d_out.ptr), lambda: ctx.stream_aad(bytes(3)),
                     lambda: ctx.stream_export(), lambda: ctx.stream_final()):
            refused(step, lib.ESTATE)
        check("stream_update_dev of %d bytes, launch %d of %d failing" % (length, k, launches))
    ctx.stream_begin(iv)                                             # begun again: a whole session, clean
    ctx.stream_update_dev(d_in.ptr, length, d_out.ptr, stream=s1)
    ctx.stream_final()
    check("a session after the failures")
print("FAKE ORDER OK")
