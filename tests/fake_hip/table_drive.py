"""Drives the two device tables -- a key table (16 slots, AES-256) and receive windows (16 windows of 64 bits, 16 of 4096) -- through the fake HIP runtime
(fakehip.cpp) for what their host sides share: create, the staging buffer that every host-to-table setter goes through, status, the range check, destroy.
Every expected answer below is a literal recorded from the commit before the two host sides were folded onto one base (DevTable, csrc/aesgcm_internal.h): this
driver passed there unchanged.  Per table and setter, on a table of its own:
  * create, then status() == (OK, 0);
  * three sets on three streams nobody has used before: A sets 2 entries, B 9 (the stage grows: hipFree + hipMalloc), C 1 (no growth).  B's set is ordered behind
    A's, C's behind B's (the vector clocks of the fake: fake_ordered_behind), neither was before, and the table holds three allocations throughout;
  * receive windows: get returns exactly what was set -- the fake copies for real, so this goes through the stage and both conversions (normalised form <-> ring) --
    with seen values that have bit 0, the top bit and bits on both sides of a word boundary set; a seen bit for a number below 0 is EARG and changes nothing;
  * the range check of every entry point that has one, at first == n_total, first + n == n_total + 1, and n == 0 at first == n_total;
  * destroy: the fake's live allocations are back where they were before create, after 2 device synchronisations (key table: around the wipe) or 1 (receive windows);
  * a KeyTable.set whose launch fails (fake_fail_launch) is EHIP, and the next set on another stream succeeds; it is NOT ordered behind the failed one's copy and
    zeroing (the failed call returns before it records the stage's event) -- recorded as it is, not as it should be.
No device discipline violation anywhere.  Without AESGCM_LIB it runs itself on libaesgcm_fake.so.

    make -C tests/fake_hip -s libaesgcm_fake.so && python tests/fake_hip/table_drive.py"""
import ctypes
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
if not os.environ.get("AESGCM_LIB"):
    subprocess.run([sys.executable, os.path.abspath(__file__)], env=dict(os.environ, AESGCM_LIB=os.path.join(HERE, "libaesgcm_fake.so")), check=True)
    sys.exit(0)

sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import aesgcm_amd  # noqa: E402,F401
from aesgcm_amd import lib  # noqa: E402

lib.load()
F = ctypes.CDLL(os.environ["AESGCM_LIB"])
F.fake_name_stream.argtypes = [ctypes.c_void_p, ctypes.c_char_p]
F.fake_ordered_behind.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
F.fake_live_allocations.restype = ctypes.c_size_t
F.fake_device_syncs.restype = ctypes.c_long
F.fake_fail_launch.argtypes = [ctypes.c_long]
OK, EARG, EHIP = lib.OK, lib.EARG, lib.EHIP
N = 16                                                                  # slots, windows

# every stream of the run, made before the first table: a context's allocations would otherwise stand between a table's create and its destroy
_ctxs = [lib.Context(bytes(32)) for _ in range(32)]
_streams = [c.stream() for c in _ctxs]
assert len(set(_streams)) == len(_streams)


def fresh(*names):
    """streams nobody has used yet, named in the fake's log"""
    out = [_streams.pop() for _ in names]
    for s, name in zip(out, names):
        F.fake_name_stream(s, name.encode())
    return out


def violations():
    b = ctypes.create_string_buffer(1 << 16)
    return b.value.decode().splitlines() if F.fake_violations(b, len(b)) else []


def rc(call):
    """the code a call of the binding ends with"""
    try:
        call()
    except lib.AesGcmError as e:
        return e.code
    return OK


def three_sets(what, table, setter):
    """setter(first, n, stream) on A (2 entries), B (9: the stage grows) and C (1)"""
    F.fake_reset()
    live = F.fake_live_allocations()
    a, b, c = fresh("A", "B", "C")
    setter(0, 2, a)
    assert F.fake_live_allocations() == live + 1, (what, "the stage is one allocation")
    assert not F.fake_ordered_behind(b, a), (what, "B is behind A before it has set anything")
    setter(2, 9, b)
    assert F.fake_ordered_behind(b, a), "%s: the set on B is not ordered behind A's, whose copy may still read the stage" % what
    assert not F.fake_ordered_behind(c, b), (what, "C is behind B before it has set anything")
    setter(11, 1, c)
    assert F.fake_ordered_behind(c, b), "%s: the set on C is not ordered behind B's" % what
    assert F.fake_live_allocations() == live + 1, (what, "a stage that grows is freed first")
    assert table.status() == (OK, 0), what
    assert violations() == [], (what, violations())


def range_check(what, total, call, ok=lambda: None):
    """call(first, n) at the three edges; the literals are the parent commit's answers"""
    assert rc(lambda: call(total, 1)) == EARG, (what, "first == n_total")
    assert rc(lambda: call(total - 1, 2)) == EARG, (what, "first + n == n_total + 1")
    assert rc(lambda: call(0, total + 1)) == EARG, (what, "n == n_total + 1")
    assert rc(lambda: call(total, 0)) == OK, (what, "n == 0 at first == n_total")
    assert rc(lambda: call(total - 1, 1)) == OK and rc(lambda: call(0, total)) == OK, (what, "the last entry, and all of them")
    assert violations() == [], (what, violations())


def destroyed(what, table, live_before, syncs_want):
    syncs = F.fake_device_syncs()
    table.close()
    assert F.fake_device_syncs() - syncs == syncs_want, (what, "destroy synchronised the device %d times" % (F.fake_device_syncs() - syncs))
    assert F.fake_live_allocations() == live_before, (what, "destroy leaves", F.fake_live_allocations() - live_before, "allocations")
    assert violations() == [], (what, violations())


# ---------------------------------------------------------------- the key table: every host-to-slot setter, on a table of its own
KEY_LEN = 32
KT_SETTERS = {
    "set": lambda kt: lambda first, n, st=None: kt.set(first, bytes(range(first, first + n)) * KEY_LEN, stream=st),
    "set_salt": lambda kt: lambda first, n, st=None: kt.set_salt(first, bytes(8 * n), stream=st),
    "set_xpn": lambda kt: lambda first, n, st=None: kt.set_xpn(first, bytes(12 * n), bytes(4 * n), stream=st),
    "set_tls_iv": lambda kt: lambda first, n, st=None: kt.set_tls_iv(first, bytes(12 * n), stream=st),
}
for name, bind in KT_SETTERS.items():
    what = "KeyTable." + name
    live = F.fake_live_allocations()
    kt = lib.KeyTable(KEY_LEN, N)
    assert F.fake_live_allocations() == live + 2 and kt.status() == (OK, 0), what      # the slots and the status word
    three_sets(what, kt, bind(kt))
    range_check(what, N, bind(kt))
    if name == "set":
        range_check("KeyTable.clear", N, lambda first, n: kt.clear(first, n))
        # a set whose launch fails, and the one after it
        d, e = fresh("D", "E")
        F.fake_reset()
        F.fake_fail_launch(1)
        assert rc(lambda: kt.set(0, bytes(KEY_LEN), stream=d)) == EHIP, what
        assert rc(lambda: kt.set(1, bytes(KEY_LEN), stream=e)) == OK, what
        assert F.fake_ordered_behind(e, d) == 0, (what, "the set after a failed one: the parent commit does not order it behind the failed call's copy and zeroing")
        assert kt.status() == (OK, 0) and violations() == [], (what, violations())
    destroyed(what, kt, live, 2)

# ---------------------------------------------------------------- receive windows: set and get at both window sizes
for W in (64, 4096):
    what = "RxWindows(window=%d)" % W
    live = F.fake_live_allocations()
    rw = lib.RxWindows(N, W)
    assert F.fake_live_allocations() == live + 2 and rw.status() == (OK, 0), what       # the records and the status word
    top = 1 << (W - 1)
    edge = (1 << 63) | (1 << 64) if W > 64 else (1 << 31) | (1 << 32)                   # both sides of a word boundary (64 bits: of the ring's wrap at next = W + 40)
    seens = [1, top, top | 1, edge, top | edge | 1, (1 << W) - 1, 0b101, 0, 1 << 7, top >> 1, 3]      # windows 0 .. 10
    nexts = [W + 40 + 3 * k for k in range(len(seens))]
    nexts[6] = 3                                                                        # 0b101: numbers 2 and 0, nothing below 0
    want_next = nexts + [77] + [0] * (N - 12)
    want_seen = seens + [0] * (N - 11)

    def rx_set(first, n, st=None):
        rw.set(first, want_next[first:first + n], want_seen[first:first + n] if first + n <= 11 else None, stream=st)
    three_sets(what, rw, rx_set)
    assert rw.get() == (want_next, want_seen), (what, rw.get())
    assert rw.get(2, 9, stream=fresh("G")[0]) == (want_next[2:11], want_seen[2:11]), what
    # a seen bit for a number below 0: EARG, and nothing changes
    assert rc(lambda: rw.set(12, [3], [1 << 3])) == EARG and rc(lambda: rw.set(0, [W + 1, W - 1], [top, top])) == EARG, what
    assert rw.get() == (want_next, want_seen), (what, "a refused set changed the table")
    range_check(what + ".set", N, lambda first, n: rw.set(first, [5] * n, [1] * n))
    range_check(what + ".get", N, lambda first, n: rw.get(first, n))
    assert rw.get() == ([5] * N, [1] * N) and rw.status() == (OK, 0), what
    destroyed(what, rw, live, 1)

assert violations() == []
print("FAKE TABLE OK")
