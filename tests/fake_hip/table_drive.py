"""Drives the six device tables -- a key table (16 slots, AES-256), receive windows (16 windows of 64 bits, 16 of 4096), send counters (16, calls of 64 packets), traffic
secrets (16 of SHA-256, 16 of SHA-384), SRTP master keys (16 each of AES-128, -192, -256) and TLS 1.2 master secrets (16 of SHA-256, 16 of SHA-384) -- through the fake HIP runtime (fakehip.cpp) for what their host sides
share: create, the staged set that every host-to-table setter is, get, clear, status, the range check, destroy.  EVERYTHING below was recorded from the parent commit
of the one that folded set, get and clear onto the base (DevTable, csrc/aesgcm_internal.h: devtab_staged, devtab_put, devtab_get, devtab_clear): the literals --
allocation counts, synchronisation counts, record hashes, the ordering bits -- and tests/golden/table_calls.txt; this driver passed on that commit's five host units,
unchanged, with one difference, the last point.  Per table and setter, on a table of its own:
  * create, then the allocation count and status() == (OK, 0);
  * three sets on three streams nobody has used before: A sets 2 entries, B 9 (the stage grows: hipFree + hipMalloc), C 1 (no growth).  B's set is ordered behind
    A's, C's behind B's (the vector clocks of the fake: fake_ordered_behind), neither was before, and the table holds three allocations throughout;
  * receive windows: get returns exactly what was set -- the fake copies for real, so this goes through the stage and both conversions (normalised form <-> ring) --
    with seen values that have bit 0, the top bit and bits on both sides of a word boundary set; a seen bit for a number below 0 is EARG and changes nothing;
  * send counters: get returns exactly what was set; a set with next > limit is EARG and changes nothing;
  * secrets and master keys, which no call reads back: an install of one entry, whose line in the fake's launch log carries the FNV-1a of the 64-byte record -- for
    an entry set on A, on B, on C, and for one never set;
  * the range check of every entry point that has one (set, get, clear), at first == n_total, first + n == n_total + 1, and n == 0 at first == n_total;
  * destroy: the fake's live allocations are back where they were before create, after 2 device synchronisations (the tables that hold secrets -- key table, secrets,
    master keys: around the wipe) or 1 (the tables that hold numbers -- receive windows, send counters);
  * the runtime calls of a table's first set of 2 entries and of its next one -- names and byte counts, no addresses (fake_log_runtime, fake_calls) -- are those of
    tests/golden/table_calls.txt (--write writes the file): a fold that adds a copy, a synchronisation or an allocation to a set, or moves the zeroing, shows there;
  * a set that fails in the runtime -- KeyTable.set's launch (fake_fail_launch), the first copy of SecretTable.set and MasterKeyTable.set (fake_fail_copy) -- is EHIP,
    and the next set on another stream succeeds and IS ordered behind the failed one's copies and zeroing.  THE ONE DELIBERATE CHANGE: the parent commit returned
    from a failed set before it recorded the stage's event, so the bit was 0 there in all three cases (this driver recorded it "as it is, not as it should be");
    devtab_staged records the event on every path once the stage is there.
THE SIXTH TABLE (MasterSecretTable, csrc/aesgcm_prf12.hip) came later and its literals were recorded the same way: on the host code of the commit before the one that
made aesgcm_prf12 a unit of its own, with nothing but the fake's klaunch_prf12_* added.  Its record hashes (128-byte records: an install_dev's and an
export_srtp_dev's launch line) are also the FNV-1a of the record as include/aesgcm.h lays it out; beyond the points above it has every AESGCM_EARG of the two device
calls (no direction array, a key table or master-key table on another device, a master-key table of AES-192), none of which launches; a set that fails at its second
copy; and, since the host's set launches nothing, the failed launch of set_dev.
No device discipline violation anywhere.  Without AESGCM_LIB it runs itself on libaesgcm_fake.so.

    make -C tests/fake_hip -s libaesgcm_fake.so && python tests/fake_hip/table_drive.py"""
import ctypes
import os
import struct
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
if not os.environ.get("AESGCM_LIB"):
    subprocess.run([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=dict(os.environ, AESGCM_LIB=os.path.join(HERE, "libaesgcm_fake.so")), check=True)
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
F.fake_fail_launch.argtypes = F.fake_fail_copy.argtypes = [ctypes.c_long]
F.fake_log.restype = F.fake_calls.restype = ctypes.c_size_t
F.fake_log.argtypes = F.fake_calls.argtypes = [ctypes.c_char_p, ctypes.c_size_t]
OK, EARG, EHIP = lib.OK, lib.EARG, lib.EHIP
N = 16                                                                  # slots, windows, counters, secrets, masters

# every stream of the run, made before the first table: a context's allocations would otherwise stand between a table's create and its destroy
_ctxs = [lib.Context(bytes(32)) for _ in range(80)]
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


def text(read):
    b = ctypes.create_string_buffer(1 << 16)
    assert read(b, len(b)) <= len(b)
    return b.value.decode().splitlines()


CALLS = []                                                              # what becomes tests/golden/table_calls.txt


def record_calls(what, table, setter):
    """the runtime calls of setter(0, 2, A) on a table of its own that nobody has set yet (the stage is allocated, its event made), then of setter(2, 2, A)"""
    a, = fresh("A")
    for title, first in (("the first set", 0), ("the next set", 2)):
        F.fake_reset()
        F.fake_log_runtime(1)
        setter(first, 2, a)
        F.fake_log_runtime(0)
        CALLS.extend(["== %s, %s of 2 entries" % (what, title)] + text(F.fake_calls))
    table.close()


def failed_set(what, table, setter, arm, behind):
    """a set on D that fails in the runtime (arm(1): its first launch, or its first copy), and the set on E after it"""
    d, e = fresh("D", "E")
    F.fake_reset()
    arm(1)
    assert rc(lambda: setter(0, 1, d)) == EHIP, what
    assert rc(lambda: setter(1, 1, e)) == OK, what
    assert F.fake_ordered_behind(e, d) == behind, (what, "the set after a failed one, against the failed call's copy and zeroing", F.fake_ordered_behind(e, d))
    assert table.status() == (OK, 0) and violations() == [], (what, violations())


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
    other = lib.KeyTable(KEY_LEN, N)
    record_calls(what, other, bind(other))
    kt = lib.KeyTable(KEY_LEN, N)
    assert F.fake_live_allocations() == live + 2 and kt.status() == (OK, 0), what      # the slots and the status word
    three_sets(what, kt, bind(kt))
    range_check(what, N, bind(kt))
    if name == "set":
        range_check("KeyTable.clear", N, lambda first, n: kt.clear(first, n))
        failed_set(what, kt, bind(kt), F.fake_fail_launch, 1)
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

    def rx_set(first, n, st=None, rw=rw):
        rw.set(first, want_next[first:first + n], want_seen[first:first + n] if first + n <= 11 else None, stream=st)
    three_sets(what, rw, rx_set)
    other = lib.RxWindows(N, W)
    record_calls(what, other, lambda first, n, st: rx_set(first, n, st, other))
    assert rw.get() == (want_next, want_seen), (what, rw.get())
    assert rw.get(2, 9, stream=fresh("G")[0]) == (want_next[2:11], want_seen[2:11]), what
    # a seen bit for a number below 0: EARG, and nothing changes
    assert rc(lambda: rw.set(12, [3], [1 << 3])) == EARG and rc(lambda: rw.set(0, [W + 1, W - 1], [top, top])) == EARG, what
    assert rw.get() == (want_next, want_seen), (what, "a refused set changed the table")
    range_check(what + ".set", N, lambda first, n: rw.set(first, [5] * n, [1] * n))
    range_check(what + ".get", N, lambda first, n: rw.get(first, n))
    assert rw.get() == ([5] * N, [1] * N) and rw.status() == (OK, 0), what
    destroyed(what, rw, live, 1)

# ---------------------------------------------------------------- send counters: set and get
what = "TxCounters"
live = F.fake_live_allocations()
tx = lib.TxCounters(N, 64)
assert F.fake_live_allocations() == live + 2 and tx.status() == (OK, 0), what           # the records with the assign call's scratch, and the status word
want_next = [1000 + 3 * k for k in range(12)] + [0] * (N - 12)
want_limit = [(1 << 32) + k for k in range(11)] + [1 << 63] + [0] * (N - 12)


def tx_set(first, n, st=None, tx=tx):
    tx.set(first, want_next[first:first + n], want_limit[first:first + n], stream=st)


three_sets(what, tx, tx_set)
other = lib.TxCounters(N, 64)
record_calls(what, other, lambda first, n, st: tx_set(first, n, st, other))
assert tx.get() == (want_next, want_limit), (what, tx.get())
assert tx.get(2, 9, stream=fresh("G")[0]) == (want_next[2:11], want_limit[2:11]), what
# next > limit: EARG, and nothing changes
assert rc(lambda: tx.set(12, [8], [7])) == EARG and rc(lambda: tx.set(0, [1, 9], [1, 8])) == EARG, what
assert tx.get() == (want_next, want_limit), (what, "a refused set changed the table")
range_check(what + ".set", N, lambda first, n: tx.set(first, [5] * n, [6] * n))
range_check(what + ".get", N, lambda first, n: tx.get(first, n))
assert tx.get() == ([5] * N, [6] * N) and tx.status() == (OK, 0), what
destroyed(what, tx, live, 1)

# ---------------------------------------------------------------- traffic secrets and SRTP master keys: set, and what an install finds in the record
d_idx, d_slots = lib.DeviceBuffer(16), lib.DeviceBuffer(16)


def installed_record(install, i, kernel="_install "):
    """the record hash in the launch log's line of one install (or export) with idx = [i]"""
    d_idx.upload(struct.pack("<I", i))
    F.fake_reset()
    install()
    line, = [ln for ln in text(F.fake_log) if kernel in ln]
    return line.split(" rec=")[1]


Z = "b9b23f3a46fd0825"                                                  # 64 zero bytes: entry 12 was never set
SECRET_RECORDS = {32: {0: "56be829029f2d03a", 10: "b07a097bf5b0c33a", 11: "40b54be85c3cd39a", 12: Z},
                  48: {0: "8024c06774b06c6a", 10: "c9a716bbe7e3c8ea", 11: "3dfbe96f02d0ac5a", 12: Z}}
for hl in (32, 48):
    what = "SecretTable(hash_len=%d)" % hl
    live = F.fake_live_allocations()
    sec = lib.SecretTable(hl, N)
    assert F.fake_live_allocations() == live + 2 and sec.status() == (OK, 0), what      # the records and the status word

    def sec_set(first, n, st=None, sec=sec):
        sec.set(first, b"".join(bytes([k + 1]) * hl for k in range(first, first + n)), stream=st)
    three_sets(what, sec, sec_set)
    other = lib.SecretTable(hl, N)
    record_calls(what, other, lambda first, n, st: sec_set(first, n, st, other))
    with lib.KeyTable(16, N) as kt:
        got = {i: installed_record(lambda: sec.install_dev(lib.KdfFormat.tls13(), kt, 1, d_idx.ptr, d_slots.ptr), i) for i in SECRET_RECORDS[hl]}
    assert got == SECRET_RECORDS[hl], (what, got)
    failed_set(what, sec, sec_set, F.fake_fail_copy, 1)
    range_check(what + ".set", N, sec_set)
    range_check(what + ".clear", N, lambda first, n: sec.clear(first, n))
    destroyed(what, sec, live, 2)

MASTER_RECORDS = {16: {0: "9a7a33434585ea30", 10: "a422a21b2a771598", 11: "0fe239bc383db6c6", 12: Z},
                  24: {0: "2fb7bd1ad9ccf528", 10: "5b0e1bba16399060", 11: "9c86f8adfc60c0a6", 12: Z},
                  32: {0: "a22c23717ac6f3e0", 10: "e02a56c00e850188", 11: "a9e1708777441486", 12: Z}}
for kl in (16, 24, 32):
    what = "MasterKeyTable(key_len=%d)" % kl
    live = F.fake_live_allocations()
    mk = lib.MasterKeyTable(kl, N)
    assert F.fake_live_allocations() == live + 2 and mk.status() == (OK, 0), what       # the records and the status word

    def mk_set(first, n, st=None, mk=mk):
        mk.set(first, b"".join(bytes([k + 1]) * kl for k in range(first, first + n)), b"".join(bytes([0x80 + k]) * 14 for k in range(first, first + n)), stream=st)
    three_sets(what, mk, mk_set)
    other = lib.MasterKeyTable(kl, N)
    record_calls(what, other, lambda first, n, st: mk_set(first, n, st, other))
    with lib.KeyTable(kl, N) as kt:
        got = {i: installed_record(lambda: mk.install_dev(lib.SRTP_RTP, kt, 1, d_idx.ptr, d_slots.ptr), i) for i in MASTER_RECORDS[kl]}
    assert got == MASTER_RECORDS[kl], (what, got)
    failed_set(what, mk, mk_set, F.fake_fail_copy, 1)
    range_check(what + ".set", N, mk_set)
    range_check(what + ".clear", N, lambda first, n: mk.clear(first, n))
    destroyed(what, mk, live, 2)

# ---------------------------------------------------------------- TLS 1.2 master secrets: set, and what an install and an export find in the record
Z128 = "8421ae126c7ced25"                                                            # 128 zero bytes: entry 12 was never set
lib.KeyTable(16, 1, device=1).close()                                   # (device 1's own state is made on first use: not an allocation of the tables below)
PRF12_RECORDS = {0: "4266d1521611c19d", 10: "dfca7ff05712211d", 11: "5a4dd056cd27682d", 12: Z128}            # a record is the 48-byte master and the two randoms, whatever the hash
for hl in (32, 48):
    what = "MasterSecretTable(hash_len=%d)" % hl
    live = F.fake_live_allocations()
    ms = lib.MasterSecretTable(hl, N)
    assert F.fake_live_allocations() == live + 2 and ms.status() == (OK, 0), what       # the records and the status word

    def ms_set(first, n, st=None, ms=ms):
        r = range(first, first + n)
        ms.set(first, b"".join(bytes([k + 1]) * 48 for k in r), b"".join(bytes([0x40 + k]) * 32 for k in r), b"".join(bytes([0x80 + k]) * 32 for k in r), stream=st)
    three_sets(what, ms, ms_set)
    other = lib.MasterSecretTable(hl, N)
    record_calls(what, other, lambda first, n, st: ms_set(first, n, st, other))
    with lib.KeyTable(16, N) as kt, lib.MasterKeyTable(16, N) as mk, lib.KeyTable(16, N, device=1) as kt1, lib.MasterKeyTable(16, N, device=1) as mk1, lib.MasterKeyTable(24, N) as mk24:
        got = {i: installed_record(lambda: ms.install_dev(kt, 1, d_idx.ptr, d_slots.ptr, None), i) for i in PRF12_RECORDS}
        assert got == PRF12_RECORDS, (what, "install_dev", got)
        got = {i: installed_record(lambda: ms.export_srtp_dev(mk, 1, d_idx.ptr, None, d_slots.ptr), i, "k_prf12_export ") for i in PRF12_RECORDS}
        assert got == PRF12_RECORDS, (what, "export_srtp_dev", got)
        # every AESGCM_EARG of the two device calls: no direction array, a table on another device, a master table of AES-192; none of them launches
        F.fake_reset()
        assert rc(lambda: ms.install_dev(kt, 1, d_idx.ptr, None, None)) == EARG and rc(lambda: ms.export_srtp_dev(mk, 1, d_idx.ptr, None, None)) == EARG, what
        assert rc(lambda: ms.install_dev(kt1, 1, d_idx.ptr, d_slots.ptr, d_slots.ptr)) == EARG and rc(lambda: ms.export_srtp_dev(mk1, 1, d_idx.ptr, d_slots.ptr, d_slots.ptr)) == EARG, what
        assert rc(lambda: ms.export_srtp_dev(mk24, 1, d_idx.ptr, d_slots.ptr, d_slots.ptr)) == EARG, what
        assert rc(lambda: ms.install_dev(kt, 0, None, None, None)) == OK and rc(lambda: ms.export_srtp_dev(mk, 0, None, None, None)) == OK, (what, "n == 0")
        assert text(F.fake_log) == [] and ms.status() == (OK, 0) and violations() == [], (what, text(F.fake_log), violations())
    failed_set(what, ms, ms_set, F.fake_fail_copy, 1)                                   # the copy into the stage
    failed_set(what, ms, ms_set, lambda k: F.fake_fail_copy(k + 1), 1)                  # the copy out of it
    # the host's set launches nothing; the set that does is set_dev, and its failed launch is EHIP, the first error, with the next set as ever
    F.fake_reset()
    F.fake_fail_launch(1)
    assert rc(lambda: ms.set_dev(1, d_idx.ptr, d_slots.ptr, d_slots.ptr, d_slots.ptr)) == EHIP and rc(lambda: ms_set(2, 1)) == OK and ms.status() == (OK, 0), what
    range_check(what + ".set", N, ms_set)
    range_check(what + ".clear", N, lambda first, n: ms.clear(first, n))
    destroyed(what, ms, live, 2)

assert violations() == []
golden = os.path.join(os.path.dirname(HERE), "golden", "table_calls.txt")
if "--write" in sys.argv:
    open(golden, "w").write("\n".join(CALLS) + "\n")
assert CALLS == open(golden).read().splitlines(), "the runtime calls of a set are not the recorded ones (tests/golden/table_calls.txt):\n" + "\n".join(CALLS)
print("FAKE TABLE OK")
