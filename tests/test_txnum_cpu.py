"""CPU: send counters (aesgcm_txnum_*: packet numbers handed out on the device, in packet order) without a GPU.  The binding and the header name the entry points
and the ABI version is still 5; the TxFormat constructors give the documented tuples; aesgcm_txnum_fmt_check refuses what it must; every call refuses its argument
errors before it looks at a table or a device; the lane code of csrc/aesgcm_txnum.h, run by the CPU harness tests/txnum_emul over a host stable sort with its lanes
in shuffled orders, is held to the harness's own sequential reference AND to tests/txnum_ref.py, and the same harness built with AddressSanitizer and
UndefinedBehaviorSanitizer runs the same scripts clean; the gfx950 assembly of the kernels (`make -C csrc asm_txnum`) holds exactly the five kernels, none with
scratch."""
import ctypes
import os
import random
import subprocess

import pytest

import aesgcm_amd  # noqa: F401
from aesgcm_amd import lib

from kt_common import asm_census, assert_in_budget

import txnum_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "aes-gcm-128-192-256-bits_amd", "csrc")
NAMES = ("create", "set", "get", "fmt_check", "assign_dev", "status", "destroy")
fields = lambda f: (f.num_off, f.num_len, f.dup_off, f.flags)


def presets():
    F = lib.TxFormat
    return {"macsec": F.macsec(), "macsec_xpn": F.macsec_xpn(), "esp": F.esp(), "esp_esn": F.esp_esn(), "tls12": F.tls12(), "dtls12": F.dtls12(), "srtcp": F.srtcp(),
            "srtcp_mki4": F.srtcp(4), "number_only": F.number_only()}


# ---------------------------------------------------------------- binding and header
def test_txnum_symbols_in_binding_and_header():
    hdr = open(os.path.join(ROOT, "include", "aesgcm.h")).read()
    for n in NAMES:
        assert "aesgcm_txnum_" + n in lib.SYMBOLS
        assert "AESGCM_API int aesgcm_txnum_%s(" % n in hdr
    assert "#define AESGCM_ABI_VERSION 5 " in hdr and "aesgcm_txnum_*" in hdr[hdr.index("#define AESGCM_ABI_VERSION 5 "):hdr.index("5 (round 6)")]
    for k, v in (("FROM_END", 1), ("KEEP_TOP", 2), ("WHOLE   ", 4)):
        assert "#define AESGCM_TXNUM_%s %du" % (k, v) in hdr
    assert (lib.TXNUM_FROM_END, lib.TXNUM_KEEP_TOP, lib.TXNUM_WHOLE) == (1, 2, 4) == (R.FROM_END, R.KEEP_TOP, R.WHOLE)
    section = hdr[hdr.index("SEND COUNTERS: packet numbers"):hdr.index("} aesgcm_txnum_fmt;")]
    for word in ("ASCENDING ARRAY INDEX", "BURNT", "capture-safe", "MUST NOT RUN CONCURRENTLY", "rollover counter (the caller's)", "fail-closed", "d_slots[p] = 0xFFFFFFFF",
                 "n_pkts > max_pkts"):
        assert word in section, word
    capture = hdr[hdr.index(" * CAPTURE (key tables"):hdr.index("tests/test_gpu_capture.py replays")]
    assert "aesgcm_txnum_assign_dev" in capture and "the counter table's scratch" in capture and "aesgcm_txnum_create, _set, _get, _status, _destroy" in capture
    # the encrypt calls' OUT OF SCOPE lines point here
    assert hdr.count("not this call's: aesgcm_txnum_assign_dev") == 2 and hdr.count("neither is this call's: aesgcm_txnum_assign_dev") == 1
    L = lib._txnum_typed(lib.load())
    assert L.aesgcm_abi_version() == 5
    assert [len(getattr(L, "aesgcm_txnum_" + n).argtypes) for n in NAMES] == [4, 6, 6, 1, 10, 3, 1]
    for m in ("set", "get", "status", "assign_dev", "assign", "close", "__enter__", "__exit__"):
        assert callable(getattr(lib.TxCounters, m)), m
    assert issubclass(lib.TxCounters, lib._Table) and issubclass(lib.TxFormat, lib._Format)
    assert ctypes.sizeof(lib.TxFormat) == 16
    for doc, words in (("INTEGRATION.md", ("## Send counters", "assign", "limit", "d_slots")), ("DESIGN.md", ("Send counters", "k_tx_scatter", "test_gpu_txnum.py", "test_txnum_cpu.py")),
                       ("README.md", ("Send counters", "TxCounters")), (os.path.join("tests", "COVERAGE_txnum.md"), ("Send counters", "test_gpu_txnum.py", "txnum_emul"))):
        text = open(os.path.join(ROOT, doc)).read()
        for w in words:
            assert w in text, (doc, w)


def test_format_constructors_give_the_documented_tuples():
    got = {k: fields(f) for k, f in presets().items()}
    assert got == {"macsec": (16, 4, 0, 4), "macsec_xpn": (16, 4, 0, 0), "esp": (4, 4, 0, 4), "esp_esn": (4, 4, 0, 0), "tls12": (5, 8, 0, 4), "dtls12": (5, 6, 15, 4),
                   "srtcp": (4, 4, 0, 7), "srtcp_mki4": (8, 4, 0, 7), "number_only": (0, 0, 0, 0)} == R.FORMATS
    assert fields(lib.TxFormat.srtcp(mki_len=128)) == (132, 4, 0, 7)
    assert repr(lib.TxFormat.dtls12()) == "TxFormat(num_off=5, num_len=6, dup_off=15, flags=4)"


def test_format_check():
    F = lib.TxFormat
    for f in list(presets().values()) + [F.srtcp(128), F(0, 2, 0, 0), F(65535, 8, 65527, 7), F(0, 8, 8, 0), F(9, 8, 1, 0), F(4, 2, 6, 2)]:
        assert f.check() == lib.OK, f
    assert lib._txnum_typed(lib.load()).aesgcm_txnum_fmt_check(None) == lib.EARG
    for fl in (8, 16, 15, 0x80000000, 0xFFFFFFFF):
        assert F(4, 4, 0, fl).check() == lib.EARG, fl                        # an unknown flag
    for n in (1, 3, 5, 7, 9, 10, 16, 2 ** 32 - 4):
        assert F(4, n, 0, 0).check() == lib.EARG, n
    for off in (65536, 2 ** 31, 2 ** 32 - 1):
        assert F(off, 4, 0, 0).check() == lib.EARG, off
        assert F(4, 4, off, 0).check() == lib.EARG, off
        assert F(off, 0, 0, 0).check() == lib.EARG, off
    for num_off, n, dup in ((5, 6, 5), (5, 6, 6), (5, 6, 10), (5, 6, 1), (5, 6, 4), (16, 4, 13), (16, 4, 19), (8, 8, 1), (8, 8, 15), (8, 2, 9), (8, 2, 7)):
        for fl in (0, 1):
            assert F(num_off, n, dup, fl).check() == lib.EARG, (num_off, n, dup)   # the duplicate overlaps the field
    for num_off, n, dup in ((5, 6, 11), (16, 4, 12), (16, 4, 20), (8, 8, 16), (8, 2, 10), (8, 2, 6)):
        assert F(num_off, n, dup, 0).check() == lib.OK, (num_off, n, dup)          # ... and touches it
    for fl, dup in ((2, 0), (4, 0), (6, 0), (0, 15), (0, 1), (1, 7)):
        assert F(0, 0, dup, fl).check() == lib.EARG, (fl, dup)               # KEEP_TOP, WHOLE or a duplicate of nothing
    assert F(0, 0, 0, 1).check() == lib.OK and F(77, 0, 0, 0).check() == lib.OK


def test_argument_errors_before_any_table_or_device():
    """t = NULL and placeholder pointers that are never followed: every call returns before it touches a table or a device"""
    L = lib._txnum_typed(lib.load())
    P = 16                                                                   # a placeholder pointer
    esn, only = lib.TxFormat.esp_esn(), lib.TxFormat.number_only()

    def asg(fmt=esn, t=None, n=1, ctr=P, pkts=P, off=P, num=P, hi=P, slots=P):
        return L.aesgcm_txnum_assign_dev(t, ctypes.byref(fmt) if fmt is not None else None, n, ctr, pkts, off, num, hi, slots, None)

    assert asg(fmt=None, t=P) == lib.EARG                                    # the format first
    assert asg(fmt=lib.TxFormat(4, 3, 0, 0), t=P, n=0) == lib.EARG
    assert asg(fmt=lib.TxFormat(5, 6, 6, 0), t=P, n=0) == lib.EARG
    for fmt in (esn, only):
        assert asg(fmt) == lib.EARG                                          # t NULL
        assert asg(fmt, n=0) == lib.EARG                                     # ... whatever else
        assert asg(fmt, t=P, n=0) == lib.OK                                  # nothing to do: nothing is looked at
        assert asg(fmt, t=P, n=0, ctr=None, num=None, pkts=None, off=None, hi=None, slots=None) == lib.OK
        assert asg(fmt, t=P, ctr=None) == lib.EARG
        assert asg(fmt, t=P, num=None) == lib.EARG
        assert asg(fmt, t=P, n=2 ** 31) == lib.EARG                          # above every max_pkts; a table's own max_pkts: tests/test_gpu_txnum.py
        assert asg(fmt, t=P, n=2 ** 31 + 5, hi=None, slots=None) == lib.EARG
    assert asg(esn, t=P, pkts=None) == lib.EARG and asg(esn, t=P, off=None) == lib.EARG
    # a format that writes nothing reads no packet: with d_pkts and d_pkt_off NULL the next refusal is n_pkts
    assert asg(only, t=P, n=2 ** 31, pkts=None, off=None) == lib.EARG
    out = ctypes.c_void_p(5)
    assert L.aesgcm_txnum_create(None, 0, 1, 1) == lib.EARG
    for n_ctrs, max_pkts in ((0, 1), (2 ** 31, 1), (2 ** 40, 1), (1, 0), (1, 2 ** 31), (1, 2 ** 40), (0, 0)):
        assert L.aesgcm_txnum_create(ctypes.byref(out), 0, n_ctrs, max_pkts) == lib.EARG, (n_ctrs, max_pkts)
        assert out.value is None
    one = (ctypes.c_uint64 * 1)(0)
    assert L.aesgcm_txnum_set(None, 0, 1, one, one, None) == lib.EARG and L.aesgcm_txnum_set(None, 0, 0, one, one, None) == lib.EARG
    assert L.aesgcm_txnum_get(None, 0, 1, one, one, None) == lib.EARG
    code = ctypes.c_int(7)
    assert L.aesgcm_txnum_status(None, ctypes.byref(code), None) == lib.EARG
    assert L.aesgcm_txnum_destroy(None) == lib.OK


# ---------------------------------------------------------------- the lane code on the CPU
@pytest.fixture(scope="module", params=["emul", "emul_asan"])
def emul(request):
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    d = os.path.join(ROOT, "tests", "txnum_emul")
    subprocess.run(["make", "-C", d, "-s", request.param], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)

    def run(script):
        out = subprocess.run([os.path.join(d, request.param)], input="\n".join(script) + "\n", stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
        assert out.returncode == 0 and "MISMATCH" not in out.stdout and "runtime error" not in out.stdout and "Sanitizer" not in out.stdout, out.stdout[-3000:]
        return [ln.split() for ln in out.stdout.splitlines()]
    return run


def _call(script, want, fmt, counters, ctrs, pkts, seed, offs=None, state=True):
    """append an assign call to the script and what tests/txnum_ref.py makes of it to `want`; state: and the counters afterwards (`counters` names all of them)"""
    if offs is None:
        offs = [0]
        for p in pkts:
            offs.append(offs[-1] + len(p))
    data = b"".join(pkts)
    script += ["D " + (data.hex() or "-"), "A %d %d %d %d %d %d" % (tuple(fmt) + (len(ctrs), seed)), "O " + " ".join(map(str, offs)), "C " + " ".join(map(str, ctrs))] + (["G"] if state else [])
    nums, his, refused, out, bad = R.assign(fmt, counters, ctrs, data, offs)
    want += [["a", str(n), str(h), str(0xFFFFFFFF if r else 7)] for n, h, r in zip(nums, his, refused)]
    want += [["d", (out + b"\xa5" * 16).hex()], ["x", str(2 ** 32 - 1 if bad is None else bad)]]
    if state:
        want += [["g", str(c), str(counters[c][0]), str(counters[c][1])] for c in sorted(counters)]
    return nums, refused


def _check(emul, script, want):
    got = emul(script)
    assert got == want, [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w][:5]


def test_passes_per_counter_count(emul):
    assert emul(["B"]) == [["b", str(n), str(p)] for n, p in ((1, 1), (255, 1), (256, 2), (65535, 2), (65536, 3), (65537, 3), (2 ** 31 - 1, 4))]


@pytest.mark.parametrize("name", sorted(R.FORMATS))
def test_every_format_in_shuffled_lane_orders(emul, name):
    """random packets of 0 .. 40 bytes on 3 counters with out-of-range counters and falling offsets among them, three calls that continue one another"""
    fmt = R.FORMATS[name]
    rng = random.Random("txnum " + name)
    counters = {0: [0, 2 ** 64 - 1], 1: [2 ** 32 - 9, 2 ** 64 - 1], 2: [5, 23]}
    script, want = ["T 3"] + ["S %d %d %d" % (c, nx, lm) for c, (nx, lm) in counters.items()], []
    some_ok = some_bad = 0
    for call in range(3):
        pkts = [bytes(rng.randrange(256) for _ in range(rng.randrange(0, 41))) for _ in range(40)] + [b"\xff" * 30, b"", b"\x00" * 30]
        ctrs = [rng.randrange(3) for _ in pkts]
        ctrs[3], ctrs[17] = 3, 2 ** 32 - 1
        offs = [0]
        for p in pkts:
            offs.append(offs[-1] + len(p))
        offs[11] = offs[10] - 1 if offs[10] else offs[11]                    # falling offsets (packet 10); packet 11 then starts below where 10 ended
        nums, refused = _call(script, want, fmt, counters, ctrs, pkts, 100 * call + 7, offs)
        some_ok += refused.count(False)
        some_bad += refused.count(True)
    assert some_ok >= 20 and some_bad >= 6 and counters[2][0] == 23          # counter 2 reached its limit in the middle of a call
    _check(emul, script, want)


def test_field_at_the_first_and_last_byte_and_one_byte_short(emul):
    script, want = ["T 1", "S 0 %d %d" % (0x0102030405060708, 2 ** 64 - 1)], []
    counters = {0: [0x0102030405060708, 2 ** 64 - 1]}
    for L in (2, 4, 6, 8):
        for flags in (0, R.FROM_END):
            first, last = (L + 9, L) if flags else (0, 9)                     # num_off of a field at the first / at the last bytes of a packet of L + 9 bytes
            # (packet length, num_off, refused): the field at the packet's first byte, at its last, the packet nothing but the field; each of those one byte short; empty
            for plen, off, bad in ((L + 9, first, False), (L + 9, last, False), (L, L if flags else 0, False), (L - 1, L if flags else 0, True),
                                   (L + 8, first if flags else last, True), (0, L if flags else 0, True)):
                pkts = [b"\x11" * 3, b"\xEE" * plen, b"\x22" * 3]
                nums, refused = _call(script, want, (off, L, 0, flags), counters, [0, 0, 0], pkts, 5 * L + plen)
                assert refused == [True, bad, True] if off > 3 or L > 3 else refused[1] == bad, (L, flags, plen, off)
    # the duplicate decides too: first place inside, second one byte short -- nothing of the packet is written, the number is burnt
    before = counters[0][0]
    nums, refused = _call(script, want, (0, 2, 9, 0), counters, [0, 0], [b"\xEE" * 10, b"\xEE" * 11], 3)
    assert refused == [True, False] and nums[1] == before + 1 and counters[0][0] == before + 2
    _check(emul, script, want)


def test_keep_top_with_the_bit_set_and_clear_and_whole_at_the_field_s_end(emul):
    script, want = ["T 4"], []
    counters = {0: [2 ** 31 - 3, 2 ** 40], 1: [2 ** 32 - 3, 2 ** 40], 2: [2 ** 32 - 3, 2 ** 40], 3: [2 ** 48 - 2, 2 ** 64 - 1]}
    script += ["S %d %d %d" % (c, nx, lm) for c, (nx, lm) in counters.items()]
    E1, E0 = b"\x80\x00\x00\x00", b"\x7f\xff\xff\xff"
    # SRTCP: E set and clear; the 31-bit index ends at 2^31 - 1
    pk = [b"hdr" + (E1 if i % 2 else E0) for i in range(6)]
    nums, refused = _call(script, want, R.FORMATS["srtcp"], counters, [0] * 6, pk, 1)
    assert refused == [False] * 3 + [True] * 3 and nums[2] == 2 ** 31 - 1
    assert bytes.fromhex(want[6][1])[3:7] == b"\x7f\xff\xff\xfd" and bytes.fromhex(want[6][1])[10:14] == b"\xff\xff\xff\xfe"       # E kept clear, E kept set
    # classic MACsec: WHOLE at 2^32 - 1 and at 2^32, whatever the limit says; the numbers past the field are burnt
    pk = [b"\x00" * 24] * 5
    nums, refused = _call(script, want, R.FORMATS["macsec"], counters, [1] * 5, pk, 2)
    assert nums == [2 ** 32 - 3, 2 ** 32 - 2, 2 ** 32 - 1, R.NONE, R.NONE] and counters[1][0] == 2 ** 32 + 2
    # XPN: the same numbers pass, the field wraps, hi steps
    nums, refused = _call(script, want, R.FORMATS["macsec_xpn"], counters, [2] * 5, pk, 3)
    assert nums[-1] == 2 ** 32 + 1 and not any(refused)
    # DTLS 1.2: 48 bits, both places
    pk = [b"\x16\xfe\xfd\x00\x01" + b"\xAA" * 6 + b"\x00\x20" + b"\x00\x01" + b"\xBB" * 6 + b"payload"] * 4
    nums, refused = _call(script, want, R.FORMATS["dtls12"], counters, [3] * 4, pk, 4)
    assert refused == [False, False, True, True]
    d = bytes.fromhex(want[-6][1])
    assert d[5:11] == d[15:21] == (2 ** 48 - 2).to_bytes(6, "big") and d[11:15] == b"\x00\x20\x00\x01" and d[28 + 5:28 + 11] == b"\xff" * 6
    _check(emul, script, want)


def test_a_limit_reached_mid_segment_and_an_unset_counter(emul):
    counters = {0: [10, 14], 1: [0, 0], 2: [2 ** 64 - 3, 2 ** 64 - 1]}
    script, want = ["T 3", "S 0 10 14", "S 2 %d %d" % (2 ** 64 - 3, 2 ** 64 - 1)], []
    ctrs = [0, 1, 0, 2, 0, 0, 2, 0, 2, 0, 1, 2]
    nums, refused = _call(script, want, R.FORMATS["number_only"], counters, ctrs, [b""] * len(ctrs), 11)
    assert nums == [10, R.NONE, 11, 2 ** 64 - 3, 12, 13, 2 ** 64 - 2, R.NONE, R.NONE, R.NONE, R.NONE, R.NONE]
    assert counters == {0: [14, 14], 1: [0, 0], 2: [2 ** 64 - 1, 2 ** 64 - 1]}
    nums, refused = _call(script, want, R.FORMATS["esp"], counters, ctrs, [b"\x00" * 8] * len(ctrs), 12)      # a second call: everything refused, nothing moves
    assert all(refused)
    _check(emul, script, want)


@pytest.mark.parametrize("n_ctrs,n", [(1, 300), (3, 300), (300, 300), (70000, 500)])
def test_populations_in_shuffled_lane_orders(emul, n_ctrs, n):
    """all on one counter, a few interleaved, about one each, and counters whose numbers differ only in a high digit; out-of-range counters sprinkled in.  A counter
    that is never set refuses everything, in the harness as in the reference (which does not know it)"""
    rng = random.Random(n_ctrs * 1000 + n)
    used = list(range(n_ctrs)) if n_ctrs <= 300 else rng.sample(range(n_ctrs), 40) + [255, 256, 65535, 65536, 69999]
    counters = {c: [rng.randrange(2 ** 40), 2 ** 41] for c in used if c % 7 != 3}
    script, want = ["T %d" % n_ctrs] + ["S %d %d %d" % (c, nx, lm) for c, (nx, lm) in counters.items()], []
    for seed in (1, 2):
        ctrs = [rng.choice(used) for _ in range(n)]
        for k in range(0, n, 37):
            ctrs[k] = n_ctrs + k                                              # out of range
        nums, refused = _call(script, want, R.FORMATS["number_only"], counters, ctrs, [b""] * n, seed, state=False)
        assert refused.count(False) > n // 2
    _check(emul, script, want)


# ---------------------------------------------------------------- the kernels' assembly
@pytest.fixture(scope="module")
def census():
    return asm_census("txnum")


def test_txnum_kernel_set(census):
    assert {n.split("(")[0] for n in census} == {"k_tx_hist", "k_tx_scan", "k_tx_scatter", "k_tx_heads", "k_tx_assign"}, sorted(census)


def test_txnum_kernels_scratch_free_and_in_budget(census):
    assert_in_budget(census, body="k_kt")                                    # (no kernel here runs the AES block loop)
    for name, k in census.items():
        if not name.startswith("k_tx_scan"):                                 # (the scan holds its 64 entries per lane in registers on purpose: one workgroup)
            assert k["vgpr"] <= 32, (name, k["vgpr"])


def test_txnum_source_is_a_unit_of_its_own_and_has_no_atomic_but_the_status_word_s():
    others = [f for f in os.listdir(CSRC) if f.endswith("_kernels.hip") and f != "aesgcm_txnum_kernels.hip"] + ["aesgcm_kernels.hip"]
    assert len(others) >= 9
    for f in others:
        assert "k_tx_" not in open(os.path.join(CSRC, f)).read(), f
    assert '#include "aesgcm_txnum_kernels.hip"' in open(os.path.join(CSRC, "aesgcm_device.hip")).read()
    mk = open(os.path.join(CSRC, "Makefile")).read().splitlines()
    assert "txnum" in [w for ln in mk if ln.startswith("FAMILIES") for w in ln.split()] and "aesgcm_txnum" in [w for ln in mk if ln.startswith("UNITS") for w in ln.split()]
    kern = open(os.path.join(CSRC, "aesgcm_txnum_kernels.hip")).read()
    code = "\n".join(ln.split("//")[0] for ln in kern.splitlines())
    assert "atomic" not in code
    hdr = "\n".join(ln.split("//")[0] for ln in open(os.path.join(CSRC, "aesgcm_txnum.h")).read().splitlines())
    assert hdr.count("atomic") == 1 and "atomicMin(status, i)" in hdr
    note = open(os.path.join(ROOT, "profiles", "txnum", "isa_unchanged.txt")).read()
    assert "every instruction stream identical: yes" in note and "no scratch" in note
