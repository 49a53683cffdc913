"""CPU: SRTP's on-device key derivation (aesgcm_srtp_kdf_*: master keys on the device, the AES-CM PRF of RFC 3711 4.3.1 / RFC 6188 into key-table slots) without a GPU.
The binding and the header name the entry points and the ABI version is still 5; every call refuses its argument errors before it looks at a table or a device;
tests/srtp_kdf_ref.py -- the reference tests/test_gpu_srtp_kdf.py holds the GPU to -- reproduces the three published vectors (tests/golden/srtp_kdf_rfc.json); the lane
code of csrc/aesgcm_srtp_kdf.h, run by the CPU harness tests/srtp_kdf_emul, is held to that reference: the x block, the session key and salt for all three key sizes, both
kinds, r in {0, 1, 2^16, 2^48 - 1} and without d_r, records stored by the set lane, every refusal kind and the status word; the same harness built with
AddressSanitizer and UndefinedBehaviorSanitizer runs the same scripts clean; the gfx950 assembly of the kernels (`make -C csrc asm_srtp_kdf`) holds exactly the kernels
the design names, none with scratch.  No published vector has r != 0 or the SRTCP labels: those rest on the formula."""
import ctypes
import os
import random
import subprocess

import pytest

import aesgcm_amd  # noqa: F401
from aesgcm_amd import lib

from kt_common import asm_census, assert_in_budget

import srtp_fixture as S
import srtp_kdf_ref as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "aes-gcm-128-192-256-bits_amd", "csrc")
NAMES = ("create", "set", "set_dev", "clear", "install_dev", "status", "destroy")
RS = (0, 1, 1 << 16, (1 << 48) - 1)


# ---------------------------------------------------------------- binding, header, documents
def test_srtp_kdf_symbols_in_binding_and_header():
    hdr = open(os.path.join(ROOT, "include", "aesgcm.h")).read()
    for n in NAMES:
        assert "aesgcm_srtp_kdf_" + n in lib.SYMBOLS
        assert "AESGCM_API int aesgcm_srtp_kdf_%s(" % n in hdr
    assert "#define AESGCM_ABI_VERSION 5 " in hdr and "aesgcm_srtp_kdf_*" in hdr[hdr.index("#define AESGCM_ABI_VERSION 5 "):hdr.index("5 (round 6)")]
    section = hdr[hdr.index("SRTP KEY DERIVATION: SRTP and SRTCP session keys"):hdr.index("typedef struct aesgcm_srtp_kdf aesgcm_srtp_kdf;")]
    for word in ("PROTECT IT LIKE KEYS", "RFC 3711 4.3.1", "RFC 6188", "RFC 7714 11", "14 BYTES HERE, ALWAYS", "WITH TWO ZERO BYTES APPENDED", "0x00", "0x02", "0x03", "0x05",
                 "NOTHING an entry names is written", "d_r = NULL", "2^48", "capture-safe", "NO DERIVED KEY IN MEMORY", "key table's status is not touched",
                 "key size is not the master table's", "TLS 1.2 / DTLS 1.2 PRF"):
        assert word in section, word
    capture = hdr[hdr.index(" * CAPTURE (key tables"):hdr.index("tests/test_gpu_capture.py replays")]
    assert "aesgcm_srtp_kdf_install_dev" in capture and "aesgcm_srtp_kdf_create, _set, _set_dev, _clear, _status, _destroy" in capture
    assert capture.index("NOT CAPTURE-SAFE") < capture.index("aesgcm_srtp_kdf_create, _set")
    # no document tells an SRTP caller any more that the session key derivation is out of scope
    assert "key derivation (RFC 3711 4.3 KDF" not in hdr and "SRTP's AES-CM key derivation (RFC 3711 4.3);" not in hdr
    for a, b in (("SRTP AND SRTCP PACKETS", "aesgcm_srtp_fmt;"), ("ON-DEVICE KEY DERIVATION: TLS 1.3", "} aesgcm_kdf_fmt;")):
        assert "aesgcm_srtp_kdf_*" in hdr[hdr.index(a):hdr.index(b)], a                   # ... each points at the table instead
    L = lib._srtp_kdf_typed(lib.load())
    assert L.aesgcm_abi_version() == 5
    assert [len(getattr(L, "aesgcm_srtp_kdf_" + n).argtypes) for n in NAMES] == [4, 6, 6, 4, 8, 3, 1]
    for m in ("set", "set_dev", "clear", "install_dev", "install", "status", "close", "__enter__", "__exit__"):
        assert callable(getattr(lib.MasterKeyTable, m)), m
    assert issubclass(lib.MasterKeyTable, lib._Table) and lib.MasterKeyTable._prefix == "aesgcm_srtp_kdf"


def test_documents_say_what_the_issue_asks():
    for doc, words in (("INTEGRATION.md", ("### SRTP and SRTCP session keys", "MasterKeyTable", "master key", "key_derivation_rate", "two zero bytes", "protected like keys")),
                       ("DESIGN.md", ("SRTP key derivation on the device", "k_srtp_kdf_install", "kdf_key_schedule", "test_gpu_srtp_kdf.py", "test_srtp_kdf_cpu.py")),
                       ("README.md", ("SRTP key derivation", "MasterKeyTable", "profiles/srtp_kdf/ab.txt")),
                       (os.path.join("tests", "COVERAGE_srtp_kdf.md"), ("SRTP key derivation", "test_gpu_srtp_kdf.py", "srtp_kdf_emul", "RFC 6188", "r != 0", "0x03"))):
        text = open(os.path.join(ROOT, doc)).read()
        for w in words:
            assert w in text, (doc, w)
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "The derivation is the caller's, once per session or key-derivation period." not in integ


def test_argument_errors_before_any_table_or_device():
    """k = NULL, keytab = NULL and placeholder pointers that are never followed: every call returns before it touches a table or a device"""
    L = lib._srtp_kdf_typed(lib.load())
    P = 16                                                                   # a placeholder pointer

    def inst(kind=lib.SRTP_RTP, k=None, kt=None, n=1, idx=P, slots=P, r=P):
        return L.aesgcm_srtp_kdf_install_dev(k, kind, kt, n, idx, slots, r, None)

    for kind in (0, 3, 4, 0x200, 0xFFFFFFFF):
        assert inst(kind=kind, k=P, kt=P, n=0) == lib.EARG, kind            # the kind first, whatever else
    assert inst() == lib.EARG and inst(k=P) == lib.EARG and inst(kt=P) == lib.EARG and inst(n=0) == lib.EARG      # k or keytab NULL
    for kind in (lib.SRTP_RTP, lib.SRTP_RTCP):
        assert inst(kind=kind, k=P, kt=P, n=0) == lib.OK and inst(kind=kind, k=P, kt=P, n=0, idx=None, slots=None, r=None) == lib.OK      # nothing to do: nothing is looked at
    assert inst(k=P, kt=P, idx=None) == lib.EARG and inst(k=P, kt=P, slots=None) == lib.EARG and inst(k=P, kt=P, n=2 ** 31) == lib.EARG
    out = ctypes.c_void_p(5)
    assert L.aesgcm_srtp_kdf_create(None, 0, 16, 1) == lib.EARG
    for key_len, n in ((0, 1), (12, 1), (14, 1), (20, 1), (33, 1), (48, 1), (16, 0), (32, 0), (24, 2 ** 31), (32, 2 ** 40)):
        assert L.aesgcm_srtp_kdf_create(ctypes.byref(out), 0, key_len, n) == lib.EARG, (key_len, n)
        assert out.value is None
    key, salt = bytes(32), bytes(14)
    assert L.aesgcm_srtp_kdf_set(None, 0, 1, key, salt, None) == lib.EARG and L.aesgcm_srtp_kdf_set(None, 0, 0, key, salt, None) == lib.EARG
    assert L.aesgcm_srtp_kdf_set_dev(None, 1, P, P, P, None) == lib.EARG and L.aesgcm_srtp_kdf_clear(None, 0, 1, None) == lib.EARG
    code = ctypes.c_int(7)
    assert L.aesgcm_srtp_kdf_status(None, ctypes.byref(code), None) == lib.EARG
    assert L.aesgcm_srtp_kdf_destroy(None) == lib.OK


# ---------------------------------------------------------------- the reference
def test_reference_reproduces_the_published_vectors():
    vs = K.vectors()
    assert [len(v[1]) for v in vs] == [16, 24, 32]
    for name, mk, ms, sk, ss in vs:
        assert len(ms) == 14 and len(ss) == 14 and len(sk) == len(mk)
        assert K.prf(mk, ms, 0x00, 0, len(mk)) == sk, name
        assert K.prf(mk, ms, 0x02, 0, 14) == ss, name
        assert K.session(S.RTP, mk, ms) == (sk, ss[:12]), name
        # the other labels and another r give other keys
        assert len({K.session(S.RTP, mk, ms), K.session(S.RTCP, mk, ms), K.session(S.RTP, mk, ms, 1), K.session(S.RTCP, mk, ms, 1)}) == 4
    # RFC 3711 B.3's own intermediate: the x block of the cipher key is the master salt (label 0, r 0), of the salt 0x02 in byte 7
    mk, ms = vs[0][1], vs[0][2]
    assert K.prf(mk, ms, 0, 0, 16) == K.aes_ecb(mk, ms + b"\0\0")
    assert K.prf(mk, ms, 2, 0, 16) == K.aes_ecb(mk, bytes.fromhex("0EC675AD498AFEE9B6960B3AABE60000"))
    # a 12-byte master salt enters with two zero bytes appended
    assert K.pad_salt(ms[:12]) == ms[:12] + b"\0\0" and K.session(S.RTP, mk, ms[:12]) == K.session(S.RTP, mk, ms[:12] + b"\0\0") != K.session(S.RTP, mk, b"\0\0" + ms[:12])


# ---------------------------------------------------------------- the lane code on the CPU
@pytest.fixture(scope="module", params=["emul", "emul_asan"])
def emul(request):
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    d = os.path.join(ROOT, "tests", "srtp_kdf_emul")
    subprocess.run(["make", "-C", d, "-s", request.param], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)

    def run(script):
        out = subprocess.run([os.path.join(d, request.param)], input="\n".join(script) + "\n", stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
        assert out.returncode == 0 and "runtime error" not in out.stdout and "Sanitizer" not in out.stdout and "bad script" not in out.stdout, out.stdout[-3000:]
        return [ln.split() for ln in out.stdout.splitlines()]
    return run


def _masters(seed, key_len, n):
    rng = random.Random("srtp kdf %s %d" % (seed, key_len))
    return [(bytes(rng.randrange(256) for _ in range(key_len)), bytes(rng.randrange(256) for _ in range(14))) for _ in range(n)]


def _want(kind, mk, ms, r):
    sk, ss = K.session(kind, mk, ms, r)
    return ["i", sk.hex(), ss.hex()]


def test_published_vectors_through_the_lane_code(emul):
    script, want = [], []
    for name, mk, ms, sk, ss in K.vectors():
        script += ["T %d 1" % len(mk), "M 0 0 %s %s" % (mk.hex(), ms.hex()), "I 1 1 0 0 0 -", "I 1 1 0 0 0 0", "S"]
        want += [["m", "ok"], ["i", sk.hex(), ss[:12].hex()], ["i", sk.hex(), ss[:12].hex()], ["s", "none"]]
    assert emul(script) == want


def test_x_block_equals_the_formula(emul):
    script, want = [], []
    ms_all = [bytes(14), b"\xff" * 14] + [m[1] for m in _masters("x", 16, 6)]
    script.append("T 16 %d" % len(ms_all))
    for i, ms in enumerate(ms_all):
        script.append("M %d %d %s %s" % (i, i, bytes(16).hex(), ms.hex()))
        want.append(["m", "ok"])
        for label in (0, 2, 3, 5, 0xFF):
            for r in RS + (0x0102030405 << 8 | 6,):
                script.append("B %d %d %d" % (i, label, r))
                want.append(["b", ((int.from_bytes(ms, "big") ^ (label << 48) ^ r) << 16).to_bytes(16, "big").hex()])
    assert emul(script) == want


@pytest.mark.parametrize("key_len", [16, 24, 32])
def test_session_keys_and_salts_equal_the_reference(emul, key_len):
    """both kinds, every r of the issue and the call without d_r, random masters and the edge ones, entries at lanes across the LDS replicas; a 12-byte master salt
    padded on the right"""
    ms = _masters("lane", key_len, 10) + [(bytes(key_len), bytes(14)), (b"\xff" * key_len, b"\xff" * 14)]
    ms.append((ms[0][0], K.pad_salt(ms[0][1][:12])))
    script, want = ["T %d %d" % (key_len, len(ms))], []
    for i, (mk, s) in enumerate(ms):
        script.append("M %d %d %s %s" % (3 * i, i, mk.hex(), s.hex()))
        want.append(["m", "ok"])
    for i, (mk, s) in enumerate(ms):
        for kind in (S.RTP, S.RTCP):
            for r in RS + ("-",):
                script.append("I %d %d %d %d %d %s" % (kind, 7, 37 * i + kind, i, 6, r))
                want.append(_want(kind, mk, s, 0 if r == "-" else r))
    script.append("S")
    want.append(["s", "none"])
    got = emul(script)
    assert len(got) == len(want)
    for g, w, ln in zip(got, want, script[1:]):
        assert g == w, ln


def test_every_refusal_kind_and_the_status_word(emul):
    (mk, s), (mk2, s2) = _masters("refusal", 16, 2)
    ok, ok2 = _want(S.RTP, mk, s, 5), _want(S.RTCP, mk2, s2, (1 << 48) - 1)
    script = ["T 16 4", "M 0 1 %s %s" % (mk.hex(), s.hex()), "M 1 3 %s %s" % (mk2.hex(), s2.hex()), "S",
              "M 9 4 %s %s" % (mk.hex(), s.hex()), "M 5 4294967295 %s %s" % (mk.hex(), s.hex()), "S", "S",     # set_dev: record 4 and record ~0 do not exist; the lowest entry is named
              "I 1 8 0 1 7 5", "I 2 8 1 3 0 281474976710655", "S",                                             # the good ones: the last slot, the largest r
              "I 1 8 40 4 0 0", "S",                                                                             # index out of range
              "I 1 8 41 4294967295 0 0", "S",
              "I 1 8 42 0 0 0", "S",                                                                             # record unset
              "I 1 8 43 1 8 0", "S",                                                                             # slot out of range
              "I 1 8 44 1 4294967295 0", "S",
              "I 1 8 45 1 0 281474976710656", "S",                                                              # r = 2^48
              "I 1 8 46 1 0 18446744073709551615", "S",
              "I 1 8 47 1 0 -", "S",                                                                             # ... no d_r: r = 0, good
              "C 1", "I 1 8 48 1 0 0",                                                                           # record cleared
              "I 2 8 7 2 0 0", "I 2 8 300 3 9 0", "S", "S",                                                      # several refused: the lowest entry is named, reading clears
              "I 2 8 2 3 0 281474976710655", "S"]                                                               # the neighbour record is as it was
    want = [["m", "ok"], ["m", "ok"], ["s", "none"], ["m", "refused"], ["m", "refused"], ["s", "5"], ["s", "none"],
            ok, ok2, ["s", "none"]]
    for i in (40, 41, 42, 43, 44, 45, 46):
        want += [["i", "refused"], ["s", str(i)]]
    want += [_want(S.RTP, mk, s, 0), ["s", "none"], ["i", "refused"], ["i", "refused"], ["i", "refused"], ["s", "7"], ["s", "none"], ok2, ["s", "none"]]
    assert emul(script) == want


def test_set_lane_stores_the_documented_record(emul):
    """a record is the key as it is, the 14 salt bytes at byte 32, zeros and the marker; a second set of the record replaces all of it.  The harness's arrays end
    with the entry, so the sanitizer build shows that the lane reads no byte past n * key_len and n * 14"""
    mk, s = _masters("record", 24, 1)[0]
    got = emul(["T 24 2", "M 0 1 %s %s" % (mk.hex(), s.hex()), "B 1 0 0", "I 1 1 0 1 0 0", "M 1 1 %s %s" % ((b"\xff" * 24).hex(), bytes(14).hex()), "B 1 0 0"])
    assert got == [["m", "ok"], ["b", (s + b"\0\0").hex()], _want(S.RTP, mk, s, 0), ["m", "ok"], ["b", bytes(16).hex()]]


# ---------------------------------------------------------------- the kernels' assembly
@pytest.fixture(scope="module")
def census():
    return asm_census("srtp_kdf")


def test_srtp_kdf_kernel_set(census):
    assert set(census) == {"k_srtp_kdf_install<10>", "k_srtp_kdf_install<12>", "k_srtp_kdf_install<14>", "k_srtp_kdf_set"}, sorted(census)


def test_srtp_kdf_kernels_scratch_free_and_in_budget(census):
    """the master key's schedule, the PRF's state and the session key's schedule stay in registers: no instance touches private memory or passes the other families'
    budget of 128 registers"""
    assert_in_budget(census, body="k_srtp_kdf_install<")


def test_srtp_kdf_source_is_a_unit_of_its_own_and_the_other_listings_are_unchanged():
    others = [f for f in os.listdir(CSRC) if f.endswith("_kernels.hip") and f != "aesgcm_srtp_kdf_kernels.hip"] + ["aesgcm_kernels.hip"]
    assert len(others) >= 11
    for f in others:
        assert "k_srtp_kdf_" not in open(os.path.join(CSRC, f)).read(), f
    assert '#include "aesgcm_srtp_kdf_kernels.hip"' in open(os.path.join(CSRC, "aesgcm_device.hip")).read()
    mk = open(os.path.join(CSRC, "Makefile")).read().splitlines()
    assert "srtp_kdf" in [w for ln in mk if ln.startswith("FAMILIES") for w in ln.split()] and "aesgcm_srtp_kdf" in [w for ln in mk if ln.startswith("UNITS") for w in ln.split()]
    hdr = "\n".join(ln.split("//")[0] for ln in open(os.path.join(CSRC, "aesgcm_srtp_kdf.h")).read().splitlines())
    kern = "\n".join(ln.split("//")[0] for ln in open(os.path.join(CSRC, "aesgcm_srtp_kdf_kernels.hip")).read().splitlines())
    slot = "\n".join(ln.split("//")[0] for ln in open(os.path.join(CSRC, "aesgcm_kdf_slot.h")).read().splitlines())
    assert "atomic" not in hdr and "atomic" not in kern and "atomic" not in slot          # the status word's minimum is kdf_refuse's, in aesgcm_kdf.h
    assert "asm" not in hdr and "asm" not in kern and "asm" not in slot
    # one schedule and one slot build for both derivation families
    assert "kdf_key_schedule<NR>(rk, smem, lb);" in slot and "kdf_key_schedule<NR>(rk, smem, lb);" in hdr
    for f in ("aesgcm_kdf_kernels.hip", "aesgcm_srtp_kdf_kernels.hip"):
        text = open(os.path.join(CSRC, f)).read()
        assert "kdf_slot_build<NR>(d, rk, smem" in text and "void kdf_slot_build" not in text, f
    note = open(os.path.join(ROOT, "profiles", "srtp_kdf", "isa_unchanged.txt")).read()
    assert "every instruction stream identical: yes" in note and "no scratch" in note
