"""CPU: on-device key derivation (aesgcm_kdf_*: traffic secrets on the device, HKDF-Expand-Label over HMAC-SHA-256 / HMAC-SHA-384) without a GPU.  The binding and the
header name the entry points and the ABI version is still 5; the KdfFormat presets give the documented labels byte for byte; aesgcm_kdf_fmt_check refuses what it must;
every call refuses its argument errors before it looks at a table or a device; the lane code of csrc/aesgcm_kdf.h, run by the CPU harness tests/kdf_emul, is held to
hashlib and to the HKDF-Expand-Label of tls_fixture, quic_fixture and dtls_fixture, and to RFC 9001 Appendix A through quic_fixture.initial_keys; the same harness built
with AddressSanitizer and UndefinedBehaviorSanitizer runs the same scripts clean; the gfx950 assembly of the kernels (`make -C csrc asm_kdf`) holds exactly the kernels
the design names, none with scratch."""
import ctypes
import hashlib
import hmac
import os
import random
import subprocess

import pytest

import aesgcm_amd  # noqa: F401
from aesgcm_amd import lib

from kt_common import asm_census

import dtls_fixture as D
import quic_fixture as Q
import tls_fixture as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "aes-gcm-128-192-256-bits_amd", "csrc")
NAMES = ("create", "set", "set_dev", "clear", "fmt_check", "install_dev", "update_dev", "status", "destroy")
HASH = {32: "sha256", 48: "sha384"}
LABELS = {"tls13": (b"tls13 key", b"tls13 iv", b"", b"tls13 traffic upd"),
          "quic_v1": (b"tls13 quic key", b"tls13 quic iv", b"tls13 quic hp", b"tls13 quic ku"),
          "quic_v2": (b"tls13 quicv2 key", b"tls13 quicv2 iv", b"tls13 quicv2 hp", b"tls13 quicv2 ku"),
          "dtls13": (b"dtls13key", b"dtls13iv", b"dtls13sn", b"dtls13traffic upd")}


# ---------------------------------------------------------------- binding, header, documents
def test_kdf_symbols_in_binding_and_header():
    hdr = open(os.path.join(ROOT, "include", "aesgcm.h")).read()
    for n in NAMES:
        assert "aesgcm_kdf_" + n in lib.SYMBOLS
        assert "AESGCM_API int aesgcm_kdf_%s(" % n in hdr
    assert "#define AESGCM_ABI_VERSION 5 " in hdr and "aesgcm_kdf_*" in hdr[hdr.index("#define AESGCM_ABI_VERSION 5 "):hdr.index("5 (round 6)")]
    section = hdr[hdr.index("ON-DEVICE KEY DERIVATION: TLS 1.3"):hdr.index("} aesgcm_kdf_fmt;")]
    for word in ("PROTECT IT LIKE KEYS", "exactly four compressions", "NOTHING an entry names is written", "d_aux_slots = NULL", "0xFFFFFFFF", "capture-safe",
                 "NO DERIVED KEY IN MEMORY", "in place", "HKDF-Extract", "TLS 1.2 PRF", "RFC 3711 4.3", "ChaCha20 and CCM", "Initial salt", "key\n * table's status is not touched"):
        assert word in section, word
    capture = hdr[hdr.index(" * CAPTURE (key tables"):hdr.index("tests/test_gpu_capture.py replays")]
    assert "aesgcm_kdf_install_dev and aesgcm_kdf_update_dev" in capture and "aesgcm_kdf_create, _set, _set_dev, _clear, _status, _destroy" in capture
    assert capture.index("NOT CAPTURE-SAFE") < capture.index("aesgcm_kdf_create, _set")
    L = lib._kdf_typed(lib.load())
    assert L.aesgcm_abi_version() == 5
    assert [len(getattr(L, "aesgcm_kdf_" + n).argtypes) for n in NAMES] == [4, 5, 5, 4, 1, 8, 6, 3, 1]
    for m in ("set", "set_dev", "clear", "install_dev", "update_dev", "install", "update", "status", "close", "__enter__", "__exit__"):
        assert callable(getattr(lib.SecretTable, m)), m
    assert issubclass(lib.SecretTable, lib._Table) and issubclass(lib.KdfFormat, lib._Format)
    assert ctypes.sizeof(lib.KdfFormat) == 84


def test_documents_say_what_the_issue_asks():
    for doc, words in (("INTEGRATION.md", ("## Key derivation", "traffic secret", "protected like keys", "`update`", "`install`", "unused slot", "`clear` the old slot", "next phase",
                                           "d_aux_slots = NULL", "HKDF-Extract", "TLS 1.2 PRF", "RFC 3711 4.3", "ChaCha20", "CCM", "Initial salt")),
                       ("DESIGN.md", ("On-device key derivation", "k_kdf_install", "k_kdf_update", "test_gpu_kdf.py", "test_kdf_cpu.py", "four compressions")),
                       ("README.md", ("On-device key derivation", "SecretTable", "profiles/kdf/ab.txt")),
                       (os.path.join("tests", "COVERAGE_kdf.md"), ("Key derivation", "test_gpu_kdf.py", "kdf_emul", "KeyUpdate", "RFC 9369"))):
        text = open(os.path.join(ROOT, doc)).read()
        for w in words:
            assert w in text, (doc, w)


def test_presets_give_the_documented_labels_byte_for_byte():
    F = lib.KdfFormat
    got = {"tls13": F.tls13(), "quic_v1": F.quic_v1(), "quic_v2": F.quic_v2(), "dtls13": F.dtls13()}
    for name, f in got.items():
        assert f.labels() == LABELS[name], name
        assert list(f.len) == [len(x) for x in LABELS[name]]
        raw = bytes(f)
        assert len(raw) == 84 and raw[:4] == bytes(len(x) for x in LABELS[name])
        for j, lab in enumerate(LABELS[name]):
            assert raw[4 + 20 * j:24 + 20 * j] == lab.ljust(20, b"\0"), (name, j)               # the label, then zeros: nothing else in the struct
        assert f.check() == lib.OK
    for name, rfc in (("tls13", "RFC 8446 7.3"), ("quic_v1", "RFC 9001 5.1"), ("quic_v2", "RFC 9369 3.3.2"), ("dtls13", "RFC 9147 5.9")):
        assert rfc in getattr(F, name).__doc__, name
    c = F.custom(b"k", b"i" * 20, None, b"")
    assert c.labels() == (b"k", b"i" * 20, b"", b"") and c.check() == lib.OK
    assert repr(F.tls13()) == "KdfFormat(b'tls13 key', b'tls13 iv', b'', b'tls13 traffic upd')"
    # the prefixes are the fixtures' own
    assert T.hkdf_expand_label("sha256", b"s" * 32, b"key", 16) == Q.hkdf_expand_label(b"s" * 32, b"key", 16)
    assert LABELS["dtls13"][0] == b"dtls13" + b"key" and LABELS["tls13"][0] == b"tls13 " + b"key"


def test_format_check():
    F = lib.KdfFormat
    assert lib._kdf_typed(lib.load()).aesgcm_kdf_fmt_check(None) == lib.EARG
    assert F.custom(b"", b"tls13 iv").check() == lib.EARG                     # no label 0
    assert F().check() == lib.EARG
    for j in range(4):
        labs = [b"a", b"b", b"c", b"d"]
        labs[j] = b"x" * 20
        assert F.custom(*labs).check() == lib.OK, j
        for n in (21, 22, 64, 255):
            labs[j] = b"x" * n
            assert F.custom(*labs).check() == lib.EARG, (j, n)                # longer than 20: an HMAC would no longer be four compressions
    assert F.custom(b"k").check() == lib.OK                                    # a key label alone is a format; install asks for label 1 as well


def test_argument_errors_before_any_table_or_device():
    """k = NULL, keytab = NULL and placeholder pointers that are never followed: every call returns before it touches a table or a device"""
    L = lib._kdf_typed(lib.load())
    P = 16                                                                   # a placeholder pointer
    quic, tls = lib.KdfFormat.quic_v1(), lib.KdfFormat.tls13()
    bad = lib.KdfFormat.custom(b"k" * 21, b"iv")

    def inst(fmt=quic, k=None, kt=None, n=1, idx=P, slots=P, aux=P):
        return L.aesgcm_kdf_install_dev(k, ctypes.byref(fmt) if fmt is not None else None, kt, n, idx, slots, aux, None)

    def upd(fmt=quic, k=None, n=1, frm=P, to=P):
        return L.aesgcm_kdf_update_dev(k, ctypes.byref(fmt) if fmt is not None else None, n, frm, to, None)

    assert inst(fmt=None, k=P, kt=P) == lib.EARG and upd(fmt=None, k=P) == lib.EARG          # the format first
    assert inst(fmt=bad, k=P, kt=P, n=0) == lib.EARG and upd(fmt=bad, k=P, n=0) == lib.EARG
    assert inst(fmt=tls, k=P, kt=P, n=0, aux=P) == lib.EARG                                  # aux slots with a format that has no label 2
    assert inst(fmt=lib.KdfFormat.custom(b"key"), k=P, kt=P, n=0, aux=None) == lib.EARG      # no label 1: a slot is a key and an IV
    assert upd(fmt=lib.KdfFormat.custom(b"key", b"iv"), k=P, n=0) == lib.EARG                # no label 3
    assert inst() == lib.EARG and inst(k=P) == lib.EARG and inst(kt=P) == lib.EARG           # k or keytab NULL
    assert inst(n=0) == lib.EARG and upd() == lib.EARG and upd(n=0) == lib.EARG              # ... whatever else
    assert inst(k=P, kt=P, n=0) == lib.OK and inst(k=P, kt=P, n=0, idx=None, slots=None, aux=None) == lib.OK      # nothing to do: nothing is looked at
    assert inst(fmt=tls, k=P, kt=P, n=0, aux=None) == lib.OK
    assert upd(k=P, n=0) == lib.OK and upd(k=P, n=0, frm=None, to=None) == lib.OK
    assert inst(k=P, kt=P, idx=None) == lib.EARG and inst(k=P, kt=P, slots=None) == lib.EARG and inst(k=P, kt=P, n=2 ** 31) == lib.EARG
    assert upd(k=P, frm=None) == lib.EARG and upd(k=P, to=None) == lib.EARG and upd(k=P, n=2 ** 31) == lib.EARG
    out = ctypes.c_void_p(5)
    assert L.aesgcm_kdf_create(None, 0, 32, 1) == lib.EARG
    for hash_len, n in ((0, 1), (16, 1), (20, 1), (33, 1), (64, 1), (32, 0), (48, 0), (32, 2 ** 31), (48, 2 ** 40)):
        assert L.aesgcm_kdf_create(ctypes.byref(out), 0, hash_len, n) == lib.EARG, (hash_len, n)
        assert out.value is None
    one = bytes(48)
    assert L.aesgcm_kdf_set(None, 0, 1, one, None) == lib.EARG and L.aesgcm_kdf_set(None, 0, 0, one, None) == lib.EARG
    assert L.aesgcm_kdf_set_dev(None, 1, P, P, None) == lib.EARG and L.aesgcm_kdf_clear(None, 0, 1, None) == lib.EARG
    code = ctypes.c_int(7)
    assert L.aesgcm_kdf_status(None, ctypes.byref(code), None) == lib.EARG
    assert L.aesgcm_kdf_destroy(None) == lib.OK


def test_the_derivation_units_reach_the_key_table_through_kt_view():
    """(that the fake runtime of tests/fake_hip links this unit and every other one is tests/test_fake_hip.py's: its libraries export the product's ABI exactly)"""
    assert "KtView kt_view(const aesgcm_keytab *t)" in open(os.path.join(CSRC, "aesgcm_keytab.hip")).read()
    assert "KtView kt_view(const aesgcm_keytab *t);" in open(os.path.join(CSRC, "aesgcm_keytab.h")).read()


# ---------------------------------------------------------------- the lane code on the CPU
@pytest.fixture(scope="module", params=["emul", "emul_asan"])
def emul(request):
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    d = os.path.join(ROOT, "tests", "kdf_emul")
    subprocess.run(["make", "-C", d, "-s", request.param], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)

    def run(script):
        out = subprocess.run([os.path.join(d, request.param)], input="\n".join(script) + "\n", stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
        assert out.returncode == 0 and "runtime error" not in out.stdout and "Sanitizer" not in out.stdout and "bad script" not in out.stdout, out.stdout[-3000:]
        return [ln.split() for ln in out.stdout.splitlines()]
    return run


def test_one_block_hashes_equal_hashlib(emul):
    rng = random.Random("kdf hash")
    msgs = {32: [b"", b"a", b"abc", bytes(rng.randrange(256) for _ in range(55)), b"\xff" * 55], 48: [b"", b"a", b"abc", bytes(rng.randrange(256) for _ in range(111)), b"\xff" * 111]}
    script, want = [], []
    for hl, ms in msgs.items():
        for m in ms:
            script.append("H %d %s" % (hl, m.hex() or "-"))
            want.append(["h", hashlib.new(HASH[hl], m).hexdigest()])
    assert emul(script) == want


def _expand_cases():
    """(hash_len, secret, full label, L, expected) over every label length 1 .. 20, every L, both hashes and the three fixtures' own derivations"""
    rng = random.Random("kdf expand")
    cases = []
    for hl in (32, 48):
        for L in (12, 16, 24, 32) + ((48,) if hl == 48 else ()):
            for n in range(1, 21):
                sec = bytes(rng.randrange(256) for _ in range(hl))
                if n >= 7:                                                   # "tls13 " + a label of n - 6 bytes, by the TLS and the QUIC fixture; "dtls13" + ...
                    rest = bytes(rng.randrange(32, 127) for _ in range(n - 6))
                    want = T.hkdf_expand_label(HASH[hl], sec, rest, L)
                    assert want == Q.hkdf_expand_label(sec, rest, L, HASH[hl])
                    cases.append((hl, sec, b"tls13 " + rest, L, want))
                    cases.append((hl, sec, b"dtls13" + rest, L, D.hkdf_expand_label13(HASH[hl], sec, rest, L)))
                else:                                                        # shorter than any prefix: the same formula on the full label (RFC 8446 7.1 with the label as it is)
                    full = bytes(rng.randrange(32, 127) for _ in range(n))
                    info = bytes([L >> 8, L & 255, n]) + full + b"\0"
                    cases.append((hl, sec, full, L, hmac.new(sec, info + b"\x01", HASH[hl]).digest()[:L]))
    # the edge secrets and a few hundred random ones under the presets' labels
    for hl in (32, 48):
        for sec in (bytes(hl), b"\xff" * hl, b"\x36" * hl, b"\x5c" * hl):
            cases.append((hl, sec, b"tls13 key", 16, T.hkdf_expand_label(HASH[hl], sec, b"key", 16)))
        for k in range(150):
            sec = bytes(rng.randrange(256) for _ in range(hl))
            name = rng.choice(sorted(LABELS))
            j = rng.choice([j for j in range(4) if LABELS[name][j]])
            L = (16, 12, 32, hl)[j] if j != 0 else rng.choice((16, 24, 32))
            full = LABELS[name][j]
            want = D.hkdf_expand_label13(HASH[hl], sec, full[6:], L) if name == "dtls13" else T.hkdf_expand_label(HASH[hl], sec, full[6:], L)
            cases.append((hl, sec, full, L, want))
    return cases


def test_expand_label_equals_the_fixtures(emul):
    cases = _expand_cases()
    assert len(cases) > 600 and {len(c[2]) for c in cases} >= set(range(1, 21)) and {(c[0], c[3]) for c in cases} >= {(32, 12), (32, 16), (32, 24), (32, 32), (48, 12), (48, 48)}
    got = emul(["X %d %s %s %d" % (hl, sec.hex(), full.hex(), L) for hl, sec, full, L, _ in cases])
    assert len(got) == len(cases)
    for g, c in zip(got, cases):
        assert g == ["x", c[4].hex()], (c[0], c[2], c[3])


def test_quic_v1_labels_on_the_client_initial_secret_of_rfc9001_appendix_a(emul):
    dcid = bytes.fromhex("8394c8f03e515708")                                  # RFC 9001 A.1
    secret = Q.hkdf_expand_label(Q.hkdf_extract(Q.INITIAL_SALT_V1, dcid), b"client in", 32)
    assert secret.hex() == "c00cf151ca5be075ed0ebfb5c80323c42d6b7db67881289af4008f1f6c357aea"
    key, iv, hp = Q.initial_keys(dcid, "client")
    labs = LABELS["quic_v1"]
    got = emul(["X 32 %s %s %d" % (secret.hex(), labs[j].hex(), L) for j, L in ((0, 16), (1, 12), (2, 16))])
    assert got == [["x", key.hex()], ["x", iv.hex()], ["x", hp.hex()]]
    assert key.hex() == "1f369613dd76d5467730efcbe3b1a22d" and iv.hex() == "fa044b2f42a3fd3b46fb255c" and hp.hex() == "9f50449e04a0e810283a1e9933adedd2"


# ---------------------------------------------------------------- the kernels' assembly
@pytest.fixture(scope="module")
def census():
    return asm_census("kdf")


def test_kdf_kernel_set(census):
    assert {n.split("(")[0].split("<")[0] for n in census} == {"k_kdf_install", "k_kdf_update", "k_kdf_set"}, sorted(census)
    assert len(census) == 3 * 2 + 2 + 1, sorted(census)                       # install: three key sizes x two hashes; update: two hashes; set


def test_kdf_kernels_have_no_scratch(census):
    """no instance touches private memory: the message schedule and the round keys stay in registers.  The SHA-384 instances may take more than the 128 registers of
    the other families' budget (64-bit words; profiles/kdf/isa_unchanged.txt lists them), the SHA-256 ones may not"""
    for name, k in census.items():
        assert k["scratch"] == 0, (name, k["scratch"])
        assert k["vgpr"] <= (256 if "48" in name.split("k_kdf_")[1] else 128), (name, k["vgpr"])


def test_kdf_source_is_a_unit_of_its_own_and_the_other_listings_are_unchanged():
    others = [f for f in os.listdir(CSRC) if f.endswith("_kernels.hip") and f != "aesgcm_kdf_kernels.hip"] + ["aesgcm_kernels.hip"]
    assert len(others) >= 10
    for f in others:
        assert "k_kdf_" not in open(os.path.join(CSRC, f)).read(), f
    assert '#include "aesgcm_kdf_kernels.hip"' in open(os.path.join(CSRC, "aesgcm_device.hip")).read()
    mk = open(os.path.join(CSRC, "Makefile")).read().splitlines()
    assert "kdf" in [w for ln in mk if ln.startswith("FAMILIES") for w in ln.split()] and "aesgcm_kdf" in [w for ln in mk if ln.startswith("UNITS") for w in ln.split()]
    hdr = "\n".join(ln.split("//")[0] for ln in open(os.path.join(CSRC, "aesgcm_kdf.h")).read().splitlines())
    assert hdr.count("atomic") == 1 and "atomicMin(status, i)" in hdr and "__constant__" in hdr and "__builtin_amdgcn_alignbit" in hdr
    kern = "\n".join(ln.split("//")[0] for ln in open(os.path.join(CSRC, "aesgcm_kdf_kernels.hip")).read().splitlines())
    assert "atomic" not in kern
    note = open(os.path.join(ROOT, "profiles", "kdf", "isa_unchanged.txt")).read()
    assert "every instruction stream identical: yes" in note and "no scratch" in note
