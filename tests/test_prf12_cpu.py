"""CPU: the TLS 1.2 PRF on the device (aesgcm_prf12_*: master secrets on the device, P_hash over HMAC-SHA-256 / HMAC-SHA-384) without a GPU.  The binding and the header
name the eight entry points and the ABI version is still 5; every call refuses its argument errors before it looks at a table or a device; the documents say what they
must and the phrases that other tests pin are pointers now; the lane code of csrc/aesgcm_prf12.h, run by the CPU harness tests/prf12_emul (plain, and under
AddressSanitizer and UndefinedBehaviorSanitizer), is held to hmac through tls_fixture.prf12, to tls_fixture.derive and dtls_fixture.keys12 on the four recorded
connections, and its verdicts to every refusal kind; the gfx950 assembly of the kernels (`make -C csrc asm_prf12`) holds exactly the kernels the design names, none
with scratch, with the register counts DESIGN.md records."""
import ctypes
import os
import random
import re
import subprocess

import pytest

import aesgcm_amd  # noqa: F401
from aesgcm_amd import lib

from kt_common import asm_census

import dtls_fixture as D
import tls_fixture as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "aes-gcm-128-192-256-bits_amd", "csrc")
NAMES = ("create", "set", "set_dev", "clear", "install_dev", "export_srtp_dev", "status", "destroy")
HASH = {32: "sha256", 48: "sha384"}
KEX, EXP = b"key expansion", b"EXTRACTOR-dtls_srtp"


# ---------------------------------------------------------------- binding, header, documents
def test_prf12_symbols_in_binding_and_header():
    hdr = open(os.path.join(ROOT, "include", "aesgcm.h")).read()
    for n in NAMES:
        assert "aesgcm_prf12_" + n in lib.SYMBOLS
        assert "AESGCM_API int aesgcm_prf12_%s(" % n in hdr
    assert len([s for s in lib.SYMBOLS if s.startswith("aesgcm_prf12_")]) == 8 and "typedef struct aesgcm_prf12 aesgcm_prf12;" in hdr
    assert "#define AESGCM_ABI_VERSION 5 " in hdr and "aesgcm_prf12_*" in hdr[hdr.index("#define AESGCM_ABI_VERSION 5 "):hdr.index("5 (round 6)")]
    section = hdr[hdr.index("TLS 1.2 PRF: TLS 1.2 and DTLS 1.2"):hdr.index("typedef struct aesgcm_prf12 aesgcm_prf12;")]
    for word in ("PROTECT IT LIKE KEYS", "RFC 5246 section 5", "\"key expansion\" | server_random | client_random", "\"EXTRACTOR-dtls_srtp\" | client_random | server_random",
                 "OTHER ORDER", "client_write_IV | 8 zero bytes", "two zero bytes appended", "0xFFFFFFFF", "not both", "NOTHING an entry names is written",
                 "status words are not touched", "NO DERIVED KEY IN MEMORY", "capture-safe", "key_len 24", "RFC 7627", "verify_data", "CBC suites", "exporters with a context",
                 "prf+", "MKA KDF"):
        assert word in section, word
    capture = hdr[hdr.index(" * CAPTURE (key tables"):hdr.index("tests/test_gpu_capture.py replays")]
    assert "aesgcm_prf12_install_dev and aesgcm_prf12_export_srtp_dev" in capture and "aesgcm_prf12_create, _set, _set_dev, _clear, _status, _destroy" in capture
    assert capture.index("NOT CAPTURE-SAFE") < capture.index("aesgcm_prf12_create, _set")
    # the phrases that said "out of scope" point at this table now
    for a, b in (("ON-DEVICE KEY DERIVATION: TLS 1.3", "} aesgcm_kdf_fmt;"), ("SRTP KEY DERIVATION: SRTP and SRTCP session keys", "typedef struct aesgcm_srtp_kdf aesgcm_srtp_kdf;"),
                 ("SRTP AND SRTCP PACKETS", "aesgcm_srtp_fmt;")):
        assert "aesgcm_prf12_" in hdr[hdr.index(a):hdr.index(b)], a
    L = lib._prf12_typed(lib.load())
    assert L.aesgcm_abi_version() == 5
    assert [len(getattr(L, "aesgcm_prf12_" + n).argtypes) for n in NAMES] == [4, 7, 7, 4, 7, 7, 3, 1]
    for m in ("set", "set_dev", "clear", "install_dev", "export_srtp_dev", "install", "export_srtp", "status", "close", "__enter__", "__exit__"):
        assert callable(getattr(lib.MasterSecretTable, m)), m
    assert issubclass(lib.MasterSecretTable, lib._Table) and lib.MasterSecretTable._prefix == "aesgcm_prf12"


def test_documents_say_what_the_issue_asks():
    for doc, words in (("INTEGRATION.md", ("TLS 1.2 and DTLS 1.2 keys", "MasterSecretTable", "master secret", "protected like keys", "export_srtp", "MasterKeyTable", "crypt_srtp",
                                           "one stream", "RFC 7627", "TLS 1.2 PRF")),
                       ("DESIGN.md", ("TLS 1.2 PRF on the device", "k_prf12_install", "k_prf12_export", "k_prf12_set", "test_gpu_prf12.py", "test_prf12_cpu.py", "aesgcm_srtp_kdf.hip")),
                       ("README.md", ("TLS 1.2 PRF", "MasterSecretTable")),
                       (os.path.join("tests", "COVERAGE_prf12.md"), ("OpenSSL", "RFC 5705", "prf12_emul", "test_gpu_prf12.py", "keymatexport"))):
        text = open(os.path.join(ROOT, doc)).read()
        for w in words:
            assert w in text, (doc, w)
    assert "The derivation is the caller's (`tests/tls_fixture.py` has both in a dozen lines of `hmac`)" not in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_argument_errors_before_any_table_or_device():
    """p = NULL, a table = NULL and placeholder pointers that are never followed: every call returns before it touches a table or a device"""
    L = lib._prf12_typed(lib.load())
    P = 16                                                                   # a placeholder pointer

    for call in (L.aesgcm_prf12_install_dev, L.aesgcm_prf12_export_srtp_dev):
        def go(p=None, other=None, n=1, idx=P, c=P, s=P):
            return call(p, other, n, idx, c, s, None)
        assert go() == lib.EARG and go(p=P) == lib.EARG and go(other=P) == lib.EARG and go(n=0) == lib.EARG
        assert go(p=P, other=P, n=0) == lib.OK and go(p=P, other=P, n=0, idx=None, c=None, s=None) == lib.OK      # nothing to do: nothing is looked at
        assert go(p=P, other=P, idx=None) == lib.EARG and go(p=P, other=P, c=None, s=None) == lib.EARG and go(p=P, other=P, n=2 ** 31) == lib.EARG
    out = ctypes.c_void_p(5)
    assert L.aesgcm_prf12_create(None, 0, 32, 1) == lib.EARG
    for hash_len, n in ((0, 1), (16, 1), (20, 1), (33, 1), (64, 1), (32, 0), (48, 0), (32, 2 ** 31), (48, 2 ** 40)):
        assert L.aesgcm_prf12_create(ctypes.byref(out), 0, hash_len, n) == lib.EARG, (hash_len, n)
        assert out.value is None
    one = bytes(48)
    assert L.aesgcm_prf12_set(None, 0, 1, one, one, one, None) == lib.EARG and L.aesgcm_prf12_set(None, 0, 0, one, one, one, None) == lib.EARG
    assert L.aesgcm_prf12_set_dev(None, 1, P, P, P, P, None) == lib.EARG and L.aesgcm_prf12_clear(None, 0, 1, None) == lib.EARG
    code = ctypes.c_int(7)
    assert L.aesgcm_prf12_status(None, ctypes.byref(code), None) == lib.EARG
    assert L.aesgcm_prf12_destroy(None) == lib.OK


# ---------------------------------------------------------------- the lane code on the CPU
@pytest.fixture(scope="module", params=["emul", "emul_asan"])
def emul(request):
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    d = os.path.join(ROOT, "tests", "prf12_emul")
    subprocess.run(["make", "-C", d, "-s", request.param], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)

    def run(script):
        out = subprocess.run([os.path.join(d, request.param)], input="\n".join(script) + "\n", stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
        assert out.returncode == 0 and "runtime error" not in out.stdout and "Sanitizer" not in out.stdout and "bad script" not in out.stdout, out.stdout[-3000:]
        return [ln.split() for ln in out.stdout.splitlines()]
    return run


def _rand(rng, n):
    return bytes(rng.randrange(256) for _ in range(n))


def test_p_hash_equals_hmac_for_both_hashes_both_labels_and_the_bound_edges(emul):
    rng = random.Random("prf12 p_hash")
    cases = []
    for hl in (32, 48):
        for label in (KEX, EXP, b"x", b"abcdefghijklmnopqrs\x00"):             # 13, 19, 1 and 20 bytes (a label may hold any byte)
            for nbytes in (4, 32, 40, 48, 56, 72, 88, 96, 100, 200):
                cases.append((hl, _rand(rng, 48), label, _rand(rng, 32), _rand(rng, 32), nbytes))
        for sec in (bytes(48), b"\xff" * 48, b"\x36" * 48, b"\x5c" * 48):
            cases.append((hl, sec, KEX, b"\xff" * 32, bytes(32), 72))
    assert {len(c[2]) for c in cases} == {1, 13, 19, 20}
    got = emul(["P %d %s %s %s %s %d" % (hl, s.hex(), lab.hex(), r1.hex(), r2.hex(), nb) for hl, s, lab, r1, r2, nb in cases])
    assert len(got) == len(cases)
    for g, (hl, s, lab, r1, r2, nb) in zip(got, cases):
        assert g == ["p", T.prf12(HASH[hl], s, lab, r1 + r2, nb).hex()], (hl, lab, nb)


def test_the_padding_rule_gives_the_headers_block_counts_for_every_label_length(emul):
    """arithmetic only: the harness's N line applies the padding rule to the three message lengths and runs no lane code.  What holds the LANE code to the bound is
    the test above, at label lengths 1, 13, 19 and 20 against hmac"""
    got = emul(["N %d %d" % (hl, ll) for hl in (32, 48) for ll in range(1, 21)])
    assert got[:20] == [["n", "2", "1", "2"]] * 20 and got[20:] == [["n", "1", "1", "2"]] * 20


def _connections():
    out = [c for c in T.golden("tls_records.json")["connections"] if c["version"] != "1.3"] + list(D.golden("dtls12_records.json")["connections"])
    assert len(out) == 4 and {(c["hash"], c["key_len"]) for c in out} == {("sha256", 16), ("sha384", 32)}
    return out


def test_the_four_recorded_connections_split_as_the_fixtures_split_them(emul):
    script, want = [], []
    for k, c in enumerate(_connections()):
        hl = {"sha256": 32, "sha384": 48}[c["hash"]]
        ms, cr, sr = (bytes.fromhex(c[x]) for x in ("master_secret", "client_random", "server_random"))
        script += ["T %d 3" % hl, "M 0 2 %s %s %s" % (ms.hex(), cr.hex(), sr.hex()), "I %d 8 0 2 5 7" % c["key_len"]]
        keys = [D.keys12(ms, cr, sr, c["key_len"], who, c["hash"]) for who in ("client", "server")]
        if "dirs" in c and c.get("version") == "1.2":
            assert keys == [T.derive(c, who) for who in ("client", "server")]
        want += [["m", "ok"], ["i", keys[0][0].hex(), keys[0][1][:4].hex(), keys[1][0].hex(), keys[1][1][:4].hex()]]
    assert emul(script) == want


def _srtp_record(out, kl, d):
    """what aesgcm_srtp_kdf's record holds of direction d of an exporter output: key, zeros to byte 32, salt | 00 00, zeros, the marker"""
    return (out[d * kl:(d + 1) * kl].ljust(32, b"\0") + out[2 * kl + 12 * d:2 * kl + 12 * d + 12] + bytes(16) + b"MDES").hex()


def test_the_exporter_outputs_that_openssl_recorded(emul):
    """tests/golden/dtls_srtp_exporter.json: SSL_export_keying_material's bytes, not this project's reading of RFC 5705 -- the label, the order of the randoms and the
    absent context are OpenSSL's here.  The cut into keys and salts is RFC 5764 4.2's, applied to OpenSSL's bytes"""
    conns = T.golden("dtls_srtp_exporter.json")["connections"]
    assert {c["hash"] for c in conns} == {"sha256", "sha384"}
    script, want = [], []
    for c in conns:
        hl = {"sha256": 32, "sha384": 48}[c["hash"]]
        out = bytes.fromhex(c["exported"])
        assert len(out) == 88 and c["label"] == EXP.decode()
        script += ["T %d 1" % hl, "M 0 0 %s %s %s" % (c["master_secret"], c["client_random"], c["server_random"])]
        want.append(["m", "ok"])
        for kl in (16, 32):                                                  # (an exporter's shorter output is the longer one's beginning)
            script.append("E %d 2 0 0 0 1" % kl)
            want.append(["e", _srtp_record(out[:2 * kl + 24], kl, 0), _srtp_record(out[:2 * kl + 24], kl, 1)])
    assert emul(script) == want


def test_install_and_export_over_every_hash_and_key_size(emul):
    rng = random.Random("prf12 entries")
    script, want = [], []
    for hl in (32, 48):
        ms, cr, sr = _rand(rng, 48), _rand(rng, 32), _rand(rng, 32)
        script += ["T %d 2" % hl, "M 3 1 %s %s %s" % (ms.hex(), cr.hex(), sr.hex())]
        want.append(["m", "ok"])
        for kl in (16, 24, 32):
            block = T.prf12(HASH[hl], ms, KEX, sr + cr, 2 * kl + 8)
            ck, sk, civ, siv = block[:kl].hex(), block[kl:2 * kl].hex(), block[2 * kl:2 * kl + 4].hex(), block[2 * kl + 4:].hex()
            script += ["I %d 4 0 1 0 3" % kl, "I %d 4 5 1 - 3" % kl, "I %d 4 0 1 2 -" % kl, "I %d 4 0 1 x 3" % kl, "I %d 4 0 1 1 x" % kl]
            want += [["i", ck, civ, sk, siv], ["i", "-", "-", sk, siv], ["i", ck, civ, "-", "-"], ["i", "-", "-", sk, siv], ["i", ck, civ, "-", "-"]]
        for kl in (16, 32):
            out = T.prf12(HASH[hl], ms, EXP, cr + sr, 2 * kl + 24)

            def record(d):                                                   # what aesgcm_srtp_kdf's record holds: key, zeros to byte 32, salt | 00 00, zeros, the marker
                return (out[d * kl:(d + 1) * kl].ljust(32, b"\0") + out[2 * kl + 12 * d:2 * kl + 12 * d + 12] + bytes(16) + b"MDES").hex()
            script += ["E %d 6 0 1 4 5" % kl, "E %d 6 2 1 - 0" % kl, "E %d 6 0 1 x 0" % kl]
            want += [["e", record(0), record(1)], ["e", "-", record(1)], ["e", "-", record(1)]]
        script.append("S")
        want.append(["s", "none"])
    assert emul(script) == want


def test_the_verdict_over_every_refusal_kind(emul):
    one = "%s %s %s" % ("11" * 48, "22" * 32, "33" * 32)
    script = ["T 32 4", "M 0 0 " + one, "M 1 1 " + one, "M 2 4 " + one, "S",          # a set_dev index out of range
              "I 16 8 3 4 0 1", "I 16 8 2 3 0 1", "S",                                # index out of range; unset: the lowest goes to the status word
              "C 1", "I 16 8 9 1 0 1", "S",                                           # cleared
              "I 16 8 5 0 8 1", "I 16 8 4 0 0 8", "I 16 8 6 0 - 8", "I 16 8 7 0 8 -", "S",      # a slot out of range, in either array, alone or not
              "I 16 8 1 0 7 x", "S",                                                  # the last slot, and none: no refusal
              "E 16 2 3 0 2 0", "E 16 2 2 0 1 2", "E 32 2 8 3 0 1", "S",              # the exporter's records
              "E 16 2 0 0 x x", "S"]
    got = emul(script)
    assert got[:4] == [["m", "ok"], ["m", "ok"], ["m", "refused"], ["s", "2"]]
    assert got[4:7] == [["i", "refused"], ["i", "refused"], ["s", "2"]]
    assert got[7:9] == [["i", "refused"], ["s", "9"]]
    assert got[9:14] == [["i", "refused"]] * 4 + [["s", "4"]]
    assert got[14][0] == "i" and got[14][3:] == ["-", "-"] and got[15] == ["s", "none"]
    assert got[16:20] == [["e", "refused"]] * 3 + [["s", "2"]]
    assert got[20:] == [["e", "-", "-"], ["s", "none"]]


# ---------------------------------------------------------------- the kernels' assembly
@pytest.fixture(scope="module")
def census():
    return asm_census("prf12")


def test_prf12_kernel_set_has_no_scratch_and_the_recorded_registers(census):
    assert {n.split("(")[0].split("<")[0] for n in census} == {"k_prf12_install", "k_prf12_export", "k_prf12_set"}, sorted(census)
    assert len(census) == 3 * 2 + 2 + 1, sorted(census)                       # install: three key sizes x two hashes; export: two hashes; set
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    table = design[design.index("TLS 1.2 PRF on the device"):]
    for name, k in census.items():
        assert k["scratch"] == 0, (name, k["scratch"])
        assert k["vgpr"] <= 512, (name, k["vgpr"])                            # the census counts both register files; 512 is what a lane of a 256-lane workgroup can have
    assert "registers " + " / ".join(str(v) for v in sorted({k["vgpr"] for k in census.values()})) in table       # the distinct counts, ascending


def test_prf12_source_is_a_unit_of_its_own():
    others = [f for f in os.listdir(CSRC) if f.endswith("_kernels.hip") and f != "aesgcm_prf12_kernels.hip"] + ["aesgcm_kernels.hip"]
    assert len(others) >= 12
    for f in others:
        assert "k_prf12_" not in open(os.path.join(CSRC, f)).read(), f
    assert '#include "aesgcm_prf12_kernels.hip"' in open(os.path.join(CSRC, "aesgcm_device.hip")).read()
    mk = open(os.path.join(CSRC, "Makefile")).read().splitlines()
    assert "prf12" in [w for ln in mk if ln.startswith("FAMILIES") for w in ln.split()] and "aesgcm_prf12" in [w for ln in mk if ln.startswith("UNITS") for w in ln.split()]
    for f in os.listdir(CSRC):                                                # the host side: compiled once, as that unit, and included nowhere
        assert not f.endswith(".hip") or not re.search(r'#\s*include\s*"aesgcm_prf12\.hip"', open(os.path.join(CSRC, f)).read()), f
    for f in ("aesgcm_prf12.h", "aesgcm_prf12_kernels.hip"):
        code = "\n".join(ln.split("//")[0] for ln in open(os.path.join(CSRC, f)).read().splitlines())
        assert "atomic" not in code, f                                        # the only atomic is kdf_refuse's, in aesgcm_kdf.h
    note = open(os.path.join(ROOT, "profiles", "prf12", "isa_unchanged.txt")).read()
    assert "every instruction stream identical: yes" in note and "no scratch" in note and note.count("byte-identical") >= 10
    assert os.path.exists(os.path.join(ROOT, "profiles", "prf12", "ab.py"))
