"""CPU: IKEv2's prf+ on the device (aesgcm_prfplus_*: SK_d values on the device, prf+ of RFC 7296 2.13 over HMAC-SHA-256 / -384 / -512) without a GPU.  The binding and
the header name the seven entry points and the ABI version is still 5; every call refuses its argument errors before it looks at a table or a device; the documents say
what they must; the lane code of csrc/aesgcm_prfplus.h, run by the CPU harness tests/prfplus_emul (plain, and under AddressSanitizer and UndefinedBehaviorSanitizer), is
held to hmac through ikev2_ref.prf_plus at every seed length 1 .. 260 and 2047 / 2048, every start alignment and the pad-byte keys, its cut of KEYMAT to
ikev2_ref.child_sa, and its verdicts to every refusal kind; the gfx950 assembly of the kernels (`make -C csrc asm_prfplus`) holds exactly the kernels the design names,
none with scratch, with the register counts DESIGN.md records."""
import ctypes
import os
import random
import subprocess

import pytest

import aesgcm_amd  # noqa: F401
from aesgcm_amd import lib

from kt_common import asm_census

import ikev2_ref as IK

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "aes-gcm-128-192-256-bits_amd", "csrc")
NAMES = ("create", "set", "set_dev", "clear", "install_dev", "status", "destroy")
HLS = (32, 48, 64)


# ---------------------------------------------------------------- binding, header, documents
def test_prfplus_symbols_in_binding_and_header():
    hdr = open(os.path.join(ROOT, "include", "aesgcm.h")).read()
    for n in NAMES:
        assert "aesgcm_prfplus_" + n in lib.SYMBOLS
        assert "AESGCM_API int aesgcm_prfplus_%s(" % n in hdr
    assert len([s for s in lib.SYMBOLS if s.startswith("aesgcm_prfplus_")]) == 7 and "typedef struct aesgcm_prfplus aesgcm_prfplus;" in hdr
    assert "#define AESGCM_ABI_VERSION 5 " in hdr and "aesgcm_prfplus_*" in hdr[hdr.index("#define AESGCM_ABI_VERSION 5 "):hdr.index("5 (round 6)")]
    section = hdr[hdr.index("IKEv2 PRF+: ESP keys of Child SAs from SK_d values that never leave the device"):hdr.index("typedef struct aesgcm_prfplus aesgcm_prfplus;")]
    for word in ("PROTECT IT\n * LIKE KEYS", "RFC 7296 2.13", "RFC 7296 2.17", "RFC 4106 8.1", "T1 = prf(K, S | 0x01)", "Tn = prf(K, T(n-1) | S | n)",
                 "key_i2r | salt_i2r[4] | key_r2i | salt_r2i[4]", "d * (key_len + 4)", "salt_i2r | 00 00 00 00", "{8, 16, 8, 4, tag, 0}", "RFC 4543", "2048 bytes",
                 "DIFFIE-HELLMAN\n *   SHARED SECRET", "to protect and to wipe", "0xFFFFFFFF", "not both", "NOTHING an entry names is written", "offsets fall", "empty or longer",
                 "status word is not touched", "NO DERIVED KEY IN MEMORY", "capture-safe", "SKEYSEED", "IKEv1", "PRF_HMAC_SHA1", "AES-XCBC", "AES-CMAC",
                 "separate integrity key", "MKA KDF"):
        assert word in section, word
    capture = hdr[hdr.index(" * CAPTURE (key tables"):hdr.index("tests/test_gpu_capture.py replays")]
    assert "aesgcm_prfplus_install_dev" in capture and "aesgcm_prfplus_create, _set, _set_dev, _clear, _status, _destroy" in capture
    assert capture.index("aesgcm_prfplus_install_dev") < capture.index("NOT CAPTURE-SAFE") < capture.index("aesgcm_prfplus_create, _set")
    # the phrases that said "out of scope" point at this table now
    for a, b in (("ON-DEVICE KEY DERIVATION: TLS 1.3", "} aesgcm_kdf_fmt;"), ("SRTP KEY DERIVATION: SRTP and SRTCP session keys", "typedef struct aesgcm_srtp_kdf aesgcm_srtp_kdf;"),
                 ("TLS 1.2 PRF: TLS 1.2 and DTLS 1.2", "typedef struct aesgcm_prf12 aesgcm_prf12;")):
        assert "aesgcm_prfplus_" in hdr[hdr.index(a):hdr.index(b)], a
    L = lib._prfplus_typed(lib.load())
    assert L.aesgcm_abi_version() == 5
    assert [len(getattr(L, "aesgcm_prfplus_" + n).argtypes) for n in NAMES] == [4, 5, 5, 4, 9, 3, 1]
    for m in ("set", "set_dev", "clear", "install_dev", "install", "status", "close", "__enter__", "__exit__"):
        assert callable(getattr(lib.IkeSaTable, m)), m
    assert issubclass(lib.IkeSaTable, lib._Table) and lib.IkeSaTable._prefix == "aesgcm_prfplus"
    assert not [s for s in lib.SYMBOLS if "prfplus" in s and (s.startswith("aesgcm_prf12_") or s.startswith("aesgcm_kdf_"))]


def test_documents_say_what_the_issue_asks():
    for doc, words in (("INTEGRATION.md", ("ESP rekey", "IkeSaTable", "SK_d", "one stream", "fresh slots", "refuses at the limit", "Ni | Nr")),
                       ("DESIGN.md", ("IKEv2 prf+ on the device", "k_prfp_install", "k_prfp_set", "run-time", "test_gpu_prfplus.py", "test_prfplus_cpu.py", "aesgcm_prf12.hip",
                                      "ACCEPTED RECOMPUTATION")),
                       ("README.md", ("IKEv2 prf+", "IkeSaTable", "RFC 7296's formula alone", "profiles/prfplus/ab.py")),
                       (os.path.join("tests", "COVERAGE_prfplus.md"), ("RFC 7296", "formula alone", "prfplus_emul", "test_gpu_prfplus.py", "ikev2_ref", "OpenSSL 3.0"))):
        text = open(os.path.join(ROOT, doc)).read()
        for w in words:
            assert w in text, (doc, w)


def test_argument_errors_before_any_table_or_device():
    """p = NULL, a table = NULL and placeholder pointers that are never followed: every call returns before it touches a table or a device"""
    L = lib._prfplus_typed(lib.load())
    P = 16                                                                   # a placeholder pointer

    def go(p=None, kt=None, n=1, idx=P, seed=P, off=P, a=P, b=P):
        return L.aesgcm_prfplus_install_dev(p, kt, n, idx, seed, off, a, b, None)
    assert go() == lib.EARG and go(p=P) == lib.EARG and go(kt=P) == lib.EARG and go(n=0) == lib.EARG
    assert go(p=P, kt=P, n=0) == lib.OK and go(p=P, kt=P, n=0, idx=None, seed=None, off=None, a=None, b=None) == lib.OK      # nothing to do: nothing is looked at
    for missing in ("idx", "seed", "off"):
        assert go(p=P, kt=P, **{missing: None}) == lib.EARG, missing
    assert go(p=P, kt=P, a=None, b=None) == lib.EARG and go(p=P, kt=P, n=2 ** 31) == lib.EARG
    out = ctypes.c_void_p(5)
    assert L.aesgcm_prfplus_create(None, 0, 32, 1) == lib.EARG
    for hash_len, n in ((0, 1), (16, 1), (20, 1), (33, 1), (63, 1), (65, 1), (128, 1), (32, 0), (48, 0), (64, 0), (32, 2 ** 31), (64, 2 ** 40)):
        assert L.aesgcm_prfplus_create(ctypes.byref(out), 0, hash_len, n) == lib.EARG, (hash_len, n)
        assert out.value is None
    one = bytes(64)
    assert L.aesgcm_prfplus_set(None, 0, 1, one, None) == lib.EARG and L.aesgcm_prfplus_set(None, 0, 0, one, None) == lib.EARG
    assert L.aesgcm_prfplus_set_dev(None, 1, P, P, None) == lib.EARG and L.aesgcm_prfplus_clear(None, 0, 1, None) == lib.EARG
    code = ctypes.c_int(7)
    assert L.aesgcm_prfplus_status(None, ctypes.byref(code), None) == lib.EARG
    assert L.aesgcm_prfplus_destroy(None) == lib.OK


# ---------------------------------------------------------------- the lane code on the CPU
@pytest.fixture(scope="module", params=["emul", "emul_asan"])
def emul(request):
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    d = os.path.join(ROOT, "tests", "prfplus_emul")
    subprocess.run(["make", "-C", d, "-s", request.param], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)

    def run(script):
        out = subprocess.run([os.path.join(d, request.param)], input="\n".join(script) + "\n", stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
        assert out.returncode == 0 and "runtime error" not in out.stdout and "Sanitizer" not in out.stdout and "bad script" not in out.stdout, out.stdout[-3000:]
        return [ln.split() for ln in out.stdout.splitlines()]
    return run


def _rand(rng, n):
    return rng.getrandbits(8 * n).to_bytes(n, "big")


def _held(emul, cases):
    """cases: (hl, key, seed, align, n_t)"""
    got = emul(["H %d %s %s %d %d" % (hl, k.hex(), s.hex(), al, nt) for hl, k, s, al, nt in cases])
    assert len(got) == len(cases)
    for g, (hl, k, s, al, nt) in zip(got, cases):
        assert g == ["h", IK.prf_plus(hl, k, s, nt * hl).hex()], (hl, len(s), al, nt)


@pytest.mark.parametrize("hl", HLS)
def test_prf_plus_equals_hmac_at_every_seed_length_to_260(emul, hl):
    """every length at every start alignment 0 .. 3, three T(n) each: T1's message S | n and T2's, T3's message T | S | n pass every padding edge (55 / 56 mod 64,
    111 / 112 mod 128, the exact blocks), and every tail residue mod 4 meets every alignment"""
    rng = random.Random("prfplus lengths %d" % hl)
    cases = [(hl, _rand(rng, hl), _rand(rng, n), al, 3) for n in range(1, 261) for al in range(4)]
    assert len(cases) == 1040
    _held(emul, cases)


def test_prf_plus_at_the_longest_seeds_every_alignment_and_the_pad_byte_keys(emul):
    rng = random.Random("prfplus long")
    cases = [(hl, _rand(rng, hl), _rand(rng, n), al, 3) for hl in HLS for n in (2047, 2048) for al in range(4)]
    cases += [(hl, bytes([v]) * hl, _rand(rng, 77), 1, 3) for hl in HLS for v in (0x00, 0xFF, 0x36, 0x5C)]
    cases += [(hl, _rand(rng, hl), _rand(rng, 64), 3, 8) for hl in HLS]                                     # eight T(n): the counter byte beyond what KEYMAT needs
    _held(emul, cases)


def test_the_padding_rule_gives_the_block_counts(emul):
    """arithmetic only: the harness's B line is prfp_blocks, held to the rule said another way -- the message, the counter, the 0x80 and the length field, in blocks"""
    script, want = [], []
    for hl in HLS:
        block, field = (64, 8) if hl == 32 else (128, 16)
        for tw in (0, hl // 4):
            for n in list(range(1, 300)) + [2047, 2048]:
                script.append("B %d %d %d" % (hl, tw, n))
                want.append(["b", str(-(-(4 * tw + n + 1 + 1 + field) // block))])
    assert emul(script) == want


def _sa(hl, key, seed, kl):
    (k0, s0), (k1, s1) = IK.child_sa(hl, key, seed, kl)
    return [k0.hex(), s0.hex(), k1.hex(), s1.hex()]


def test_keymat_cut_over_every_hash_and_key_size_and_direction(emul):
    rng = random.Random("prfplus keymat")
    script, want = [], []
    for hl in HLS:
        key, other = _rand(rng, hl), _rand(rng, hl)
        script += ["T %d 5" % hl, "K 3 1 " + key.hex(), "K 0 4 " + other.hex()]
        want += [["k", "ok"], ["k", "ok"]]
        for kl in (16, 24, 32):
            seed = _rand(rng, 64)
            w = _sa(hl, key, seed, kl)
            for a, b, ww in (("0", "3", w), ("-", "3", ["-", "-"] + w[2:]), ("2", "-", w[:2] + ["-", "-"]), ("x", "3", ["-", "-"] + w[2:]), ("1", "x", w[:2] + ["-", "-"])):
                script.append("I %d 4 5 1 %s %s %s" % (kl, a, b, seed.hex()))
                want.append(["i"] + ww)
            for i in range(6):                                               # many Child SAs on one record, each its own nonces; another record in between
                seed = _rand(rng, 32 + 7 * i)
                script.append("I %d 9 %d %d %d %d %s" % (kl, i, 1 if i != 3 else 4, i, 8 - i, seed.hex()))
                want.append(["i"] + _sa(hl, key if i != 3 else other, seed, kl))
        script.append("S")
        want.append(["s", "none"])
    assert emul(script) == want


def test_the_verdict_over_every_refusal_kind(emul):
    one, seed = "11" * 32, "ab" * 40
    script = ["T 32 4", "K 0 0 " + one, "K 1 1 " + one, "K 2 4 " + one, "S",                       # a set_dev index out of range
              "I 16 8 3 4 0 1 " + seed, "I 16 8 2 3 0 1 " + seed, "S",                             # index out of range; unset: the lowest goes to the status word
              "C 1", "I 16 8 9 1 0 1 " + seed, "S",                                                # cleared
              "I 16 8 5 0 8 1 " + seed, "I 16 8 4 0 0 8 " + seed, "I 16 8 6 0 - 8 " + seed, "I 16 8 7 0 8 - " + seed, "S",      # a slot out of range, in either array, alone or not
              "I 16 8 1 0 7 x " + seed, "S",                                                       # the last slot, and none: no refusal
              "I 16 8 12 0 0 1 /100/60", "I 16 8 11 0 0 1 /100/100", "I 16 8 13 0 0 1 /0/2049", "S",       # falling offsets, an empty seed, 2049 bytes
              "I 16 8 3 0 0 1 /7/2055", "I 16 8 2 0 0 1 " + "cd" * 2048, "S"]                      # 2048 bytes at either kind of address: no refusal
    got = emul(script)
    assert got[:4] == [["k", "ok"], ["k", "ok"], ["k", "refused"], ["s", "2"]]
    assert got[4:7] == [["i", "refused"], ["i", "refused"], ["s", "2"]]
    assert got[7:9] == [["i", "refused"], ["s", "9"]]
    assert got[9:14] == [["i", "refused"]] * 4 + [["s", "4"]]
    assert got[14] == ["i"] + _sa(32, bytes.fromhex(one), bytes.fromhex(seed), 16)[:2] + ["-", "-"] and got[15] == ["s", "none"]
    assert got[16:20] == [["i", "refused"]] * 3 + [["s", "11"]]
    assert got[20] == ["i"] + _sa(32, bytes.fromhex(one), bytes(2048), 16) and got[21] == ["i"] + _sa(32, bytes.fromhex(one), b"\xcd" * 2048, 16) and got[22] == ["s", "none"]


# ---------------------------------------------------------------- the kernels' assembly
@pytest.fixture(scope="module")
def census():
    return asm_census("prfplus")


def test_prfplus_kernel_set_has_no_scratch_and_the_recorded_registers(census):
    assert {n.split("(")[0].split("<")[0] for n in census} == {"k_prfp_install", "k_prfp_set"}, sorted(census)
    assert len(census) == 3 * 3 + 1, sorted(census)                           # install: three key sizes x three hashes; set
    assert len([n for n in census if n.startswith("k_prfp_install")]) == 9
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    table = design[design.index("IKEv2 prf+ on the device"):]
    for name, k in census.items():
        assert k["scratch"] == 0, (name, k["scratch"])
        assert k["vgpr"] <= 512, (name, k["vgpr"])                            # the census counts both register files; 512 is what a lane of a 256-lane workgroup can have
    assert "registers " + " / ".join(str(v) for v in sorted({k["vgpr"] for k in census.values()})) in table       # the distinct counts, ascending


def test_prfplus_source_is_a_family_of_its_own_inside_the_prf12_unit():
    others = [f for f in os.listdir(CSRC) if f.endswith("_kernels.hip") and f != "aesgcm_prfplus_kernels.hip"] + ["aesgcm_kernels.hip"]
    assert len(others) >= 13
    for f in others:
        assert "k_prfp_" not in open(os.path.join(CSRC, f)).read(), f
    assert '#include "aesgcm_prfplus_kernels.hip"' in open(os.path.join(CSRC, "aesgcm_device.hip")).read()
    mk = open(os.path.join(CSRC, "Makefile")).read().splitlines()
    assert "prfplus" in [w for ln in mk if ln.startswith("FAMILIES") for w in ln.split()]
    assert "aesgcm_prfplus" not in [w for ln in mk if ln.startswith("UNITS") for w in ln.split()]           # no unit of its own: the host-only test library links a fixed list
    assert open(os.path.join(CSRC, "aesgcm_prf12.hip")).read().rstrip().endswith('#include "aesgcm_prfplus.hip"')
    host = open(os.path.join(CSRC, "aesgcm_prfplus.hip")).read()
    assert host.count("__attribute__((weak)) hipError_t klaunch_prfp_") == 3 and host.count("hipErrorNotSupported") == 3
    for f in ("aesgcm_prfplus.h", "aesgcm_prfplus_kernels.hip"):
        code = "\n".join(ln.split("//")[0] for ln in open(os.path.join(CSRC, f)).read().splitlines())
        assert "atomic" not in code, f                                        # the only atomic is kdf_refuse's, in aesgcm_kdf.h
    note = open(os.path.join(ROOT, "profiles", "prfplus", "isa_unchanged.txt")).read()
    assert "every instruction stream identical: yes" in note and "no scratch" in note
    assert os.path.exists(os.path.join(ROOT, "profiles", "prfplus", "ab.py"))
