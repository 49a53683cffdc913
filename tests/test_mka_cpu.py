"""CPU: MACsec's MKA on the device (aesgcm_mka_*: CAKs on the device, the AES-CMAC KDF of IEEE 802.1X-2010 6.2, AES Key Wrap of RFC 3394) without a GPU.  The reference
tests/mka_ref.py is pinned to RFC 4493, SP 800-38B and RFC 3394 and held to libcrypto's own CMAC; the binding and the header name the eight entry points and the ABI
version is still 5; every call refuses its argument errors before it looks at a table or a device; the documents say what they must; the lane code of
csrc/aesgcm_mka.h, run by the CPU harness tests/mka_emul (plain, and under AddressSanitizer and UndefinedBehaviorSanitizer), is held to mka_ref: the inverse cipher
against libcrypto's AES_decrypt, the CMAC at every message length 0 .. 80, the KDF at every context length 1 .. 80, 2047 and 2048 and every start alignment, SAK, KEK and
wrap over the four (cak_len, key_len) pairs, unwrap of a good wrap and of every single-bit corruption of it, and every refusal kind; the gfx950 assembly of the kernels
(`make -C csrc asm_mka`) holds exactly the kernels the design names, none with scratch, with the register counts DESIGN.md records."""
import ctypes
import os
import random
import subprocess

import pytest

import aesgcm_amd  # noqa: F401
from aesgcm_amd import lib

from kt_common import asm_census

import mka_ref as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "aes-gcm-128-192-256-bits_amd", "csrc")
NAMES = ("create", "set", "set_dev", "clear", "install_dev", "unwrap_dev", "status", "destroy")
PAIRS = [(16, 16), (16, 32), (32, 16), (32, 32)]


def _rand(rng, n):
    return rng.getrandbits(8 * n).to_bytes(n, "big") if n else b""


# ---------------------------------------------------------------- the reference
def test_reference_is_pinned_to_the_published_vectors():
    v = M.vectors()
    msg = bytes.fromhex(v["message"])
    assert len(v["cmac"]) == 8 and len(v["wrap"]) == 2
    for c in v["cmac"]:
        key, m = bytes.fromhex(c["key"]), msg[:c["len"]]
        assert M.cmac(key, m).hex() == c["mac"] == M.cmac_libcrypto(key, m).hex(), c["name"]
    for w in v["wrap"]:
        kek, key, wrapped = (bytes.fromhex(w[k]) for k in ("kek", "key", "wrapped"))
        assert M.wrap(kek, key) == wrapped and M.unwrap(kek, wrapped) == key, w["name"]
        bad = bytearray(wrapped)
        bad[11] ^= 4
        assert M.unwrap(kek, bytes(bad)) is None
    f = v["formula_reading"]                                                 # no authority: one reading of the formula, recorded so that a change shows
    assert M.kek(bytes.fromhex(f["cak"]), bytes.fromhex(f["ckn"])).hex() == f["kek"]
    assert M.sak(bytes.fromhex(f["cak"]), bytes.fromhex(f["sak_context"]), 32).hex() == f["sak256"]
    assert bytes.fromhex(f["sak_context"]) == M.sak_context(bytes(32), [bytes(12)], 1) == lib.mka_sak_context(bytes(32), [bytes(12)], 1)


def test_reference_cmac_equals_libcryptos_on_random_keys_and_lengths():
    rng = random.Random("mka cmac")
    for _ in range(300):
        key, m = _rand(rng, rng.choice((16, 32))), _rand(rng, rng.randrange(0, 200))
        assert M.cmac(key, m) == M.cmac_libcrypto(key, m), (len(key), len(m))


# ---------------------------------------------------------------- binding, header, documents
def test_mka_symbols_in_binding_and_header():
    hdr = open(os.path.join(ROOT, "include", "aesgcm.h")).read()
    for n in NAMES:
        assert "aesgcm_mka_" + n in lib.SYMBOLS
        assert "AESGCM_API int aesgcm_mka_%s(" % n in hdr
    assert len([s for s in lib.SYMBOLS if s.startswith("aesgcm_mka_")]) == 8 and "typedef struct aesgcm_mka aesgcm_mka;" in hdr
    assert "#define AESGCM_ABI_VERSION 5 " in hdr and "aesgcm_mka_*" in hdr[hdr.index("#define AESGCM_ABI_VERSION 5 "):hdr.index("5 (round 6)")]
    section = hdr[hdr.index("MACSEC MKA: SAKs from CAKs that never leave the device"):hdr.index("typedef struct aesgcm_mka aesgcm_mka;")]
    for word in ("PROTECT IT\n * LIKE KEYS", "IEEE 802.1X-2010", "RFC 4493", "SP 800-38B", "RFC 3394", "0x01 | Label | 0x00 | Context | be16(Length)", '"IEEE8021 KEK"',
                 '"IEEE8021 SAK"', "zero-padded on the right", "KS-nonce | MI-value list | KN", "A6A6A6A6A6A6A6A6", "key_len + 8", "24 or 40", "1 .. 2048", "does not parse it",
                 "aesgcm_keytab_set_salt", "aesgcm_keytab_set_xpn", "Many entries may name one record", "0 (installed), 1 (refused for what it names) or 2",
                 "MACsec has no AES-192", "n == 0 is AESGCM_OK", "NOTHING an entry names is written", "offsets fall", "empty or longer", "unwrap check fails",
                 "status word is not touched", "NO DERIVED KEY IN MEMORY", "capture-safe", "no scratch memory", "OUT OF SCOPE", "EAP MSK", "ICK", "MKPDUs", "802.1AEbw",
                 "AES-192", "RFC 5649"):
        assert word in section, word
    capture = hdr[hdr.index(" * CAPTURE (key tables"):hdr.index("tests/test_gpu_capture.py replays")]
    assert "aesgcm_mka_install_dev and aesgcm_mka_unwrap_dev" in capture and "aesgcm_mka_create, _set, _set_dev, _clear, _status, _destroy" in capture
    assert capture.index("aesgcm_mka_install_dev") < capture.index("NOT CAPTURE-SAFE") < capture.index("aesgcm_mka_create, _set")
    # the two sentences that said "another feature" point at this table now, the words still in them
    for a, b in (("TLS 1.2 PRF: TLS 1.2 and DTLS 1.2", "typedef struct aesgcm_prf12 aesgcm_prf12;"), ("IKEv2 PRF+: ESP keys of Child SAs", "typedef struct aesgcm_prfplus aesgcm_prfplus;")):
        part = hdr[hdr.index(a):hdr.index(b)]
        assert "aesgcm_mka_*" in part and "MKA KDF" in part and "AES-CMAC" in part and "another feature" not in part, a
    L = lib._mka_typed(lib.load())
    assert L.aesgcm_abi_version() == 5
    assert [len(getattr(L, "aesgcm_mka_" + n).argtypes) for n in NAMES] == [4, 6, 6, 4, 9, 8, 3, 1]
    for m in ("set", "set_dev", "clear", "install_dev", "install", "unwrap_dev", "unwrap", "status", "close", "__enter__", "__exit__"):
        assert callable(getattr(lib.CakTable, m)), m
    assert issubclass(lib.CakTable, lib._Table) and lib.CakTable._prefix == "aesgcm_mka" and callable(lib.mka_sak_context)


def test_documents_say_what_the_issue_asks():
    for doc, words in (("INTEGRATION.md", ("MACsec rekey", "CakTable", "one stream", "refuses at 2^32", "KN + 1", "next AN", "set_salt", "unwrap", "RxWindows")),
                       ("DESIGN.md", ("MACsec MKA on the device", "k_mka_install", "k_mka_unwrap", "k_mka_set", "same lane", "inverse S-box", "InvMixColumns", "run-time",
                                      "test_gpu_mka.py", "test_mka_cpu.py", "aesgcm_prfplus.hip")),
                       ("README.md", ("MACsec MKA", "CakTable", "802.1X's formula", "profiles/mka/ab.py")),
                       (os.path.join("tests", "COVERAGE_mka.md"), ("RFC 4493", "SP 800-38B", "RFC 3394", "formula", "mka_emul", "test_gpu_mka.py", "mka_ref", "OpenSSL 3.0"))):
        text = open(os.path.join(ROOT, doc)).read()
        for w in words:
            assert w in text, (doc, w)


def test_argument_errors_before_any_table_or_device():
    """m = NULL, a table = NULL and placeholder pointers that are never followed: every call returns before it touches a table or a device"""
    L = lib._mka_typed(lib.load())
    P = 16                                                                   # a placeholder pointer

    def inst(m=None, kt=None, n=1, idx=P, ctx=P, off=P, slots=P, wrapped=P):
        return L.aesgcm_mka_install_dev(m, kt, n, idx, ctx, off, slots, wrapped, None)

    def unw(m=None, kt=None, n=1, idx=P, wrapped=P, slots=P, verdict=P):
        return L.aesgcm_mka_unwrap_dev(m, kt, n, idx, wrapped, slots, verdict, None)
    for go in (inst, unw):
        assert go() == lib.EARG and go(m=P) == lib.EARG and go(kt=P) == lib.EARG and go(n=0) == lib.EARG
        assert go(m=P, kt=P, n=0) == lib.OK and go(m=P, kt=P, n=2 ** 31) == lib.EARG
    assert inst(m=P, kt=P, n=0, idx=None, ctx=None, off=None, slots=None, wrapped=None) == lib.OK      # nothing to do: nothing is looked at
    assert unw(m=P, kt=P, n=0, idx=None, wrapped=None, slots=None, verdict=None) == lib.OK
    for missing in ("idx", "ctx", "off", "slots"):
        assert inst(m=P, kt=P, **{missing: None}) == lib.EARG, missing
    for missing in ("idx", "wrapped", "slots"):
        assert unw(m=P, kt=P, **{missing: None}) == lib.EARG, missing
    out = ctypes.c_void_p(5)
    assert L.aesgcm_mka_create(None, 0, 16, 1) == lib.EARG
    for cak_len, n in ((0, 1), (8, 1), (15, 1), (17, 1), (24, 1), (33, 1), (64, 1), (16, 0), (32, 0), (16, 2 ** 31), (32, 2 ** 40)):
        assert L.aesgcm_mka_create(ctypes.byref(out), 0, cak_len, n) == lib.EARG, (cak_len, n)
        assert out.value is None
    one = bytes(32)
    assert L.aesgcm_mka_set(None, 0, 1, one, one, None) == lib.EARG and L.aesgcm_mka_set(None, 0, 0, one, one, None) == lib.EARG
    assert L.aesgcm_mka_set_dev(None, 1, P, P, P, None) == lib.EARG and L.aesgcm_mka_clear(None, 0, 1, None) == lib.EARG
    code = ctypes.c_int(7)
    assert L.aesgcm_mka_status(None, ctypes.byref(code), None) == lib.EARG
    assert L.aesgcm_mka_destroy(None) == lib.OK


# ---------------------------------------------------------------- the lane code on the CPU
@pytest.fixture(scope="module", params=["emul", "emul_asan"])
def emul(request):
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    d = os.path.join(ROOT, "tests", "mka_emul")
    subprocess.run(["make", "-C", d, "-s", request.param], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)

    def run(script):
        out = subprocess.run([os.path.join(d, request.param)], input="\n".join(script) + "\n", stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
        assert out.returncode == 0 and "runtime error" not in out.stdout and "Sanitizer" not in out.stdout and "bad script" not in out.stdout, out.stdout[-3000:]
        return [ln.split() for ln in out.stdout.splitlines()]
    return run


def test_inverse_cipher_equals_libcryptos_at_both_key_sizes(emul):
    rng = random.Random("mka inverse")
    cases = [(_rand(rng, kl), _rand(rng, 16)) for kl in (16, 32) for _ in range(64)]
    cases += [(bytes([v]) * kl, bytes([u]) * 16) for kl in (16, 32) for v in (0x00, 0xFF) for u in (0x00, 0xFF, 0x80)]
    got = emul(["D %s %s" % (k.hex(), b.hex()) for k, b in cases])
    assert got == [["d", M.aes_decrypt(k, b).hex()] for k, b in cases]


def test_cmac_at_every_message_length_to_80(emul):
    """the empty message, every ragged tail, the exact blocks (K1 against K2), one to five blocks, at moving start alignments"""
    rng = random.Random("mka cmac lane")
    cases = [(_rand(rng, kl), _rand(rng, n), (n + kl) % 16) for kl in (16, 32) for n in range(81)]
    got = emul(["M %s %s %d" % (k.hex(), m.hex() or "-", al) for k, m, al in cases])
    assert got == [["m", M.cmac(k, m).hex()] for k, m, al in cases]


@pytest.mark.parametrize("cak_len", [16, 32])
def test_kdf_at_every_context_length_and_alignment(emul, cak_len):
    """lengths 1 .. 80, 2047 and 2048, both output sizes (one and two iterations), both labels; every start alignment 0 .. 15 at the lengths around a block"""
    rng = random.Random("mka kdf %d" % cak_len)
    cases = [(_rand(rng, cak_len), "S", out, _rand(rng, n), (n + out) % 16) for n in list(range(1, 81)) + [2047, 2048] for out in (16, 32)]
    cases += [(_rand(rng, cak_len), which, out, _rand(rng, n), al) for n in (1, 2, 3, 15, 16, 17, 18, 19, 31, 32, 33) for al in range(16) for which, out in (("S", 32), ("K", cak_len))]
    cases += [(_rand(rng, cak_len), "S", 32, _rand(rng, n), al) for n in (2047, 2048) for al in range(16)]
    got = emul(["F %s %s %d %s %d" % (k.hex(), w, out, c.hex(), al) for k, w, out, c, al in cases])
    assert len(got) == len(cases)
    for g, (k, w, out, c, al) in zip(got, cases):
        assert g == ["f", M.kdf(k, M.LABEL_SAK if w == "S" else M.LABEL_KEK, c, 8 * out).hex()], (w, out, len(c), al)


def test_wrap_equals_libcryptos_and_rfc_3394(emul):
    rng = random.Random("mka wrap")
    v = M.vectors()["wrap"]
    cases = [(bytes.fromhex(w["kek"]), bytes.fromhex(w["key"])) for w in v] + [(_rand(rng, a), _rand(rng, b)) for a, b in PAIRS for _ in range(8)]
    got = emul(["W %s %s" % (k.hex(), key.hex()) for k, key in cases])
    assert got == [["w", M.wrap(k, key).hex()] for k, key in cases]
    assert got[0] == ["w", v[0]["wrapped"]] and got[1] == ["w", v[1]["wrapped"]]


@pytest.mark.parametrize("cak_len,key_len", PAIRS)
def test_sak_kek_wrap_and_unwrap_of_every_single_bit_flip(emul, cak_len, key_len):
    """install with and without wrapped output against mka_ref; unwrap of the good wrap installs; the same wrap with each single bit of its key_len + 8 bytes flipped,
    one at a time: every one is refused with verdict 2 and nothing is written"""
    rng = random.Random("mka pair %d %d" % (cak_len, key_len))
    cak, other, ckn = _rand(rng, cak_len), _rand(rng, cak_len), _rand(rng, 1 + key_len // 4)
    ctx = M.sak_context(_rand(rng, key_len), [_rand(rng, 12) for _ in range(3)], 7)
    sak, w = M.sak(cak, ctx, key_len), M.wrapped_sak(cak, ckn, ctx, key_len)
    assert M.unwrap(M.kek(cak, ckn), w) == sak
    script = ["T %d 5" % cak_len, "K 3 1 %s %s" % (cak.hex(), M.keyid(ckn).hex()), "K 0 4 %s %s" % (other.hex(), M.keyid(b"other").hex()),
              "I %d 9 2 1 5 1 %s" % (key_len, ctx.hex()), "I %d 9 6 1 8 0 %s" % (key_len, ctx.hex()), "I %d 9 0 4 0 1 %s" % (key_len, ctx.hex()),
              "U %d 9 3 1 2 1 %s" % (key_len, w.hex()), "U %d 9 0 1 8 0 %s" % (key_len, w.hex()), "S"]
    want = [["k", "ok"], ["k", "ok"], ["i", sak.hex(), w.hex()], ["i", sak.hex(), "-"], ["i", M.sak(other, ctx, key_len).hex(), M.wrapped_sak(other, b"other", ctx, key_len).hex()],
            ["u", "0", sak.hex()], ["u", "-", sak.hex()], ["s", "none"]]
    for bit in range(8 * (key_len + 8)):
        bad = bytearray(w)
        bad[bit // 8] ^= 0x80 >> (bit % 8)
        assert M.unwrap(M.kek(cak, ckn), bytes(bad)) is None
        script.append("U %d 9 %d 1 %d 1 %s" % (key_len, 1 + bit % 5, bit % 9, bad.hex()))
        want.append(["u", "2", "refused", "clean"])
    script += ["S", "U %d 9 4 4 2 1 %s" % (key_len, w.hex()), "S"]            # the other CAK's KEK does not open it
    want += [["s", "1"], ["u", "2", "refused", "clean"], ["s", "4"]]
    assert emul(script) == want


def test_the_verdict_over_every_refusal_kind(emul):
    cak, keyid, ctx = "11" * 16, "22" * 16, "ab" * 40
    w = M.wrapped_sak(bytes.fromhex(cak), bytes.fromhex(keyid), bytes.fromhex(ctx), 16)
    sak = lambda c: M.sak(bytes.fromhex(cak), c, 16).hex()
    wrapped = lambda c: M.wrapped_sak(bytes.fromhex(cak), bytes.fromhex(keyid), c, 16).hex()
    script = ["T 16 4", "K 0 0 %s %s" % (cak, keyid), "K 1 1 %s %s" % (cak, keyid), "K 2 4 %s %s" % (cak, keyid), "S",      # a set_dev index out of range
              "I 16 8 3 4 0 1 " + ctx, "I 16 8 2 3 0 1 " + ctx, "S",                               # index out of range; unset: the lowest goes to the status word
              "C 1", "I 16 8 9 1 0 1 " + ctx, "S",                                                 # cleared
              "I 16 8 5 0 8 1 " + ctx, "I 16 8 4 0 4294967295 1 " + ctx, "S",                      # a slot out of range
              "I 16 8 1 0 7 1 " + ctx, "S",                                                        # the last slot: no refusal
              "I 16 8 12 0 0 1 /100/60", "I 16 8 11 0 0 1 /100/100", "I 16 8 13 0 0 1 /0/2049", "S",       # falling offsets, an empty context, 2049 bytes
              "I 16 8 3 0 0 1 /7/2055", "I 16 8 2 0 0 1 " + "cd" * 2048, "S",                      # 2048 bytes at either kind of address: no refusal
              "U 16 8 6 4 0 1 " + w.hex(), "U 16 8 5 3 0 1 " + w.hex(), "U 16 8 7 1 0 1 " + w.hex(), "U 16 8 8 0 8 1 " + w.hex(), "U 16 8 9 0 8 0 " + w.hex(), "S",
              "U 16 8 2 0 7 1 " + w.hex(), "S"]
    got = emul(script)
    refused = ["i", "refused", "clean"]
    assert got[:4] == [["k", "ok"], ["k", "ok"], ["k", "refused"], ["s", "2"]]
    assert got[4:7] == [refused, refused, ["s", "2"]]
    assert got[7:9] == [refused, ["s", "9"]]
    assert got[9:12] == [refused, refused, ["s", "4"]]
    assert got[12] == ["i", sak(bytes.fromhex(ctx)), wrapped(bytes.fromhex(ctx))] and got[13] == ["s", "none"]
    assert got[14:18] == [refused] * 3 + [["s", "11"]]
    assert got[18] == ["i", sak(bytes(2048)), wrapped(bytes(2048))] and got[19] == ["i", sak(b"\xcd" * 2048), wrapped(b"\xcd" * 2048)] and got[20] == ["s", "none"]
    assert got[21:27] == [["u", "1", "refused", "clean"]] * 4 + [["u", "-", "refused", "clean"], ["s", "5"]]
    assert got[27] == ["u", "0", sak(bytes.fromhex(ctx))] and got[28] == ["s", "none"]


# ---------------------------------------------------------------- the kernels' assembly
@pytest.fixture(scope="module")
def census():
    return asm_census("mka")


def test_mka_kernel_set_has_no_scratch_and_the_recorded_registers(census):
    assert {n.split("(")[0].split("<")[0] for n in census} == {"k_mka_install", "k_mka_unwrap", "k_mka_set"}, sorted(census)
    assert len(census) == 4 + 4 + 1, sorted(census)                           # install and unwrap: two CAK sizes x two SAK sizes; set
    assert len([n for n in census if n.startswith("k_mka_install")]) == 4 and len([n for n in census if n.startswith("k_mka_unwrap")]) == 4
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    table = design[design.index("MACsec MKA on the device"):]
    for name, k in census.items():
        assert k["scratch"] == 0, (name, k["scratch"])
        assert k["vgpr"] <= 256, (name, k["vgpr"])                            # two 256-lane workgroups' LDS fit a CU: two waves per SIMD, 256 registers each
    assert "registers " + " / ".join(str(v) for v in sorted({k["vgpr"] for k in census.values()})) in table       # the distinct counts, ascending


def test_mka_source_is_a_family_of_its_own_inside_the_prf12_unit():
    others = [f for f in os.listdir(CSRC) if f.endswith("_kernels.hip") and f != "aesgcm_mka_kernels.hip"] + ["aesgcm_kernels.hip"]
    assert len(others) >= 14
    for f in others:
        assert "k_mka_" not in open(os.path.join(CSRC, f)).read(), f
    assert '#include "aesgcm_mka_kernels.hip"' in open(os.path.join(CSRC, "aesgcm_device.hip")).read()
    mk = open(os.path.join(CSRC, "Makefile")).read().splitlines()
    assert "mka" in [w for ln in mk if ln.startswith("FAMILIES") for w in ln.split()]
    assert "aesgcm_mka" not in [w for ln in mk if ln.startswith("UNITS") for w in ln.split()]               # no unit of its own: the host-only test library links a fixed list
    assert open(os.path.join(CSRC, "aesgcm_prfplus.hip")).read().rstrip().endswith('#include "aesgcm_mka.hip"')
    host = open(os.path.join(CSRC, "aesgcm_mka.hip")).read()
    assert host.count("__attribute__((weak)) hipError_t klaunch_mka_") == 4 and host.count("hipErrorNotSupported") == 4
    for f in ("aesgcm_mka.h", "aesgcm_mka_kernels.hip"):
        code = "\n".join(ln.split("//")[0] for ln in open(os.path.join(CSRC, f)).read().splitlines())
        assert "atomic" not in code, f                                        # the only atomic is kdf_refuse's, in aesgcm_kdf.h
    note = open(os.path.join(ROOT, "profiles", "mka", "isa_unchanged.txt")).read()
    assert "every instruction stream identical: yes" in note and "no scratch" in note
    assert os.path.exists(os.path.join(ROOT, "profiles", "mka", "ab.py"))
