"""CPU: SSH packets in wire format (aesgcm_keytab_ssh_crypt_dev, RFC 5647) and SSH's key derivation on the device (aesgcm_sshkdf_*, RFC 4253 7.2) without a GPU.
The cut and the add-nonce of csrc/aesgcm_wirecut.h run on the host in the stand-alone program tests/sshcut_emul (wirecut_emul's sibling) against tests/ssh_fixture.py; the KDF's lane code of
csrc/aesgcm_sshkdf.h, run by the stand-alone program tests/sshkdf_emul (plain, and its twin under AddressSanitizer and UndefinedBehaviorSanitizer), is held to hashlib
at every secret length 1 .. 300 at every start alignment 0 .. 15, and its verdicts to every refusal kind; the binding and the header name the new symbols, the ABI
version is still 5, and every call refuses its argument errors where the header says so, before it looks at a table or a device; the gfx950 assembly of the two new
families holds exactly the kernels the design names, none with scratch."""
import ctypes
import os
import random
import struct
import subprocess

import pytest

import aesgcm_amd  # noqa: F401
from aesgcm_amd import lib

from kt_common import asm_census, assert_in_budget

import ssh_fixture as SSH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "aes-gcm-128-192-256-bits_amd", "csrc")
NAMES = ("create", "set", "set_dev", "clear", "install_dev", "status", "destroy")
HLS = (32, 48, 64)
EDGES = (1, 55, 56, 63, 64, 111, 112, 119, 120, 127, 128, 129, 300, 2048)


def _rand(rng, n):
    return rng.getrandbits(8 * n).to_bytes(n, "big")


def _make(d, target):
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    subprocess.run(["make", "-C", d, "-s"] + target, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)


def _script(exe, args, script):
    out = subprocess.run([exe] + args, input="\n".join(script) + "\n", stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert out.returncode == 0 and "runtime error" not in out.stdout and "Sanitizer" not in out.stdout and "bad script" not in out.stdout, out.stdout[-3000:]
    return [ln.split() for ln in out.stdout.splitlines()]


# ---------------------------------------------------------------- the cut and the nonce on the host
@pytest.fixture(scope="module", params=["emul", "emul_asan"])
def wirecut(request):
    d = os.path.join(ROOT, "tests", "sshcut_emul")
    _make(d, [request.param])
    exe = os.path.join(d, request.param)
    own = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)      # its own seeded packets and edges against the rule restated
    assert own.returncode == 0 and own.stdout.startswith("SSHCUT OK ") and int(own.stdout.split()[2]) > 3000, own.stdout[-3000:]
    return lambda script: _script(exe, ["script"], script)


def _held_cut(wirecut, cases):
    """cases: (iv, seq, packet)"""
    got = wirecut(["%s %d %s" % (iv.hex(), seq, pkt.hex()) for iv, seq, pkt in cases])
    assert len(got) == len(cases)
    for g, (iv, seq, pkt) in zip(got, cases):
        if SSH.refused(pkt):
            assert g == ["refused"], (len(pkt), pkt[:4].hex())
        else:
            aad, body = SSH.split(pkt)
            assert g == ["ok", str(len(aad)), "4", str(len(body)), SSH.nonce_of(iv, seq).hex()], (len(pkt), iv.hex(), seq)


def test_cut_and_nonce_against_the_fixture(wirecut):
    rng = random.Random("ssh cut")
    cases = [(_rand(rng, 12), rng.getrandbits(64), pkt) for pkt in SSH.make_packets(0x55C0, [16, 32, 48, 112, 128, 144, 1008, 1024, 32768])]
    for n in list(range(1, 70)) + [100, 116, 117, 131, 132]:             # every length around the shortest packet, ragged bodies
        cases.append((_rand(rng, 12), rng.getrandbits(64), _rand(rng, 4) + _rand(rng, max(n - 4, 0)) if n >= 4 else _rand(rng, n)))
        if n >= 20:
            cases.append((_rand(rng, 12), rng.getrandbits(64), struct.pack(">I", n - 20) + _rand(rng, n - 4)))                 # the field right, the length not always
    good = SSH.make_packets(0x55C1, [64])[0]
    for byte in range(4):                                                # a length field that says something else, in every byte
        for bit in (0, 7):
            cases.append((_rand(rng, 12), 5, good[:byte] + bytes([good[byte] ^ (1 << bit)]) + good[byte + 1:]))
    assert sum(not SSH.refused(p) for _, _, p in cases) >= 14 and sum(SSH.refused(p) for _, _, p in cases) >= 70
    _held_cut(wirecut, cases)


def test_counter_carries_and_the_fixed_field(wirecut):
    """the low word's carry and the wrap at 2^64, by the emulation against the fixture and against their values said by hand; an XOR of the same inputs differs"""
    pkt = SSH.make_packets(0x55C2, [16])[0]
    fixed = bytes.fromhex("c0ffee01")
    low, top = fixed + bytes.fromhex("00000000ffffffff"), fixed + bytes.fromhex("fffffffffffffffe")
    cases = [(low, s, pkt) for s in (0, 1, 2)] + [(top, s, pkt) for s in (1, 2, 3)]
    _held_cut(wirecut, cases)
    by_hand = ["00000000ffffffff", "0000000100000000", "0000000100000001", "ffffffffffffffff", "0000000000000000", "0000000000000001"]
    for (iv, seq, _), tail in zip(cases, by_hand):
        assert SSH.nonce_of(iv, seq) == fixed + bytes.fromhex(tail)
    # (seq 0 adds and XORs nothing; FE + 1 = FE ^ 1: the other four are where a carry runs)
    assert [SSH.nonce_of(iv, s) != SSH.nonce_xor(iv, s) for iv, s, _ in cases] == [False, True, True, False, True, True]


# ---------------------------------------------------------------- the KDF's lane code on the host
@pytest.fixture(scope="module", params=["emul", "emul_asan"])
def emul(request):
    d = os.path.join(ROOT, "tests", "sshkdf_emul")
    _make(d, [request.param])
    return lambda script: _script(os.path.join(d, request.param), [], script)


def _held(emul, cases):
    """cases: (hl, secret, sid, align, letter)"""
    got = emul(["H %d %s %s %d %s" % (hl, s.hex(), sid.hex(), al, letter) for hl, s, sid, al, letter in cases])
    assert len(got) == len(cases)
    for g, (hl, s, sid, al, letter) in zip(got, cases):
        assert g == ["h", SSH.kdf(hl, s, sid, letter.encode(), hl).hex()], (hl, len(s), al, letter)


@pytest.mark.parametrize("hl", HLS)
def test_hash_equals_hashlib_at_every_secret_length_and_alignment(emul, hl):
    """every length 1 .. 300 at every start alignment 0 .. 15: the message secret | letter | session_id passes every padding edge of both block sizes, and every
    tail residue mod 4 meets every alignment"""
    rng = random.Random("sshkdf lengths %d" % hl)
    cases = [(hl, _rand(rng, n), _rand(rng, hl), al, "ABCD"[(n + al) % 4]) for n in range(1, 301) for al in range(16)]
    assert len(cases) == 4800
    _held(emul, cases)


def test_hash_at_the_longest_secrets_and_the_block_counts(emul):
    rng = random.Random("sshkdf long")
    _held(emul, [(hl, _rand(rng, n), _rand(rng, hl), al, letter) for hl in HLS for n in (2047, 2048) for al in (0, 1, 15) for letter in "AD"])
    script, want = [], []
    for hl in HLS:
        block, field = (64, 8) if hl == 32 else (128, 16)
        for n in list(range(1, 300)) + [2047, 2048]:
            script.append("B %d %d" % (hl, n))
            want.append(["b", str(-(-(n + 1 + hl + 1 + field) // block))])
    assert emul(script) == want


def _inst(hl, secret, sid, kl):
    (k0, i0), (k1, i1) = SSH.derive(hl, secret, sid, kl)
    return [k0.hex(), i0.hex(), k1.hex(), i1.hex()]


def test_records_and_install_over_every_hash_key_size_direction_and_padding_edge(emul):
    rng = random.Random("sshkdf install")
    script, want = [], []
    for hl in HLS:
        script.append("T %d 2048 %d" % (hl, len(EDGES) + 1))
        recs = []
        for r, n in enumerate(EDGES):
            secret, sid = _rand(rng, n), _rand(rng, hl)
            recs.append((secret, sid))
            script.append("K %d %d %s %s" % (r % 5, r, secret.hex(), sid.hex()))
            want.append(["k", "ok"])
        for r, (secret, sid) in enumerate(recs):
            kl = (16, 24, 32)[r % 3]
            w = _inst(hl, secret, sid, kl)
            a, b, ww = [("0", "3", w), ("-", "3", ["-", "-"] + w[2:]), ("2", "-", w[:2] + ["-", "-"]), ("x", "3", ["-", "-"] + w[2:]), ("1", "x", w[:2] + ["-", "-"])][r % 5]
            script.append("I %d 4 %d %d %s %s" % (kl, r, r, a, b))
            want.append(["i"] + ww)
        # a re-exchange: a new K | H under the same session identifier gives other keys
        secret2 = _rand(rng, 77)
        script += ["K 0 3 %s %s" % (secret2.hex(), recs[3][1].hex()), "I 32 4 0 3 0 1", "S"]
        want += [["k", "ok"], ["i"] + _inst(hl, secret2, recs[3][1], 32), ["s", "none"]]
    assert emul(script) == want


def test_the_verdict_over_every_refusal_kind(emul):
    one, sid = "11" * 40, "22" * 32
    script = ["T 32 100 4", "K 0 0 %s %s" % (one, sid), "K 1 1 %s %s" % (one, sid), "K 2 4 %s %s" % (one, sid), "S",      # a set_dev index out of range
              "K 3 2 /50/50 " + sid, "K 4 2 /50/40 " + sid, "K 5 2 /0/101 " + sid, "S", "K 0 2 /7/107 " + sid, "S",      # empty, falling, too long; the longest: no refusal
              "I 16 8 3 4 0 1", "I 16 8 2 3 0 1", "S",                          # index out of range; unset: the lowest goes to the status word
              "C 1", "I 16 8 9 1 0 1", "S",                                     # cleared
              "I 16 8 5 0 8 1", "I 16 8 4 0 0 8", "I 16 8 6 0 - 8", "I 16 8 7 0 8 -", "S",      # a slot out of range, in either array, alone or not
              "I 16 8 1 0 7 x", "S"]                                            # the last slot, and none: no refusal
    got = emul(script)
    assert got[:4] == [["k", "ok"], ["k", "ok"], ["k", "refused"], ["s", "2"]]
    assert got[4:10] == [["k", "refused"]] * 3 + [["s", "3"], ["k", "ok"], ["s", "none"]]
    assert got[10:13] == [["i", "refused"], ["i", "refused"], ["s", "2"]]
    assert got[13:15] == [["i", "refused"], ["s", "9"]]
    assert got[15:20] == [["i", "refused"]] * 4 + [["s", "4"]]
    assert got[20] == ["i"] + _inst(32, bytes.fromhex(one), bytes.fromhex(sid), 16)[:2] + ["-", "-"] and got[21] == ["s", "none"]


# ---------------------------------------------------------------- binding, header, argument errors
def test_symbols_in_binding_and_header():
    hdr = open(os.path.join(ROOT, "include", "aesgcm.h")).read()
    assert "aesgcm_keytab_ssh_crypt_dev" in lib.SYMBOLS and "AESGCM_API int aesgcm_keytab_ssh_crypt_dev(" in hdr
    for n in NAMES:
        assert "aesgcm_sshkdf_" + n in lib.SYMBOLS
        assert "AESGCM_API int aesgcm_sshkdf_%s(" % n in hdr
    assert len([s for s in lib.SYMBOLS if s.startswith("aesgcm_sshkdf_")]) == 7 and "typedef struct aesgcm_sshkdf aesgcm_sshkdf;" in hdr
    version = hdr[hdr.index("#define AESGCM_ABI_VERSION 5 "):hdr.index("5 (round 6)")]
    assert "aesgcm_keytab_ssh_crypt_dev" in version and "aesgcm_sshkdf_*" in version
    L = lib._sshkdf_typed(lib._keytab_typed(lib.load()))
    assert L.aesgcm_abi_version() == 5
    for n in ["aesgcm_keytab_ssh_crypt_dev"] + ["aesgcm_sshkdf_" + n for n in NAMES]:
        assert getattr(L, n) is not None, n                                  # the library exports every one
    assert [len(getattr(L, "aesgcm_sshkdf_" + n).argtypes) for n in NAMES] == [5, 7, 7, 4, 7, 3, 1] and len(L.aesgcm_keytab_ssh_crypt_dev.argtypes) == 10
    for m in ("set", "set_dev", "clear", "install_dev", "install", "status", "close", "__enter__", "__exit__"):
        assert callable(getattr(lib.SshKexTable, m)), m
    assert issubclass(lib.SshKexTable, lib._Table) and lib.SshKexTable._prefix == "aesgcm_sshkdf"
    assert callable(lib.KeyTable.crypt_ssh) and callable(lib.KeyTable.ssh_crypt_dev)


def test_argument_errors_before_any_table_or_device():
    """placeholder pointers that are never followed: every call returns before it touches a table or a device"""
    L = lib._sshkdf_typed(lib._keytab_typed(lib.load()))
    P = 16

    def crypt(t=P, dec=0, n=1, slots=P, seq=P, i=P, off=P, o=P, auth=P):
        return L.aesgcm_keytab_ssh_crypt_dev(t, dec, n, slots, seq, i, off, o, auth, None)
    assert crypt(seq=None) == lib.EARG and crypt(t=None, seq=None) == lib.EARG and crypt(seq=None, n=0) == lib.EARG      # d_seq first, as the TLS call
    assert crypt(t=None) == lib.EARG and crypt(dec=2) == lib.EARG and crypt(n=0) == lib.OK
    for missing in ("slots", "i", "off", "o"):
        assert crypt(**{missing: None}) == lib.EARG, missing
    assert crypt(dec=1, auth=None) == lib.EARG and crypt(n=2 ** 31) == lib.EARG

    def go(p=None, kt=None, n=1, idx=P, a=P, b=P):
        return L.aesgcm_sshkdf_install_dev(p, kt, n, idx, a, b, None)
    assert go() == lib.EARG and go(p=P) == lib.EARG and go(kt=P) == lib.EARG and go(n=0) == lib.EARG
    assert go(p=P, kt=P, n=0) == lib.OK and go(p=P, kt=P, n=0, idx=None, a=None, b=None) == lib.OK
    assert go(p=P, kt=P, idx=None) == lib.EARG and go(p=P, kt=P, a=None, b=None) == lib.EARG and go(p=P, kt=P, n=2 ** 31) == lib.EARG
    out = ctypes.c_void_p(5)
    assert L.aesgcm_sshkdf_create(None, 0, 32, 64, 1) == lib.EARG
    for hash_len, mx, n in ((0, 64, 1), (16, 64, 1), (20, 64, 1), (33, 64, 1), (65, 64, 1), (32, 0, 1), (48, 2049, 1), (64, 2 ** 40, 1), (32, 64, 0), (64, 64, 2 ** 31)):
        assert L.aesgcm_sshkdf_create(ctypes.byref(out), 0, hash_len, mx, n) == lib.EARG, (hash_len, mx, n)
        assert out.value is None
    one, off = bytes(64), struct.pack("<2I", 0, 40)
    assert L.aesgcm_sshkdf_set(None, 0, 1, one, off, one, None) == lib.EARG and L.aesgcm_sshkdf_set(None, 0, 0, one, off, one, None) == lib.EARG
    assert L.aesgcm_sshkdf_set_dev(None, 1, P, P, P, P, None) == lib.EARG and L.aesgcm_sshkdf_clear(None, 0, 1, None) == lib.EARG
    code = ctypes.c_int(7)
    assert L.aesgcm_sshkdf_status(None, ctypes.byref(code), None) == lib.EARG
    assert L.aesgcm_sshkdf_destroy(None) == lib.OK


def test_documents_say_what_is_checked_against_what():
    for doc, words in (("INTEGRATION.md", ("SSH packets", "SshKexTable", "crypt_ssh", "TxCounters", "no replay window", "packet boundaries", "re-exchange")),
                       ("DESIGN.md", ("cut_ssh", "nonce_iv_add_num", "k_kt_ssh", "k_sshk_install", "test_gpu_ssh.py", "test_ssh_cpu.py", "NOT BUILT")),
                       ("README.md", ("SSH packets", "crypt_ssh", "SshKexTable", "profiles/ssh/ab.py")),
                       (os.path.join("tests", "COVERAGE_ssh.md"), ("RFC 5647", "RFC 4253", "OpenSSH", "formulas", "hashlib", "libcrypto", "sshkdf_emul"))):
        text = open(os.path.join(ROOT, doc)).read()
        for w in words:
            assert w in text, (doc, w)
    assert "pinned" not in open(os.path.join(ROOT, "tests", "COVERAGE_ssh.md")).read().replace("not pinned", "")


# ---------------------------------------------------------------- the kernels' assembly
def test_ssh_kernels_scratch_free_and_in_budget():
    census = asm_census("ssh")
    assert {n.split("(")[0].split("<")[0] for n in census} == {"k_kt_ssh"} and len(census) == 18, sorted(census)
    assert_in_budget(census)
    for f in os.listdir(CSRC):
        if f.endswith("_kernels.hip") and f != "aesgcm_ssh_kernels.hip" or f == "aesgcm_kernels.hip":
            assert "k_kt_ssh" not in open(os.path.join(CSRC, f)).read(), f
    assert '#include "aesgcm_ssh_kernels.hip"' in open(os.path.join(CSRC, "aesgcm_device.hip")).read()


def test_sshkdf_kernel_set_has_no_scratch():
    census = asm_census("sshkdf")
    assert {n.split("(")[0].split("<")[0] for n in census} == {"k_sshk_install", "k_sshk_set"}, sorted(census)
    assert len(census) == 3 * 3 + 1, sorted(census)                           # install: three key sizes x three hashes; set
    for name, k in census.items():
        assert k["scratch"] == 0, (name, k["scratch"])
    mk = open(os.path.join(CSRC, "Makefile")).read().splitlines()
    fam = [w for ln in mk if ln.startswith("FAMILIES") for w in ln.split()]
    assert "ssh" in fam and "sshkdf" in fam and "aesgcm_sshkdf" not in [w for ln in mk if ln.startswith("UNITS") for w in ln.split()]
    assert open(os.path.join(CSRC, "aesgcm_mka.hip")).read().rstrip().endswith('#include "aesgcm_sshkdf.hip"')
