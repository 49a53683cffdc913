"""CPU: the C-ABI library builds for gfx950, loads, exports exactly what include/aesgcm.h declares,
and refuses to compute without a GPU (no CPU fallback)."""
import os
import re
import subprocess
import sys

import pytest

import aesgcm_amd  # noqa: F401
from aesgcm_amd import lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "aesgcm.h")


def declared_symbols():
    src = open(HEADER).read()
    return sorted(set(re.findall(r"AESGCM_API\s+[\w \*]+?\b(aesgcm_\w+)\s*\(", src)))


def test_header_and_binding_list_agree():
    assert declared_symbols() == sorted(lib.SYMBOLS)


def test_library_builds_and_exports_every_declared_symbol():
    from aesgcm_amd.build import build, SO
    build()
    out = subprocess.check_output(["nm", "-D", "--defined-only", SO], text=True)
    exported = set(re.findall(r" T (aesgcm_\w+)", out))
    assert exported == set(declared_symbols())
    L = lib.load()
    assert L.aesgcm_abi_version() == lib.ABI_VERSION == 5
    for s in declared_symbols():
        assert hasattr(L, s)


def test_debug_build_is_the_product_plus_one_symbol_and_the_product_reads_no_environment():
    """libaesgcm_hip_dbg.so (-DAESGCM_DEBUG_KNOBS) exports aesgcm_debug_force_shape and nothing else beyond the product's symbols; the product library
    imports no getenv: no environment variable can change which kernel a production caller runs (round-3 verdict, item 6)."""
    from aesgcm_amd.build import build, SO, SO_DEBUG
    build()
    def exported(path):
        return set(re.findall(r" T (aesgcm_\w+)", subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)))
    assert exported(SO_DEBUG) == exported(SO) | {"aesgcm_debug_force_shape"}
    hdr = open(os.path.join(ROOT, "include", "aesgcm_debug.h")).read()
    assert re.findall(r"AESGCM_API\s+[\w \*]+?\b(aesgcm_\w+)\s*\(", hdr) == ["aesgcm_debug_force_shape"]
    for path in (SO, SO_DEBUG):
        undefined = subprocess.check_output(["nm", "-D", "--undefined-only", path], text=True)
        assert not re.search(r"\b(secure_)?getenv\b", undefined), path
    csrc = os.path.join(ROOT, "aes-gcm-128-192-256-bits_amd", "csrc")
    srcs = [f for f in os.listdir(csrc) if f.endswith((".hip", ".h"))]
    assert len(srcs) >= 12
    for src in srcs:
        assert "getenv" not in open(os.path.join(ROOT, "aes-gcm-128-192-256-bits_amd", "csrc", src)).read(), src


def test_code_object_targets_gfx950_only(tmp_path):
    """the library's device code is ONE code object, for gfx950 (the offload bundle is zstd-compressed since round 6 -- 5.6 MB of kernels as 1 MB -- so the bundle's
    entries are listed with the toolchain's own bundler, not grepped)"""
    from aesgcm_amd.build import SO
    llvm = "/opt/rocm/lib/llvm/bin"
    if not (os.path.exists(llvm + "/llvm-objcopy") and os.path.exists(llvm + "/clang-offload-bundler")):
        import pytest
        pytest.skip("no llvm-objcopy / clang-offload-bundler")
    fb = str(tmp_path / "fatbin")
    subprocess.run([llvm + "/llvm-objcopy", "--dump-section", ".hip_fatbin=" + fb, SO, str(tmp_path / "copy.so")], check=True)
    entries = subprocess.check_output([llvm + "/clang-offload-bundler", "--list", "--type=o", "--input=" + fb], text=True).split()
    assert [e for e in entries if not e.startswith("host-")] == ["hipv4-amdgcn-amd-amdhsa--gfx950"], entries
    # (no grep over the library's bytes any more: three bytes like "sm_" turn up in a megabyte of compressed code by chance -- they did in round 6's last build)


def test_strerror_covers_all_codes():
    L = lib.load()
    for code in range(0, -10, -1):
        assert L.aesgcm_strerror(code).decode() not in ("", "unknown error")
    assert L.aesgcm_strerror(-99).decode() == "unknown error"


def test_format_reprs_are_the_recorded_ones():
    """repr() of the six format structs by every constructor: the strings stand in failure messages and logs, and are literals recorded from the commit before
    check() and __repr__ moved into one mixin.  WireFormatX prints its nested WireFormat positionally.  No device, no library."""
    W, X, T, D, S, R = lib.WireFormat, lib.WireFormatX, lib.TlsFormat, lib.DtlsFormat, lib.SrtpFormat, lib.RxFormat
    want = [
        ('W()', 'WireFormat(aad_len=0, hdr_len=0, iv_off=0, salt_len=0, tag_len=0, flags=0)'),
        ('W(1, 2, 3, 4, 5, 6)', 'WireFormat(aad_len=1, hdr_len=2, iv_off=3, salt_len=4, tag_len=5, flags=6)'),
        ('W.macsec()', 'WireFormat(aad_len=28, hdr_len=28, iv_off=16, salt_len=8, tag_len=16, flags=0)'),
        ('W.macsec(sci=False)', 'WireFormat(aad_len=20, hdr_len=20, iv_off=16, salt_len=8, tag_len=16, flags=0)'),
        ('W.macsec(auth_only=True)', 'WireFormat(aad_len=28, hdr_len=28, iv_off=16, salt_len=8, tag_len=16, flags=1)'),
        ('W.macsec(sci=False, auth_only=True)', 'WireFormat(aad_len=20, hdr_len=20, iv_off=16, salt_len=8, tag_len=16, flags=1)'),
        ('W.esp()', 'WireFormat(aad_len=8, hdr_len=16, iv_off=8, salt_len=4, tag_len=16, flags=0)'),
        ('W.esp(12)', 'WireFormat(aad_len=8, hdr_len=16, iv_off=8, salt_len=4, tag_len=12, flags=0)'),
        ('W.esp(tag_len=8)', 'WireFormat(aad_len=8, hdr_len=16, iv_off=8, salt_len=4, tag_len=8, flags=0)'),
        ('X()', 'WireFormatX(WireFormat(aad_len=0, hdr_len=0, iv_off=0, salt_len=0, tag_len=0, flags=0), ext=0, reserved=0)'),
        ('X(W.esp(8), 2, 7)', 'WireFormatX(WireFormat(aad_len=8, hdr_len=16, iv_off=8, salt_len=4, tag_len=8, flags=0), ext=2, reserved=7)'),
        ('X.macsec_xpn()', 'WireFormatX(WireFormat(aad_len=28, hdr_len=28, iv_off=16, salt_len=8, tag_len=16, flags=0), ext=1, reserved=0)'),
        ('X.macsec_xpn(sci=False, auth_only=True)', 'WireFormatX(WireFormat(aad_len=20, hdr_len=20, iv_off=16, salt_len=8, tag_len=16, flags=1), ext=1, reserved=0)'),
        ('X.esp_esn()', 'WireFormatX(WireFormat(aad_len=8, hdr_len=16, iv_off=8, salt_len=4, tag_len=16, flags=0), ext=2, reserved=0)'),
        ('X.esp_esn(12)', 'WireFormatX(WireFormat(aad_len=8, hdr_len=16, iv_off=8, salt_len=4, tag_len=12, flags=0), ext=2, reserved=0)'),
        ('T()', 'TlsFormat(version=0, reserved=0)'),
        ('T.tls13()', 'TlsFormat(version=1, reserved=0)'),
        ('T.tls12()', 'TlsFormat(version=2, reserved=0)'),
        ('T(9, 1)', 'TlsFormat(version=9, reserved=1)'),
        ('D()', 'DtlsFormat(version=0, reserved=0)'),
        ('D.dtls13()', 'DtlsFormat(version=1, reserved=0)'),
        ('D.dtls12()', 'DtlsFormat(version=2, reserved=0)'),
        ('D(9, 1)', 'DtlsFormat(version=9, reserved=1)'),
        ('S()', 'SrtpFormat(kind=0, mki_len=0)'),
        ('S.rtp()', 'SrtpFormat(kind=1, mki_len=0)'),
        ('S.rtp(4)', 'SrtpFormat(kind=1, mki_len=4)'),
        ('S.rtcp()', 'SrtpFormat(kind=2, mki_len=0)'),
        ('S.rtcp(mki_len=128)', 'SrtpFormat(kind=2, mki_len=128)'),
        ('R()', 'RxFormat(rule=0, num_off=0, num_len=0, flags=0)'),
        ('R.macsec()', 'RxFormat(rule=1, num_off=16, num_len=4, flags=0)'),
        ('R.macsec_xpn()', 'RxFormat(rule=2, num_off=16, num_len=4, flags=0)'),
        ('R.esp()', 'RxFormat(rule=1, num_off=4, num_len=4, flags=0)'),
        ('R.esp_esn()', 'RxFormat(rule=2, num_off=4, num_len=4, flags=0)'),
        ('R.dtls12()', 'RxFormat(rule=1, num_off=5, num_len=6, flags=0)'),
        ('R.srtp()', 'RxFormat(rule=3, num_off=2, num_len=2, flags=0)'),
        ('R.srtcp()', 'RxFormat(rule=1, num_off=4, num_len=4, flags=3)'),
        ('R.srtcp(4)', 'RxFormat(rule=1, num_off=8, num_len=4, flags=3)'),
        ('R.expect()', 'RxFormat(rule=4, num_off=0, num_len=0, flags=0)'),
    ]
    assert {c.split("(")[0].split(".")[0] for c, _ in want} == set("WXTDSR")
    for expr, text in want:
        assert repr(eval(expr)) == text, expr


def test_header_compiles_as_plain_c():
    # the boundary is a C ABI: the header must be consumable by gcc -std=c99 with no HIP/C++ types
    code = '#include "aesgcm.h"\nint main(void){return AESGCM_ABI_VERSION==3?0:1;}\n'
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-x", "c", "-", "-fsyntax-only"],
                   input=code.encode(), check=True)


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="a GPU is present")
def test_no_cpu_fallback_without_gpu():
    with pytest.raises(lib.AesGcmError) as e:
        lib.Context(b"k" * 16)
    assert e.value.code == lib.EHIP
    from aesgcm_amd import gcm_model
    with pytest.raises(lib.AesGcmError):
        gcm_model.encrypt(b"k" * 16, b"i" * 12, b"", b"data")
    with pytest.raises(lib.AesGcmError):
        gcm_model.gcm({'data': '00' * 16, 'n_bytes': 16}, {'data': '00' * 12, 'n_bytes': 12}, 'enc')


def test_product_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "aes-gcm-128-192-256-bits_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                txt = open(os.path.join(dirpath, f)).read()
                assert "oracle" not in txt.replace("oracle/aesgcm_oracle.c by definition", ""), f
                assert "libcrypto" not in txt and "Crypto.Cipher" not in txt.replace("from Crypto.Cipher import AES", ""), f


def test_plain_c_caller_builds_and_fails_loudly_without_gpu():
    """examples/kat.c links against the library with nothing but the header; on a box without a HIP device it
    must report AESGCM_EHIP and exit non-zero (no CPU fallback anywhere)."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.run(["make", "-C", os.path.join(root, "examples"), "-s"], check=True)
    r = subprocess.run([os.path.join(root, "examples", "kat")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    if os.path.exists("/dev/kfd"):
        assert r.returncode == 0 and "KAT OK" in r.stdout, r.stderr
    else:
        assert r.returncode != 0 and "-6" in r.stderr, (r.returncode, r.stderr)


def test_oracle_is_only_used_where_allowed():
    """oracle/ is test infrastructure: besides tests/, only __graft_entry__ (build + smoke) and the cpu_baseline leg of
    bench.py may touch it; the package, the examples and the profiling scripts never do."""
    import ast
    import glob
    offenders = []
    files = glob.glob(os.path.join(ROOT, "aes-gcm-128-192-256-bits_amd", "**", "*.py"), recursive=True)
    files += glob.glob(os.path.join(ROOT, "profiles", "**", "*.py"), recursive=True) + [os.path.join(ROOT, "aesgcm_amd.py")]
    for f in files:
        if re.search(r"^\s*(from|import)\s+oracle", open(f).read(), re.M):
            offenders.append(f)
    tree = ast.parse(open(os.path.join(ROOT, "bench.py")).read())
    for node in tree.body:
        inside = node.name if isinstance(node, ast.FunctionDef) else None
        for sub in ast.walk(node):
            if isinstance(sub, (ast.Import, ast.ImportFrom)):
                names = [a.name for a in sub.names] + [getattr(sub, "module", "") or ""]
                if any(n.split(".")[0] == "oracle" for n in names) and inside != "cpu_baseline":
                    offenders.append("bench.py:%s" % (inside or "<module>"))
    for f in glob.glob(os.path.join(ROOT, "examples", "*")) + glob.glob(os.path.join(ROOT, "aes-gcm-128-192-256-bits_amd", "csrc", "*")):
        if os.path.isfile(f) and not f.endswith((".so", ".s")) and b"oracle/" in open(f, "rb").read():
            offenders.append(f)
    assert not offenders, offenders


def test_host_splitmix_matches_the_oracle_generator():
    from aesgcm_amd import sharding
    from oracle import oracle as O
    for seed, n, w in ((0x4B4559, 32, 0), (0x4956, 12, 0), (7, 100, 0), (5, 24, 3)):
        assert sharding.splitmix64_bytes(seed, n, w) == bytes(O.fill_splitmix64(n, seed, w))


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="a GPU is present")
def test_bench_self_launch_fails_loudly_without_gpu():
    """`python bench.py --gpus 2` with no launcher starts two rank processes itself; without a device every rank fails, and the
    parent must exit non-zero and print no bench line (never a silent 1-GPU measurement)"""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "1", "--no-cpu-baseline",
                        "--gib-per-gpu", "0.01", "--launch-timeout", "120"], env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=300)
    assert p.returncode != 0
    assert "{" not in p.stdout
    assert "rank exit codes" in p.stderr
