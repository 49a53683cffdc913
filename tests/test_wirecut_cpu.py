"""CPU: csrc/aesgcm_wirecut.h, what each wire format of the key tables decides about a packet, run on the host by tests/wirecut_emul -- a stand-alone program with its own
main that calls the very functions the kernels call: every cut over seeded packets and the refusal edges of each format against a plain restatement of its rules, the
ranges of the plain wire family as tests/kt_common.py's fixtures state them, and for QUIC and DTLS 1.3 the AEAD kernel's cut against the mask kernel's front tests,
which must give the same verdict on every packet.  Once as it is and once built with the address and undefined-behaviour sanitizers (host code only), where every packet
lies alone in a heap block of its own size.  The header names no kernel, so that the families' sources stay units of their own."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "aes-gcm-128-192-256-bits_amd", "csrc")
EMUL = os.path.join(ROOT, "tests", "wirecut_emul")


def _run(target, exe):
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    subprocess.run(["make", "-C", EMUL, "-s"] + target, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    out = subprocess.run([os.path.join(EMUL, exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    m = re.search(r"^WIRECUT OK (\d+)$", out.stdout, flags=re.M)
    assert out.returncode == 0 and m, out.stdout[-3000:]
    assert int(m.group(1)) > 13 * 3000 + 3 * 3000                             # every format of the plain family, QUIC, DTLS 1.3 and SRTCP over the seeded packets (SRTP's cut is text in the body)
    return out.stdout


def test_cuts_match_the_formats_rules_and_both_kernels_agree():
    _run([], "emul")


def test_cuts_under_address_and_ub_sanitizers():
    if not os.path.exists(os.path.join(EMUL, "asan.mk")):
        pytest.skip("sanitizer recipe not shipped to this machine")
    out = _run(["asan"], "emul_asan")
    assert "ERROR" not in out and "runtime error" not in out, out[-3000:]


def test_the_header_names_no_kernel_and_the_body_no_format():
    hdr = open(os.path.join(CSRC, "aesgcm_wirecut.h")).read()
    assert "k_kt_" not in hdr and "k_batch3" not in hdr
    body = open(os.path.join(CSRC, "aesgcm_batch3_body.inc")).read()
    assert len(body.split("\n")) < 300
    assert body.count("if constexpr (WIREX == KT_WIREX_SRTP)") == 2              # the one format whose cut and nonce stayed text: as functions they moved the block loop
    for word in ("x_quic", "x_d13", "x_srtp", "x_rtcp", "x_esn", "x_xpn", "x_t12", "x_t13", "x_d12"):
        assert word not in body, word
    for call in ("wire_cut<WIREX>(", "wire_nonce<WIREX>(", "wire_aad_block<WIREX>(", "wire_tag_place<WIREX>("):
        assert body.count(call) == 1, call
    # the two mask kernels refuse by the functions the AEAD's cuts call
    for f, words in (("aesgcm_quic_kernels.hip", ("mask_take(q, i, QUIC_TAIL, m)", "quic_pn_bad(")), ("aesgcm_dtls_kernels.hip", ("mask_take(q, i, DTLS13_TAIL, m)", "dtls13_hdr("))):
        src = open(os.path.join(CSRC, f)).read()
        for w in words:
            assert w in src, (f, w)
    assert "wire_front(" in open(os.path.join(CSRC, "aesgcm_mask.h")).read()
