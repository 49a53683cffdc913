"""CPU: csrc/aesgcm_dispatch.h, which turns a launch's run-time arguments (rounds, mode or decrypt, lanes per packet, form) into the template arguments of the kernel
instance that runs it, for every launcher of the library.  A stand-alone C++17 program built with the host compiler against that header alone -- no HIP header, no GPU
library, no device -- prints what it was handed: for every input exactly one call with the constants of the fall-through rules (or the refusal), every instance set
with its size, and the stop of a walk at the first error.  The launchers of aesgcm_kernels.hip call the very functions checked here."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "aes-gcm-128-192-256-bits_amd", "csrc")

NRS, DECS, LGS = (10, 12, 14, 0, 11, 16), (0, 1, 3), (3, 4, 6, 0, 5, 7)

PROGRAM = r"""
#include "aesgcm_dispatch.h"
#include <cstdio>

enum { ENC = 0, DEC = 1, KS = 2, ECB = 3, PROBE = 4 };          // the caller's mode constants: the header takes them as template arguments

template <int... Vs> void prim(const char *name, klist<Vs...> l) {
    for (int v = -1; v <= 10; v++) {
        int calls = 0;
        const int back = pick(l, v, [&](auto V) { calls++; return 1000 + V(); });
        std::printf("pick %s %d -> %d %d\n", name, v, calls, back);
    }
    for (int fail_at = 0; fail_at <= (int)sizeof...(Vs); fail_at++) {       // 0: never
        int seen = 0;
        std::printf("walk %s-%d visits", name, fail_at);
        const int e = each(l, [&](auto V) { seen++; std::printf(" %d", (int)V()); return seen == fail_at ? 800 + V() : 0; });
        std::printf(" returned %d\n", e);
    }
}

int main() {
    const int nrs[] = {10, 12, 14, 0, 11, 16}, decs[] = {0, 1, 3}, lgs[] = {3, 4, 6, 0, 5, 7};
    for (int nr : nrs) for (int dec : decs) for (int lg : lgs) {
        int calls = 0;
        batch3_dispatch(nr, dec, lg, [&](auto NR, auto D, auto LG) {
            static_assert(NR() == 10 || NR() == 12 || NR() == 14, "compile-time constants");
            calls++;
            std::printf("dispatch %d %d %d -> %d %d %d\n", nr, dec, lg, NR(), D(), LG());
        });
        std::printf("calls %d\n", calls);
        const int back = batch3_dispatch(nr, dec, lg, [](auto NR, auto D, auto LG) { return 10000 * NR() + 100 * D() + LG(); });      // f's value comes back
        std::printf("value %d\n", back);
    }
    for (int nr : nrs) std::printf("nr %d -> %d\n", nr, nr_dispatch(nr, [](auto NR) { return (int)NR(); }));
    for (int fail_at = 0; fail_at <= 18; fail_at++) {           // 0: never
        int seen = 0;
        const int e = batch3_each([&](auto NR, auto D, auto LG) {
            seen++;
            if (!fail_at) std::printf("each %d %d %d\n", NR(), D(), LG());
            return seen == fail_at ? 700 + seen : 0;
        });
        std::printf("each_fail %d seen %d returned %d\n", fail_at, seen, e);
    }
    for (int fail_at = 0; fail_at <= 3; fail_at++) {
        int seen = 0;
        const int e = nr_each([&](auto NR) { seen++; return seen == fail_at ? 900 + (int)NR() : 0; });
        std::printf("nr_each_fail %d seen %d returned %d\n", fail_at, seen, e);
    }
    // the wire families' sets: the body kernels with a two-valued variant (here 1, 2), and the two mask kernels
    const int vs[] = {1, 2, 0, 3};
    for (int nr : nrs) for (int dec : decs) for (int lg : lgs) for (int v : vs) {
        int calls = 0;
        const int back = batch3v_dispatch<1, 2>(nr, dec, lg, v, [&](auto NR, auto D, auto LG, auto V) { calls++; return 100000 * NR() + 1000 * D() + 10 * LG() + V(); });
        std::printf("b3v %d %d %d %d -> %d %d\n", nr, dec, lg, v, calls, back);
    }
    for (int nr : nrs) for (int dec : decs) {
        int calls = 0;
        const int back = mask_dispatch(nr, dec, [&](auto NR, auto D) { calls++; return 100 * NR() + D(); });
        std::printf("mask %d %d -> %d %d\n", nr, dec, calls, back);
    }
    for (int fail_at = 0; fail_at <= 37; fail_at++) {
        int seen = 0;
        const int e = batch3v_each<1, 2>([&](auto NR, auto D, auto LG, auto V) { seen++; if (!fail_at) std::printf("b3v_each %d %d %d %d\n", NR(), D(), LG(), V()); return seen == fail_at ? 600 + seen : 0; });
        std::printf("b3v_fail %d seen %d returned %d\n", fail_at, seen, e);
        seen = 0;
        const int em = mask_each([&](auto NR, auto D) { seen++; if (!fail_at) std::printf("mask_each %d %d\n", NR(), D()); return seen == fail_at ? 600 + seen : 0; });
        std::printf("mask_fail %d seen %d returned %d\n", fail_at, seen, em);
    }
    prim("p2", klist<7, 9>{});
    prim("p3", klist<3, 4, 6>{});
    prim("p4", klist<2, 3, 4, 6>{});
    const int modes[] = {ENC, DEC, KS, ECB, PROBE, -1, 9}, dec4[] = {0, 1, 2, 3}, lg7[] = {2, 3, 4, 6, 0, 5, 7};
    for (int nr : nrs) for (int mode : modes) {
        int calls = 0;
        const int back = set_pick(main_set<ENC, DEC, KS, ECB>{}, [&](auto NR, auto M) { calls++; return 100 * NR() + M(); }, nr, mode);
        std::printf("main %d %d -> %d %d %d\n", nr, mode, calls, back / 100, back % 100);
        for (int cyc = 0; cyc < 2; cyc++) for (int half = 0; half < 2; half++) {
            calls = 0;
            body_dispatch<ENC, DEC, PROBE>(nr, mode, cyc, half, [&](auto NR, auto M, auto FORM) { calls++; std::printf("body %d %d %d %d -> %d %d %d", nr, mode, cyc, half, NR(), M(), FORM()); });
            std::printf(" %d\n", calls);
        }
    }
    for (int nr : nrs) for (int dec : dec4) for (int sc = 0; sc < 2; sc++) {
        for (int ilp = 0; ilp < 2; ilp++) {
            int calls = 0;
            std::printf("pktl %d %d %d %d -> ", nr, dec, ilp, sc);
            const bool ok = pktl_dispatch(nr, dec, ilp, sc, [&](auto NR, auto D, auto ILP, auto S) { calls++; std::printf("%d %d %d %d ", NR(), D(), ILP(), S()); });
            std::printf("%s %d\n", ok ? "ok" : "refused", calls);
        }
        for (int lg : lg7) {
            int calls = 0;
            std::printf("pktg %d %d %d %d -> ", nr, dec, lg, sc);
            const bool ok = pktg_dispatch(nr, dec, lg, sc, [&](auto NR, auto D, auto LG, auto S) { calls++; std::printf("%d %d %d %d ", NR(), D(), LG(), S()); });
            std::printf("%s %d\n", ok ? "ok" : "refused", calls);
        }
        if (!sc) std::printf("rows %d %d -> %d\n", nr, dec, rows_dispatch<ENC, DEC>(nr, dec, [](auto NR, auto M) { return 100 * NR() + M(); }));
    }
    // the sets the attribute setters walk, and a walk that fails at its k-th instance (0: never)
    for (int fail_at = 0; fail_at <= 48; fail_at++) {
        int seen = 0;
        const auto visit = [&](const char *set, int a, int b, int c, int d) { seen++; if (!fail_at) std::printf("set %s %d %d %d %d\n", set, a, b, c, d); return seen == fail_at ? 500 + seen : 0; };
        if (!fail_at) {
            set_each(main_set<ENC, DEC, KS, ECB>{}, [&](auto NR, auto M) { return visit("main", NR(), M(), 0, 0); });
            set_each(rows_set<ENC, DEC>{}, [&](auto NR, auto M) { return visit("rows", NR(), M(), 0, 0); });
        }
        seen = 0;
        const int eb = body_each<ENC, DEC, PROBE>([&](auto NR, auto M, auto FORM) { return visit("body", NR(), M(), FORM(), 0); });
        std::printf("set_fail body %d seen %d returned %d\n", fail_at, seen, eb);
        seen = 0;
        const int el = pktl_each([&](auto NR, auto D, auto ILP, auto S) { return visit("pktl", NR(), D(), ILP(), S()); });
        std::printf("set_fail pktl %d seen %d returned %d\n", fail_at, seen, el);
        seen = 0;
        const int eg = pktg_each([&](auto NR, auto D, auto LG, auto S) { return visit("pktg", NR(), D(), LG(), S()); });
        std::printf("set_fail pktg %d seen %d returned %d\n", fail_at, seen, eg);
    }
    return 0;
}
"""


def _rule_nr(nr):
    return nr if nr in (10, 12) else 14


def _rule(nr, dec, lg):
    return _rule_nr(nr), 0 if dec == 0 else 1, lg if lg in (3, 4) else 6


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("dispatch")
    src, exe = str(d / "dispatch_check.cpp"), str(d / "dispatch_check")
    with open(src, "w") as f:
        f.write(PROGRAM)
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-O1", "-I", CSRC, "-o", exe, src], check=True)
    return subprocess.run([exe], check=True, stdout=subprocess.PIPE, text=True).stdout.split("\n")


def test_header_needs_no_hip():
    text = open(os.path.join(CSRC, "aesgcm_dispatch.h")).read()
    includes = [ln.split()[1] for ln in text.split("\n") if ln.startswith("#include")]
    assert includes == ["<type_traits>"], includes


def test_every_input_reaches_exactly_one_instance(lines):
    got = [tuple(int(x) for x in ln.replace("->", "").split()[1:]) for ln in lines if ln.startswith("dispatch ")]
    want = [(nr, dec, lg) + _rule(nr, dec, lg) for nr in NRS for dec in DECS for lg in LGS]
    assert got == want                                                       # one line per input, in the loop's order, with the rules' constants
    assert [ln for ln in lines if ln.startswith("calls ")] == ["calls 1"] * len(want)
    values = [int(ln.split()[1]) for ln in lines if ln.startswith("value ")]
    assert values == [10000 * a + 100 * b + c for a, b, c in (_rule(*w[:3]) for w in want)]
    assert {w[3:] for w in want} == {(nr, dec, lg) for nr in (10, 12, 14) for dec in (0, 1) for lg in (3, 4, 6)}      # the inputs reach all 18


def test_nr_alone(lines):
    got = [tuple(int(x) for x in ln.replace("->", "").split()[1:]) for ln in lines if ln.startswith("nr ")]
    assert got == [(nr, _rule_nr(nr)) for nr in NRS]


def test_each_visits_18_instances_once_and_stops_at_the_first_error(lines):
    seen = [tuple(int(x) for x in ln.split()[1:]) for ln in lines if ln.startswith("each ")]
    assert len(seen) == 18 and set(seen) == {(nr, dec, lg) for nr in (10, 12, 14) for dec in (0, 1) for lg in (3, 4, 6)}
    fails = [tuple(int(x) for x in ln.split()[1::2]) for ln in lines if ln.startswith("each_fail ")]
    assert fails == [(0, 18, 0)] + [(k, k, 700 + k) for k in range(1, 19)]   # (fail_at, calls made, value returned)
    nr_fails = [tuple(int(x) for x in ln.split()[1::2]) for ln in lines if ln.startswith("nr_each_fail ")]
    assert nr_fails == [(0, 3, 0), (1, 1, 910), (2, 2, 912), (3, 3, 914)]


def test_wire_family_sets(lines):
    """the body kernels with a variant (k_kt_wirex, k_kt_tls, k_kt_dtls, k_kt_srtp: 36 instances) and the two mask kernels (6): every input reaches exactly one instance by
    the fall-through rules -- a variant that is not the first lands on the second, which is why the launchers refuse an unknown one first -- and the walks visit every
    instance once and stop at the first error"""
    got = [_ints(ln) for ln in lines if ln.startswith("b3v ")]
    want = []
    for nr in NRS:
        for dec in DECS:
            for lg in LGS:
                for v in (1, 2, 0, 3):
                    a, b, c = _rule(nr, dec, lg)
                    want.append([nr, dec, lg, v, 1, 100000 * a + 1000 * b + 10 * c + (1 if v == 1 else 2)])
    assert got == want
    got = [_ints(ln) for ln in lines if ln.startswith("mask ")]
    assert got == [[nr, dec, 1, 100 * _rule_nr(nr) + (0 if dec == 0 else 1)] for nr in NRS for dec in DECS]
    seen = [tuple(_ints(ln)) for ln in lines if ln.startswith("b3v_each ")]
    assert len(seen) == 36 and set(seen) == {(nr, d, lg, v) for nr in (10, 12, 14) for d in (0, 1) for lg in (3, 4, 6) for v in (1, 2)}
    seen = [tuple(_ints(ln)) for ln in lines if ln.startswith("mask_each ")]
    assert len(seen) == 6 and set(seen) == {(nr, d) for nr in (10, 12, 14) for d in (0, 1)}
    for name, size in (("b3v", 36), ("mask", 6)):
        fails = [_ints(ln) for ln in lines if ln.startswith("%s_fail " % name)]
        assert fails == [[k, size if k == 0 or k > size else k, 0 if k == 0 or k > size else 600 + k] for k in range(0, 38)], name


# ---- the two primitives, and the compositions the launchers of aesgcm_kernels.hip use (the rules: what those launchers did as macro ladders)
ENC, DEC, KS, ECB, PROBE = 0, 1, 2, 3, 4
MODES, DEC4, LG7 = (ENC, DEC, KS, ECB, PROBE, -1, 9), (0, 1, 2, 3), (2, 3, 4, 6, 0, 5, 7)
BODY_DEALT, BODY_CYC, BODY_HALF = 0, 1, 2


def _ints(ln):
    return [int(x) for x in ln.replace("->", " ").split() if x.lstrip("-").isdigit()]


@pytest.mark.parametrize("name,values", [("p2", (7, 9)), ("p3", (3, 4, 6)), ("p4", (2, 3, 4, 6))])
def test_primitives(lines, name, values):
    got = [_ints(ln) for ln in lines if ln.startswith("pick %s " % name)]
    assert got == [[v, 1, 1000 + (v if v in values else values[-1])] for v in range(-1, 11)]           # one call; the first equal constant, else the last; f's value comes back
    walks = [ln for ln in lines if ln.startswith("walk %s-" % name)]
    want = ["walk %s-0 visits %s returned 0" % (name, " ".join(map(str, values)))]                       # every constant once, in order
    want += ["walk %s-%d visits %s returned %d" % (name, k, " ".join(map(str, values[:k])), 800 + values[k - 1]) for k in range(1, len(values) + 1)]
    assert walks == want


def test_main_and_rows_rules(lines):
    got = [_ints(ln) for ln in lines if ln.startswith("main ")]
    assert got == [[nr, mode, 1, _rule_nr(nr), mode if mode in (ENC, DEC, KS) else ECB] for nr in NRS for mode in MODES]
    got = [_ints(ln) for ln in lines if ln.startswith("rows ")]
    assert got == [[nr, dec, 100 * _rule_nr(nr) + (DEC if dec else ENC)] for nr in NRS for dec in DEC4]


def test_body_rules(lines):
    def rule(mode, cyc, half):
        if half:
            return DEC if mode == DEC else ENC, BODY_HALF
        if cyc:
            return DEC if mode == DEC else ENC, BODY_CYC
        return mode if mode in (DEC, PROBE) else ENC, BODY_DEALT
    got = [_ints(ln) for ln in lines if ln.startswith("body ")]
    assert got == [[nr, mode, cyc, half, _rule_nr(nr), *rule(mode, cyc, half), 1] for nr in NRS for mode in MODES for cyc in (0, 1) for half in (0, 1)]


def _pkt(lines, kind):
    """-> [(inputs, instance or None)]: a refusal calls nothing"""
    out = []
    for ln in lines:
        if ln.startswith(kind + " "):
            left, right = ln.split("->")
            r = right.split()
            assert (r[-2], r[-1]) in (("ok", "1"), ("refused", "0")), ln
            out.append((tuple(_ints(left)), tuple(int(x) for x in r[:-2]) if r[-2] == "ok" else None))
    return out


def test_pktl_rules(lines):
    def rule(nr, dec, ilp, sc):
        if sc:
            return _rule_nr(nr), 1 if dec else 0, 0, 1                       # k_pktls: a dec of 2 lands on 1, ilp is ignored
        if dec == 2:
            return None if ilp else (_rule_nr(nr), 2, 0, 0)                  # the probe has no ILP form: refused
        return _rule_nr(nr), 1 if dec else 0, ilp, 0
    assert _pkt(lines, "pktl") == [((nr, dec, ilp, sc), rule(nr, dec, ilp, sc)) for nr in NRS for dec in DEC4 for sc in (0, 1) for ilp in (0, 1)]


def test_pktg_rules(lines):
    def rule(nr, dec, lg, sc):
        small = lg in (2, 3, 4)
        if sc:
            return (_rule_nr(nr), 1 if dec else 0, lg, 1) if small else None
        if dec == 2:
            return (_rule_nr(nr), 2, lg, 0) if small else None
        return _rule_nr(nr), 1 if dec else 0, lg if small else 6, 0
    assert _pkt(lines, "pktg") == [((nr, dec, lg, sc), rule(nr, dec, lg, sc)) for nr in NRS for dec in DEC4 for sc in (0, 1) for lg in LG7]


def test_instance_sets(lines):
    """what klaunch_set_attributes walks: k_main 12, k_body 15, k_bodyh 6, k_rows 6, k_pktg 24 + 9 probes, k_pktl 12 + 3 probes, k_pktgs 18, k_pktls 6; nothing twice"""
    sets = {}
    for ln in lines:
        if ln.startswith("set ") and not ln.startswith("set_fail"):
            sets.setdefault(ln.split()[1], []).append(tuple(_ints(ln)))
    for name, members in sets.items():
        assert len(set(members)) == len(members), name
    nrs = (10, 12, 14)
    assert set(sets["main"]) == {(nr, m, 0, 0) for nr in nrs for m in (ENC, DEC, KS, ECB)} and len(sets["main"]) == 12
    assert set(sets["rows"]) == {(nr, m, 0, 0) for nr in nrs for m in (ENC, DEC)} and len(sets["rows"]) == 6
    body = [m for m in sets["body"] if m[2] != BODY_HALF]
    assert set(body) == {(nr, m, BODY_DEALT, 0) for nr in nrs for m in (ENC, DEC, PROBE)} | {(nr, m, BODY_CYC, 0) for nr in nrs for m in (ENC, DEC)} and len(body) == 15
    bodyh = [m for m in sets["body"] if m[2] == BODY_HALF]
    assert set(bodyh) == {(nr, m, BODY_HALF, 0) for nr in nrs for m in (ENC, DEC)} and len(bodyh) == 6
    pktg = [m for m in sets["pktg"] if not m[3]]
    assert set(pktg) == {(nr, d, lg, 0) for nr in nrs for d in (0, 1) for lg in (2, 3, 4, 6)} | {(nr, 2, lg, 0) for nr in nrs for lg in (2, 3, 4)} and len(pktg) == 33
    pktl = [m for m in sets["pktl"] if not m[3]]
    assert set(pktl) == {(nr, d, i, 0) for nr in nrs for d in (0, 1) for i in (0, 1)} | {(nr, 2, 0, 0) for nr in nrs} and len(pktl) == 15
    pktgs = [m for m in sets["pktg"] if m[3]]
    assert set(pktgs) == {(nr, d, lg, 1) for nr in nrs for d in (0, 1) for lg in (2, 3, 4)} and len(pktgs) == 18
    pktls = [m for m in sets["pktl"] if m[3]]
    assert set(pktls) == {(nr, d, 0, 1) for nr in nrs for d in (0, 1)} and len(pktls) == 6


def test_set_walks_stop_at_the_first_error(lines):
    for name, size in (("body", 21), ("pktl", 21), ("pktg", 51)):
        fails = [_ints(ln) for ln in lines if ln.startswith("set_fail %s " % name)]
        assert fails == [[k, size if k == 0 or k > size else k, 0 if k == 0 or k > size else 500 + k] for k in range(0, 49)], name      # (fail_at, calls made, value returned)
