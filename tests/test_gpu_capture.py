"""GPU: key-table and receive-window calls under hipStreamBeginCapture, replayed as graphs (include/aesgcm.h, CAPTURE).

Every case has one shape: an ordinary warm-up call; the same call captured on a created stream (tests/hip_graph.py) and instantiated; three replays, and between replays
OTHER packets are uploaded into the SAME device buffers -- other lengths, offsets, slots, numbers and bytes, the same n and the same pointers.  Every replay's whole
output arena (canary bytes in front and behind), d_auth, the decoded numbers and status() are compared with the family fixture's reference over libcrypto (kt_common,
quic_fixture, dtls_fixture, srtp_fixture, tls_fixture) -- never with a direct call of the library.  The three references of a case differ from one another (asserted), so a
graph that baked in what it saw at capture time cannot pass.

CAPTURE MODE: thread-local (hipStreamCaptureModeThreadLocal), the strictest mode in which the uploads that the other tests' threads might make stay legal; every captured
graph is a single-stream chain (no fork, no parallel branches), and no environment variable of the runtime is set.  A HIP call that fails ends the test with the code
in its message, and tests/hip_graph.py starts nothing more after it.

Key tables (encrypt and decrypt, one tag in seven forged on decrypt; about 300 packets with payloads of 0 .. 272 bytes byte-packed behind a lead of 0 .. 15 bytes; the lane-group
shapes 8, 16 and 64 forced through the debug library; the key size rotating over the cases): macsec, esn16, tls13, quic (two launches), dtls13 (two launches, the decoded
numbers out), dtls12, srtp with a 4-byte MKI, srtcp with E set and E clear in one call, the five-array crypt_dev with offset arrays, and one graph that holds two calls
behind one another on different buffers.  One case runs macsec and srtp with batch_order forced: a captured call is never ordered, and must still be right.

The receive loop in ONE graph (the flows, the three batches and their reference: tests/rx_loop.py, shared with tests/test_gpu_rxwin_grid.py): recover_dev, the family's decrypt out of place, commit_dev with d_accept = d_auth and d_why, wipe_failed_dev.  Replay 1: fresh reordered
traffic with loss, duplicates inside the call and forged tags.  Replay 2: the same input again -- every packet that still authenticates is a REPLAY (the reference says so
itself, asserted), the state is unchanged, every output byte zero.  Replay 3: the next batch from where the reference window stands, with numbers at next - W - 1, next - W,
next - 1, next + W - 1, next + W and one far enough ahead to clear the whole ring.  After each: d_num / d_hi against rxwin_ref.recover, d_why through
rxwin_ref.same_verdicts against the sequential Window, rw.get() against the reference's normalised state, the outputs against the fixture's plaintext for accepted packets
and zeros for the rest, rw.status() and kt.status().  State travels from replay to replay through device memory alone.

test_perturbed_references_are_reported holds the comparisons themselves to account: a payload byte, a tag, a verdict, a window's next, and replay 2's reference swapped for
replay 1's are each reported."""
import random
import struct

import pytest

import dtls_fixture as D
import hip_graph as G
import kt_common as KC
import quic_fixture as Q
import rxwin_ref as R
import srtp_fixture as S
import tls_fixture as T
from kt_common import _u32, _u64, evp  # noqa: F401
from rx_loop import CANARY, N, POISON, RTP_HEADERS, TAG, _arena, _lengths, _offsets, loop_reference, loop_same
from util import splitmix_bytes

pytestmark = pytest.mark.gpu

KEY_LENS = (16, 24, 32)
LANES = (8, 16, 64)
N_SLOTS, N_HP = 11, 5
FAMILIES = ("macsec", "esn16", "tls13", "quic", "dtls13", "dtls12", "srtp", "srtcp", "crypt5")
TRAIL = {"srtp": 4, "srtcp": 4}


class Variant:
    """one set of packets of a family: what goes up for encrypt / decrypt (name -> bytes) and what must come down (name -> bytes)"""


class Ref:
    """a family under one key size: what the slots hold and three variants, from the fixtures alone"""


_REFS = {}


def reference(hip, evp, fam, key_len):
    if (fam, key_len) in _REFS:
        return _REFS[fam, key_len]
    r = Ref()
    r.fam, r.key_len = fam, key_len
    seed = 0x4CA90000 + 4096 * FAMILIES.index(fam) + key_len
    r.keys = splitmix_bytes(seed, key_len * (N_SLOTS + N_HP))
    r.sa = KC.Sa(N_SLOTS + N_HP, seed + 1)
    ib = splitmix_bytes(seed + 4, 12 * (N_SLOTS + N_HP))
    r.ivs = [ib[12 * s:12 * s + 12] for s in range(N_SLOTS + N_HP)]
    r.variants = [_variant(hip, evp, r, k, seed + 16 * (k + 1)) for k in range(3)]
    r.size = max(len(v.frames_bytes) for v in r.variants) + 64
    for a in range(3):
        for b in range(a + 1, 3):
            for dec in (0, 1):
                va, vb = r.variants[a], r.variants[b]
                assert all(va.want[dec][k] != vb.want[dec][k] for k in va.want[dec]) and va.up[dec]["off"] != vb.up[dec]["off"] and va.up[dec]["slots"] != vb.up[dec]["slots"], (fam, a, b)
    _REFS[fam, key_len] = r
    return r


def _variant(hip, evp, r, k, seed):
    fam, kl = r.fam, r.key_len
    rng = random.Random(seed)
    key = lambda s: r.keys[kl * s:kl * (s + 1)]
    n, lens = N, _lengths(rng, N)
    slots = [rng.randrange(N_SLOTS) for _ in range(n)]
    hps = [N_SLOTS + rng.randrange(N_HP) for _ in range(n)]
    blob = splitmix_bytes(seed + 1, 400 * n)
    fill = lambda i: blob[400 * i:400 * i + 400]
    v = Variant()
    v.lead = (5 * k + 3) % 16
    up, pn_out, extra_dec = {"slots": _u32(slots)}, None, {}
    tr = TRAIL.get(fam, 0)
    if fam == "crypt5":
        ivs = [fill(i)[:12] for i in range(n)]
        aads = [fill(i)[16:16 + rng.randrange(41)] for i in range(n)]
        datas = [fill(i)[100:100 + L] for i, L in enumerate(lens)]
        enc = KC.evp_by_slot(evp, kl, r.keys, slots, list(zip(ivs, aads, datas)), [d + TAG for d in datas], 16)
        cts, tags = [e[:-16] for e in enc], [e[-16:] for e in enc]
        forged = [(i + k) % 7 == 3 for i in range(n)]
        exp = [bytes([t[0] ^ (1 << (i % 8))]) + t[1:] if f else t for i, (t, f) in enumerate(zip(tags, forged))]
        aoff = _offsets(aads, 0)
        common = dict(up, ivs=b"".join(ivs), aad=b"".join(aads) or b"\0", aoff=_u64(aoff))
        v.frames_bytes = b"".join(datas)
        off = _offsets(datas, v.lead)
        v.up = [dict(common, off=_u64(off), **{"in": (datas,)}), dict(common, off=_u64(off), exp=b"".join(exp), **{"in": (cts,)})]
        v.want = [{"out": (cts,), "tags": b"".join(tags)}, {"out": (datas,), "tags": b"".join(tags), "auth": struct.pack("<%di" % n, *[0 if f else 1 for f in forged])}]
        v.auth = [0 if f else 1 for f in forged]
        return v
    if fam == "macsec":
        fmt = hip.WireFormat.macsec()
        plain = [fill(i)[:28] + fill(i)[100:100 + L] + TAG for i, L in enumerate(lens)]
        enc = KC.wire_ref_encrypt(evp, kl, r.keys, r.sa.salt, fmt, slots, plain)
    elif fam == "esn16":
        xf = hip.WireFormatX.esp_esn(16)
        his = [rng.getrandbits(32) for _ in range(n)]
        his[0], his[1] = 0, 2 ** 32 - 1
        up["hi"] = _u32(his)
        plain = [fill(i)[:16] + fill(i)[100:100 + L] + TAG for i, L in enumerate(lens)]
        enc = KC.x_ref_encrypt(evp, kl, r.keys, r.sa, xf, slots, his, plain)
    elif fam == "tls13":
        seqs = [rng.getrandbits(64) for _ in range(n)]
        seqs[0], seqs[1] = 0, 2 ** 64 - 1
        up["num"] = _u64(seqs)
        plain = [fill(i)[:5] + fill(i)[100:100 + L] + TAG for i, L in enumerate(lens)]
        enc = KC.tls_ref_encrypt(evp, kl, r.keys, r.ivs, T.TLS13, slots, seqs, plain)
    elif fam == "quic":
        pls = [4 if L < 3 else 1 + i % 4 for i, L in enumerate(lens)]
        pns = [rng.getrandbits((8, 16, 31, 33, 62)[i % 5]) for i in range(n)]
        pns[0], pns[1] = 0, 2 ** 62 - 1
        exps = [max(0, pn - rng.randrange(min((1 << (8 * pl - 1)) - 1, 100) + 1)) for pn, pl in zip(pns, pls)]
        up.update(hp=_u32(hps), pn_off=_u32([9] * n), num=_u64(pns))
        extra_dec = {"num": _u64(exps)}
        plain = [bytes([(0xC0 if i % 5 in (1, 4) else 0x40) | (pl - 1)]) + fill(i)[:8] + (pn & ((1 << 8 * pl) - 1)).to_bytes(pl, "big") + fill(i)[100:100 + L] + TAG
                 for i, (L, pl, pn) in enumerate(zip(lens, pls, pns))]
        enc = [Q.protect(key(s), r.ivs[s], key(h), pn, 9, p) for s, h, pn, p in zip(slots, hps, pns, plain)]
        opened = lambda i, b: Q.unprotect(key(slots[i]), r.ivs[slots[i]], key(hps[i]), exps[i], 9, b)
    elif fam == "dtls13":
        cids = [fill(i)[:(0, 1, 7, 20)[i % 4]] for i in range(n)]
        s16 = [bool(i % 3) for i in range(n)]
        seqs = [rng.getrandbits((8, 16, 31, 33, 48, 64)[i % 6]) for i in range(n)]
        seqs[0], seqs[1] = 0, 2 ** 64 - 1
        exps = [max(0, q - rng.randrange(min((1 << (15 if s else 7)) - 1, 100) + 1)) for q, s in zip(seqs, s16)]
        sn_off = [1 + len(c) for c in cids]
        up.update(hp=_u32(hps), pn_off=_u32(sn_off), num=_u64(seqs))
        extra_dec = {"num": _u64(exps)}
        plain = [D.header13(cids[i], seqs[i], s16[i], i % 5 in (1, 4), i & 3, L + 16) + fill(i)[100:100 + L] + TAG for i, L in enumerate(lens)]
        enc = [D.protect13(key(slots[i]), r.ivs[slots[i]], key(hps[i]), seqs[i], sn_off[i], plain[i]) for i in range(n)]
        opened = lambda i, b: D.unprotect13(key(slots[i]), r.ivs[slots[i]], key(hps[i]), exps[i], sn_off[i], b)
    elif fam == "dtls12":
        plain = [D.header12(23, i & 0xFFFF, rng.getrandbits(48), L) + fill(i)[:8] + fill(i)[100:100 + L] + TAG for i, L in enumerate(lens)]
        enc = [D.protect12(key(s), r.ivs[s], p) for s, p in zip(slots, plain)]
        opened = lambda i, b: D.unprotect12(key(slots[i]), r.ivs[slots[i]], b)
    elif fam == "srtp":
        rocs = [rng.getrandbits((1, 16, 32)[i % 3]) for i in range(n)]
        rocs[0], rocs[1] = 0, 2 ** 32 - 1
        up["hi"] = _u32(rocs)
        plain = [S.rtp_header(RTP_HEADERS[i % 6][0], RTP_HEADERS[i % 6][1], rng.getrandbits(16), rng.getrandbits(32), rng.getrandbits(32), fill(i)) + fill(i)[300:300 + L]
                 + TAG + fill(i)[396:400] for i, L in enumerate(lens)]
        enc = [S.protect_rtp(key(s), r.ivs[s], roc, p, 4) for s, roc, p in zip(slots, rocs, plain)]
        opened = lambda i, b: S.unprotect_rtp(key(slots[i]), r.ivs[slots[i]], rocs[i], b, 4)
    else:                                                                       # srtcp: E set and E clear in one call
        plain = [bytes([0x80 | (fill(i)[0] & 0x3F)]) + fill(i)[1:8] + fill(i)[100:100 + L] + TAG + struct.pack(">I", ((i + k) % 2) << 31 | rng.getrandbits(31)) for i, L in enumerate(lens)]
        enc = [S.protect_rtcp(key(s), r.ivs[s], p, 0) for s, p in zip(slots, plain)]
        opened = lambda i, b: S.unprotect_rtcp(key(slots[i]), r.ivs[slots[i]], b, 0)
    assert [len(e) for e in enc] == [len(p) for p in plain]
    forged = [(i + k) % 7 == 3 for i in range(n)]
    bad = []
    for i, e in enumerate(enc):
        b = bytearray(e)
        if forged[i]:
            b[len(e) - tr - 16 + i % 16] ^= 1 << (i % 8)
        bad.append(bytes(b))
    if fam in ("macsec", "esn16", "tls13"):
        dec = [p[:len(p) - 16] + b[len(b) - 16:] for p, b in zip(plain, bad)]
        auth = [0 if f else 1 for f in forged]
    else:
        res = [opened(i, b) for i, b in enumerate(bad)]
        dec, auth = [x[0] for x in res], [int(bool(x[-1])) for x in res]
        assert auth == [0 if f else 1 for f in forged]
        if len(res[0]) == 3:
            pn_out = [x[1] for x in res]
    off = _u64(_offsets(plain, v.lead))
    v.frames_bytes = b"".join(plain)
    v.up = [dict(up, off=off, **{"in": (plain,)}), dict(up, off=off, **extra_dec, **{"in": (bad,)})]
    v.want = [{"out": (enc,)}, {"out": (dec,), "auth": struct.pack("<%di" % n, *auth)}]
    if pn_out is not None:
        v.want[1]["pn_out"] = _u64(pn_out)
    v.auth = auth
    return v


def table(hip, r):
    kt = hip.KeyTable(r.key_len, N_SLOTS + N_HP)
    kt.set(0, r.keys)
    if r.fam == "macsec":
        kt.set_salt(0, b"".join(r.sa.salt))
    elif r.fam == "esn16":
        kt.set_salt(0, b"".join(r.sa.salt))
        kt.set_xpn(0, b"".join(r.sa.xsalt), b"".join(r.sa.ssci))
    elif r.fam != "crypt5":
        kt.set_tls_iv(0, b"".join(r.ivs))
    return kt


class Job:
    """one call of a family on device buffers of its own: the same pointers for every variant"""

    def __init__(self, hip, r, dec):
        self.hip, self.r, self.dec = hip, r, dec
        self.kt = table(hip, r)
        sizes = {}
        for v in r.variants:
            for k, b in list(v.up[dec].items()) + list(v.want[dec].items()):
                sizes[k] = max(sizes.get(k, 16), r.size if isinstance(b, tuple) else len(b))
        self.B = {k: hip.DeviceBuffer(nb) for k, nb in sizes.items()}

    def load(self, k):
        v = self.r.variants[k]
        for name, b in v.up[self.dec].items():
            self.B[name].upload(_arena(b[0], v.lead, self.r.size) if isinstance(b, tuple) else b)
        for name, b in v.want[self.dec].items():
            self.B[name].upload(bytes([CANARY if isinstance(b, tuple) else POISON]) * self.B[name].nbytes)

    def enqueue(self, st=None):
        hip, kt, dec, fam, n = self.hip, self.kt, self.dec, self.r.fam, N
        p = lambda k: self.B[k].ptr
        a = p("auth") if dec else None
        if fam == "macsec":
            kt.frames_crypt_dev(dec, hip.WireFormat.macsec(), n, p("slots"), p("in"), p("off"), p("out"), d_auth=a, stream=st)
        elif fam == "esn16":
            kt.frames_crypt_x_dev(dec, hip.WireFormatX.esp_esn(16), n, p("slots"), p("hi"), p("in"), p("off"), p("out"), d_auth=a, stream=st)
        elif fam == "tls13":
            kt.records_crypt_dev(dec, hip.TlsFormat.tls13(), n, p("slots"), p("num"), p("in"), p("off"), p("out"), d_auth=a, stream=st)
        elif fam == "quic":
            kt.quic_crypt_dev(dec, n, p("slots"), p("hp"), p("num"), p("pn_off"), p("in"), p("off"), p("out"), d_pn_out=p("pn_out") if dec else None, d_auth=a, stream=st)
        elif fam == "dtls13":
            kt.dtls_crypt_dev(dec, hip.DtlsFormat.dtls13(), n, p("slots"), p("in"), p("off"), p("out"), d_sn_slots=p("hp"), d_seq=p("num"), d_sn_off=p("pn_off"),
                              d_seq_out=p("pn_out") if dec else None, d_auth=a, stream=st)
        elif fam == "dtls12":
            kt.dtls_crypt_dev(dec, hip.DtlsFormat.dtls12(), n, p("slots"), p("in"), p("off"), p("out"), d_auth=a, stream=st)
        elif fam == "srtp":
            kt.srtp_crypt_dev(dec, hip.SrtpFormat.rtp(4), n, p("slots"), p("in"), p("off"), p("out"), d_roc=p("hi"), d_auth=a, stream=st)
        elif fam == "srtcp":
            kt.srtp_crypt_dev(dec, hip.SrtpFormat.rtcp(0), n, p("slots"), p("in"), p("off"), p("out"), d_auth=a, stream=st)
        else:
            kt.crypt_dev(dec, n, p("slots"), p("ivs"), p("in"), p("off"), p("out"), p("tags"), d_aad=p("aad"), d_aad_off=p("aoff"), d_expect_tags=p("exp") if dec else None,
                         d_auth=a, stream=st)

    def read(self):
        got = {name: bytes(self.B[name].download()) for name in self.r.variants[0].want[self.dec]}
        got["status"] = self.kt.status()
        return got

    def want(self, k):
        v = self.r.variants[k]
        w = {name: _arena(b[0], v.lead, self.r.size) if isinstance(b, tuple) else b for name, b in v.want[self.dec].items()}
        w["status"] = (self.hip.OK, 0)
        return w

    def close(self):
        self.kt.close()
        for b in self.B.values():
            b.free()


def same(got, want, label):
    """every output of a replay against its reference: the whole arena, canaries included"""
    for name, w in want.items():
        g = got[name] if name == "status" else got[name][:len(w)]
        if g != w:
            at = next(i for i, (x, y) in enumerate(zip(g, w)) if x != y) if name != "status" else 0
            raise AssertionError("%s: %s differs from the reference at %s %d: got %r, want %r" % (label, name, "entry" if name in ("auth", "pn_out") else "byte", at // (4 if name == "auth" else 8 if name == "pn_out" else 1),
                                                                                            g[at:at + 8] if name != "status" else g, w[at:at + 8] if name != "status" else w))
        if name != "status" and len(got[name]) > len(w):
            assert set(got[name][len(w):]) <= {CANARY if name == "out" else POISON}, (label, name, "bytes behind the array were written")


def replays(jobs, label):
    """warm-up, capture, three replays over other packets in the same buffers -> [[what each job read] per replay]"""
    hip = jobs[0].hip
    for j in jobs:
        j.load(0)
        j.enqueue()                                                             # the ordinary call on this device, with this table and key size
    hip.dev_sync()
    st = G.stream_create()
    out = []
    with G.Graph(st, lambda: [j.enqueue(st) for j in jobs]) as g:
        assert g.nodes >= 2 * len(jobs), (label, g.nodes)                       # the dispenser's memset node and the launch, per call
        for k in range(3):
            for j in jobs:
                j.load(k)
            g.launch()
            out.append([j.read() for j in jobs])
    G.stream_destroy(st)
    return out


def run_case(hip, evp, fams, dec, lanes, key_len, order=0):
    refs = [reference(hip, evp, f, key_len) for f in fams]
    label = "%s %s lanes %d AES-%d" % ("+".join(fams), "dec" if dec else "enc", lanes, 8 * key_len)
    with hip.debug_library() as dbg:
        dbg.force(batch_lanes=lanes, batch_order=order)
        jobs = [Job(hip, r, dec) for r in refs]
        try:
            got = replays(jobs, label)
            for k in range(3):
                for j, g in zip(jobs, got[k]):
                    same(g, j.want(k), "%s, replay %d" % (label, k + 1))
            return jobs, got
        finally:
            for j in jobs:
                j.close()


CASES = [(f, dec, lanes, KEY_LENS[(i + dec + LANES.index(lanes)) % 3]) for i, f in enumerate(FAMILIES) for dec in (0, 1) for lanes in LANES]


@pytest.mark.parametrize("fam, dec, lanes, key_len", CASES)
def test_key_table_call_replayed_over_other_packets(hip, evp, fam, dec, lanes, key_len):  # noqa: F811
    run_case(hip, evp, [fam], dec, lanes, key_len)


@pytest.mark.parametrize("dec, lanes, key_len", [(0, 8, 32), (1, 16, 16)])
def test_two_calls_in_one_graph(hip, evp, dec, lanes, key_len):  # noqa: F811
    """two calls behind one another on the stream, each with a table and buffers of its own (and a dispenser of its own): both right in every replay"""
    run_case(hip, evp, ["macsec", "dtls13"], dec, lanes, key_len)


@pytest.mark.parametrize("fam, lanes, key_len", [("macsec", 8, 24), ("srtp", 16, 32)])
def test_ordered_call_is_captured_in_array_order(hip, evp, fam, lanes, key_len):  # noqa: F811
    """batch_order forced: an ordinary call is ordered by falling length class (the warm-up is), a captured one never (aesgcm_host.hip, batch_plan: no order slot, event,
    allocation or sort under capture).  Encrypt and decrypt must be the reference's either way"""
    for dec in (0, 1):
        run_case(hip, evp, [fam], dec, lanes, key_len, order=1)


def test_the_cases_cover_what_they_claim():
    assert {(f, d) for f, d, _, _ in CASES} == {(f, d) for f in FAMILIES for d in (0, 1)} and len(CASES) == len(set(CASES)) == 6 * len(FAMILIES)
    for f in FAMILIES:
        assert {l for ff, _, l, _ in CASES if ff == f} == set(LANES) and {k for ff, _, _, k in CASES if ff == f} == set(KEY_LENS)


# ---------------------------------------------------------------- the receive loop in one graph (the flows, the three batches and loop_same: tests/rx_loop.py)
def run_loop(hip, name, W, key_len, lanes):
    flow, starts, batches = loop_reference(hip, name, W, key_len)
    n, size = N, max(b.off[-1] for b in batches) + 64
    label = "receive loop %s W=%d lanes %d" % (name, W, lanes)
    with hip.debug_library() as dbg:
        dbg.force(batch_lanes=lanes)
        kt, rw = flow.table(hip), hip.RxWindows(flow.n_wins, W)
        B = {k: hip.DeviceBuffer(nb) for k, nb in dict(win=4 * n, slots=4 * n, hp=4 * n, off=8 * (n + 1), sn_off=4 * n, num=8 * n, hi=4 * n, pn_out=8 * n, auth=4 * n, why=4 * n).items()}
        B["in"], B["out"] = hip.DeviceBuffer(size), hip.DeviceBuffer(size)
        p = lambda k: B[k].ptr
        expect = name in ("quic", "dtls13")

        def load(b):
            B["win"].upload(_u32(b.wins)); B["slots"].upload(_u32([flow.slot(w) for w in b.wins])); B["hp"].upload(_u32([flow.n_wins + w for w in b.wins]))
            B["off"].upload(_u64(b.off)); B["sn_off"].upload(_u32(b.sn_off)); B["in"].upload(_arena(b.pkts, b.lead, size)); B["out"].upload(bytes([CANARY]) * size)
            for k in ("num", "hi", "pn_out", "auth", "why"):
                B[k].upload(bytes([POISON]) * B[k].nbytes)

        def enqueue(st=None):
            rw.recover_dev(flow.fmt, n, p("win"), None if expect else p("in"), None if expect else p("off"), p("num"), p("hi"), stream=st)
            if name == "esn":
                kt.frames_crypt_x_dev(1, hip.WireFormatX.esp_esn(16), n, p("slots"), p("hi"), p("in"), p("off"), p("out"), d_auth=p("auth"), stream=st)
            elif name == "srtp":
                kt.srtp_crypt_dev(1, hip.SrtpFormat.rtp(), n, p("slots"), p("in"), p("off"), p("out"), d_roc=p("hi"), d_auth=p("auth"), stream=st)
            elif name == "srtcp":
                kt.srtp_crypt_dev(1, hip.SrtpFormat.rtcp(0), n, p("slots"), p("in"), p("off"), p("out"), d_auth=p("auth"), stream=st)
            elif name == "quic":
                kt.quic_crypt_dev(1, n, p("slots"), p("hp"), p("num"), p("sn_off"), p("in"), p("off"), p("out"), d_pn_out=p("pn_out"), d_auth=p("auth"), stream=st)
            else:
                kt.dtls_crypt_dev(1, hip.DtlsFormat.dtls13(), n, p("slots"), p("in"), p("off"), p("out"), d_sn_slots=p("hp"), d_seq=p("num"), d_sn_off=p("sn_off"), d_seq_out=p("pn_out"),
                                  d_auth=p("auth"), stream=st)
            rw.commit_dev(n, p("win"), p("pn_out") if expect else p("num"), p("auth"), p("auth"), p("why"), stream=st)
            hip.wipe_failed_dev(n, p("out"), p("auth"), d_data_off=p("off"), stream=st)

        try:
            # the ordinary call first, on windows that are then put where the reference starts
            load(batches[0])
            rw.set(0, starts)
            enqueue()
            hip.dev_sync()
            kt.status(), rw.status()
            rw.set(0, starts)
            hip.dev_sync()
            st = G.stream_create()
            got = []
            with G.Graph(st, lambda: enqueue(st)) as g:
                for b in batches:
                    load(b)
                    g.launch()
                    d = lambda k, code: list(struct.unpack("<%d%s" % (n, code), bytes(B[k].download(n * struct.calcsize("<" + code)))))
                    got.append(dict(num=d("num", "Q"), hi=d("hi", "I"), why=d("why", "i"), accept=d("auth", "i"), out=bytes(B["out"].download()), state=rw.get(),
                                    status=(rw.status(), kt.status())))
            G.stream_destroy(st)
        finally:
            kt.close(); rw.close()
            for x in B.values():
                x.free()
    return flow, batches, got, size, label


LOOPS = [("esn", 1024, 16, 8), ("esn", 64, 24, 16), ("srtp", 1024, 32, 16), ("srtp", 64, 16, 8), ("quic", 64, 24, 8), ("quic", 1024, 32, 64), ("dtls13", 1024, 16, 16), ("dtls13", 64, 32, 8),
         ("srtcp", 64, 16, 64), ("srtcp", 1024, 24, 8)]


@pytest.mark.parametrize("name, W, key_len, lanes", LOOPS)
def test_receive_loop_in_one_graph(hip, name, W, key_len, lanes):
    flow, batches, got, size, label = run_loop(hip, name, W, key_len, lanes)
    for k, (b, g) in enumerate(zip(batches, got)):
        loop_same(hip, flow, b, g, size, "%s, replay %d" % (label, k + 1))
    assert set(got[1]["out"][batches[1].lead:batches[1].off[-1]]) == {0}          # replay 2: every output byte zero
    assert got[1]["state"] == got[0]["state"] and got[2]["state"] != got[1]["state"]


def test_perturbed_references_are_reported(hip, evp):  # noqa: F811
    """the comparisons fail when the reference is wrong by one payload byte, one tag byte, one verdict, one window's next, or when replay 2 is held to replay 1's"""
    jobs, got = run_case(hip, evp, ["macsec"], 1, 8, 16)
    j = jobs[0]
    v = j.r.variants[0]
    t = v.lead + len(v.want[1]["out"][0][0])                                     # one byte behind the first frame's end: inside its tag / the next frame

    def flipped(w, name, at):
        w = dict(w)
        w[name] = w[name][:at] + bytes([w[name][at] ^ 1]) + w[name][at + 1:]
        return w
    for what, w in (("a payload byte", flipped(j.want(0), "out", v.lead + 30)), ("a tag byte", flipped(j.want(0), "out", t - 1)), ("a verdict", flipped(j.want(0), "auth", 8))):
        with pytest.raises(AssertionError):
            same(got[0][0], w, what)
    with pytest.raises(AssertionError):
        same(got[1][0], j.want(0), "replay 2 against replay 1's reference")
    same(got[1][0], j.want(1), "replay 2")
    flow, batches, lg, size, label = run_loop(hip, "esn", 1024, 16, 8)
    import copy
    for what, change in (("a verdict", lambda b: b.why.__setitem__(b.why.index(R.ACCEPT), R.REPLAY)), ("a window's next", lambda b: b.state.__setitem__(1, (b.state[1][0] + 1, b.state[1][1] << 1))),
                         ("a recovered number", lambda b: b.rec.__setitem__(4, (b.rec[4][0] + 2 ** 32, b.rec[4][1] + 1))), ("a payload byte", lambda b: b.plain.__setitem__(
                             b.why.index(R.ACCEPT), bytes([b.plain[b.why.index(R.ACCEPT)][0] ^ 1]) + b.plain[b.why.index(R.ACCEPT)][1:]))):
        b = copy.deepcopy(batches[0])
        change(b)
        with pytest.raises(AssertionError):
            loop_same(hip, flow, b, lg[0], size, what)
    with pytest.raises(AssertionError):
        loop_same(hip, flow, batches[0], lg[1], size, "replay 2 against replay 1's reference")
    loop_same(hip, flow, batches[0], lg[0], size, "replay 1")
