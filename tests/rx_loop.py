"""What the receive-loop tests share (tests/test_gpu_capture.py: the loop in one graph; tests/test_gpu_rxwin_grid.py: the loop on an ordinary stream for the formats
the graph cases leave out; tests/test_rxwin_cpu.py: the flows themselves, without a device): a Flow per receive format -- packets protected under their TRUE numbers by the
family fixtures over libcrypto (kt_common's nonce and AAD formulas, dtls_fixture, srtp_fixture, quic_fixture) and opened by them under whatever numbers recover gave --
and loop_reference, the three batches every loop runs with what tests/rxwin_ref.py makes of them:
  1  fresh reordered traffic with loss, duplicates inside the call and forged tags (one far ahead, one a copy of a good packet)
  2  the same input again: every packet that still authenticates is a REPLAY, the state unchanged
  3  the next batch from where the reference window stands: next - W - 1, next - W, next - 1, next + W - 1, next + W, one far enough ahead to clear the whole ring, and for
     the flows whose number field ends (top_win) one packet with the field's LAST number
loop_same compares what a run left (d_num, d_hi, d_why, d_accept, the state through get, the output arena, both status words) with a Batch.
Nothing here calls the library: a Flow takes the binding only for the RxFormat / WireFormat presets."""
import random
import struct

import dtls_fixture as D
import kt_common as KC
import quic_fixture as Q
import rxwin_ref as R
import srtp_fixture as S
from util import splitmix_bytes

N = 300
CANARY, POISON, TAG = 0xC5, 0x07, b"\xAA" * 16
RTP_HEADERS = ((0, None), (1, None), (15, None), (0, 0), (1, 1), (15, 5))
FLOWS = ("esn", "srtp", "quic", "dtls13", "srtcp", "macsec", "esp", "xpn", "dtls12", "srtcp_mki")        # (the order seeds the keys: new names go behind)


def _lengths(rng, n):
    lens = [0, 1, 15, 16, 17, 31, 32, 33, 127, 128, 129, 255, 256, 257, 271, 272] + [rng.randrange(273) for _ in range(n - 16)]
    rng.shuffle(lens)
    return lens


def _arena(frames, lead, size):
    b = bytes([CANARY]) * lead + b"".join(frames)
    assert len(b) <= size
    return b + bytes([CANARY]) * (size - len(b))


def _offsets(frames, lead):
    off = [lead]
    for f in frames:
        off.append(off[-1] + len(f))
    return off


class Flow:
    """A receive format on n_wins windows: packets protected under their TRUE numbers by the fixtures, opened by the fixtures under whatever numbers recover gave.
    make(w, num, i, L) -> the packet on the wire; open(w, (num, hi), pkt) -> (what an accepted packet's output is, authentic, the number for the commit).
    The flows that tests/test_gpu_rxwin_grid.py adds also have plain(w, num, i, L), the packet before protection (make = its protection), and:
      macsec     IEEE 802.1AE, the 32-bit PN in the SecTAG (RxFormat.macsec, WireFormat.macsec)
      esp        RFC 4303 without ESN, a 16-byte ICV (RxFormat.esp, WireFormat.esp)
      xpn        IEEE 802.1AEbw: the SecTAG holds the PN's lower half (RxFormat.macsec_xpn, WireFormatX.macsec_xpn)
      dtls12     RFC 6347: windows 2 c and 2 c + 1 are epochs 1 and 2 of connection c, each with a slot of its own (RxFormat.dtls12, DtlsFormat.dtls12)
      srtcp_mki  RFC 3711 3.4 with a 4-byte MKI behind the index; E is set on even indices and clear on odd ones (RxFormat.srtcp(4), SrtpFormat.rtcp(4))"""

    def __init__(self, hip, name, key_len, n_wins):
        self.name, self.kl, self.n_wins = name, key_len, n_wins
        seed = 0x4CB00000 + 256 * FLOWS.index(name) + key_len
        self.n_slots = 2 * n_wins
        self.keys = splitmix_bytes(seed, key_len * self.n_slots)
        self.sa = KC.Sa(self.n_slots, seed + 1)
        ib = splitmix_bytes(seed + 4, 12 * self.n_slots)
        self.ivs = [ib[12 * s:12 * s + 12] for s in range(self.n_slots)]
        self.blob = splitmix_bytes(seed + 5, 1 << 16)
        F = hip.RxFormat
        self.fmt = {"esn": F.esp_esn, "srtp": F.srtp, "quic": F.expect, "dtls13": F.expect, "srtcp": F.srtcp, "macsec": F.macsec, "esp": F.esp, "xpn": F.macsec_xpn,
                    "dtls12": F.dtls12, "srtcp_mki": lambda: F.srtcp(4)}[name]()
        self.one_key = name == "srtp"                                            # one key for every SSRC: a window is not a key slot
        self.top = {"esn": 2 ** 64 - 2, "srtp": 2 ** 48 - 1, "quic": 2 ** 62 - 1, "dtls13": 2 ** 64 - 2, "srtcp": 2 ** 31 - 1, "macsec": 2 ** 32 - 1, "esp": 2 ** 32 - 1,
                    "xpn": 2 ** 64 - 2, "dtls12": 2 ** 48 - 1, "srtcp_mki": 2 ** 31 - 1}[name]
        self.trail = {"srtcp": 4, "srtcp_mki": 8}.get(name, 0)                  # what follows the tag
        self.top_win = 1 if name in ("macsec", "esp", "dtls12", "srtcp_mki") else None      # the window whose traffic ends at the field's last number, `top`
        self.wf = {"macsec": hip.WireFormat.macsec, "esp": hip.WireFormat.esp, "xpn": hip.WireFormatX.macsec_xpn}.get(name, lambda: None)()

    def key(self, s):
        return self.keys[self.kl * s:self.kl * (s + 1)]

    def slot(self, w):
        return 0 if self.one_key else w

    def starts(self, W):
        """where each window's traffic begins: the first three are the format's edges"""
        edge = {"esn": [2 ** 32 - 20, 2 ** 32 - 3, 2 ** 33 + 77], "srtp": [(5 << 16) + 65536 - 25, (2 ** 32 - 2 << 16) + 65536 - 9, 1000], "quic": [0, 2 ** 32 - 10, 2 ** 40],
                "dtls13": [0, 2 ** 32 - 10, 2 ** 48 - 7], "srtcp": [0, 2 ** 16 - 11, 2 ** 30], "xpn": [2 ** 32 - 20, 2 ** 32 - 3, 2 ** 33 + 77],
                "macsec": [0, self.top - 3 * W, 2 ** 31 + 5], "esp": [0, self.top - 3 * W, 2 ** 31 + 5], "dtls12": [0, self.top - 3 * W, 2 ** 32 - 10],
                "srtcp_mki": [0, self.top - 3 * W, 2 ** 30 + 2 ** 16 - 11]}[self.name]
        return edge + [7777 * (w + 1) + (2 ** 20 if not self.name.startswith("srtcp") else 0) for w in range(3, self.n_wins)]

    def plain(self, w, num, i, L):
        """the new flows' packet before protection: header with the truncated number | payload | 16 placeholder bytes | trailer"""
        f = self.blob[(97 * i) % 60000:(97 * i) % 60000 + 400]
        pay = f[100:100 + L]
        if self.name in ("macsec", "xpn"):                                       # DA SA | EtherType, TCI / AN, SL | PN | SCI
            return f[:16] + struct.pack(">I", num & 0xFFFFFFFF) + f[20:28] + pay + TAG
        if self.name == "esp":                                                   # SPI | sequence number | IV
            return f[:4] + struct.pack(">I", num) + f[8:16] + pay + TAG
        if self.name == "dtls12":
            return D.header12(23, 1 + (w & 1), num, L) + f[:8] + pay + TAG
        assert self.name == "srtcp_mki"
        return bytes([0x80 | (f[0] & 0x3F)]) + f[1:8] + pay + TAG + struct.pack(">I", (1 - num % 2) << 31 | num) + f[8:12]

    def make(self, w, num, i, L):
        f = self.blob[(97 * i) % 60000:(97 * i) % 60000 + 400]
        s, pay = self.slot(w), f[100:100 + L]
        if self.name == "esn":
            from oracle import libcrypto_ref as LR
            hdr = f[:4] + struct.pack(">I", num & 0xFFFFFFFF) + f[8:16]
            ct, tag = LR.encrypt(self.key(s), self.sa.salt[s][:4] + hdr[8:16], hdr[:4] + struct.pack(">I", num >> 32) + hdr[4:8], pay)
            return hdr + bytes(ct) + bytes(tag)
        if self.name == "srtp":
            pkt = S.rtp_header(RTP_HEADERS[i % 6][0], RTP_HEADERS[i % 6][1], num & 0xFFFF, 1000 + i, 0xABCD0000 + w, f) + pay + TAG
            return S.protect_rtp(self.key(s), self.ivs[s], num >> 16, pkt)
        if self.name == "quic":
            pkt = bytes([0x43]) + f[:8] + (num & 0xFFFFFFFF).to_bytes(4, "big") + pay + TAG
            return Q.protect(self.key(s), self.ivs[s], self.key(self.n_wins + w), num, 9, pkt)
        if self.name == "dtls13":
            cid = f[:(0, 1, 7, 20)[i % 4]]
            pkt = D.header13(cid, num, True, i % 5 in (1, 4), w & 3, len(pay) + 16) + pay + TAG
            return D.protect13(self.key(s), self.ivs[s], self.key(self.n_wins + w), num, 1 + len(cid), pkt)
        if self.name == "srtcp":
            pkt = bytes([0x80 | (f[0] & 0x3F)]) + f[1:8] + pay + TAG + struct.pack(">I", (i % 2) << 31 | num)
            return S.protect_rtcp(self.key(s), self.ivs[s], pkt, 0)
        p = self.plain(w, num, i, L)
        if self.name in ("macsec", "esp", "xpn"):
            from oracle import libcrypto_ref as LR
            nonce, aad, data = KC.x_split(self.wf, self.sa, s, num >> 32, p) if self.name == "xpn" else KC.wire_split(self.wf, self.sa.salt[s], p)
            ct, tag = LR.encrypt(self.key(s), nonce, aad, data)
            return p[:len(p) - 16 - len(data)] + bytes(ct) + bytes(tag)
        if self.name == "dtls12":
            return D.protect12(self.key(s), self.ivs[s], p)
        return S.protect_rtcp(self.key(s), self.ivs[s], p, 4)

    def open(self, w, rec, pkt, cid_len=None):
        num, hi = rec
        s = self.slot(w)
        if self.name == "esn":
            from oracle import libcrypto_ref as LR
            pt, ok = LR.decrypt(self.key(s), self.sa.salt[s][:4] + pkt[8:16], pkt[:4] + struct.pack(">I", hi) + pkt[4:8], pkt[16:-16], pkt[-16:])
            return pkt[:16] + bytes(pt) + pkt[-16:], int(bool(ok)), num
        if self.name == "srtp":
            out, ok = S.unprotect_rtp(self.key(s), self.ivs[s], hi, pkt)
            return out, int(bool(ok)), num
        if self.name == "quic":
            out, pn, ok = Q.unprotect(self.key(s), self.ivs[s], self.key(self.n_wins + w), num, 9, pkt)
            return out, int(bool(ok)), pn
        if self.name == "dtls13":
            out, q, ok = D.unprotect13(self.key(s), self.ivs[s], self.key(self.n_wins + w), num, 1 + cid_len, pkt)
            return out, int(bool(ok)), q
        if self.name == "srtcp":
            out, ok = S.unprotect_rtcp(self.key(s), self.ivs[s], pkt, 0)
            return out, int(bool(ok)), num
        if self.name in ("macsec", "esp", "xpn"):
            from oracle import libcrypto_ref as LR
            nonce, aad, data = KC.x_split(self.wf, self.sa, s, hi, pkt) if self.name == "xpn" else KC.wire_split(self.wf, self.sa.salt[s], pkt)
            pt, ok = LR.decrypt(self.key(s), nonce, aad, data, pkt[-16:])
            return pkt[:len(pkt) - 16 - len(data)] + bytes(pt) + pkt[-16:], int(bool(ok)), num
        if self.name == "dtls12":
            out, ok = D.unprotect12(self.key(s), self.ivs[s], pkt)
            return out, int(bool(ok)), num
        out, ok = S.unprotect_rtcp(self.key(s), self.ivs[s], pkt, 4)
        return out, int(bool(ok)), num

    def table(self, hip):
        kt = hip.KeyTable(self.kl, self.n_slots)
        kt.set(0, self.keys)
        if self.name in ("esn", "xpn"):
            kt.set_salt(0, b"".join(self.sa.salt)).set_xpn(0, b"".join(self.sa.xsalt), b"".join(self.sa.ssci))
        elif self.name in ("macsec", "esp"):
            kt.set_salt(0, b"".join(self.sa.salt))
        else:
            kt.set_tls_iv(0, b"".join(self.ivs))
        return kt


def _fresh(rng, start, count):
    """count numbers from `start` upwards with loss, reordered inside groups of eight"""
    nums, at = [], start
    for _ in range(count):
        nums.append(at)
        at += 1 + (rng.randrange(4) == 0)
    for i in range(0, count - 8, 8):
        seg = nums[i:i + 8]
        rng.shuffle(seg)
        nums[i:i + 8] = seg
    return nums


class Batch:
    """one replay's input and what the reference makes of it"""


def _packets(flow, rng, items, k):
    """items = [(window, true number, forged)] -> (the packets on the wire, each one's connection-ID length where the format has one)"""
    n = len(items)
    lens = _lengths(rng, n)
    made, pkts, cids = {}, [], []
    for i, (w, num, forged) in enumerate(items):
        if (w, num) not in made:                                                # a duplicate is the same packet again, byte for byte
            made[w, num] = (flow.make(w, num, 1000 * k + i, lens[i]), (0, 1, 7, 20)[(1000 * k + i) % 4])
        pkt, cid = made[w, num]
        if forged:
            x = bytearray(pkt)
            x[len(pkt) - flow.trail - 16 + i % 16] ^= 1 << (i % 8)
            pkt = bytes(x)
        pkts.append(pkt)
        cids.append(cid)
    return pkts, cids


def _batch(flow, W, windows, items, made, lead):
    """the reference's recover, decrypt and commit of one replay's packets over `windows` (which move)"""
    b = Batch()
    pkts, cids = made
    b.wins = [w for w, _, _ in items]
    b.pkts, b.lead = pkts, lead
    b.off = _offsets(pkts, lead)
    data = bytes(lead) + b"".join(pkts)
    nexts = [windows[w].next for w in range(flow.n_wins)]
    f = flow.fmt
    b.rec, bad = R.recover((f.rule, f.num_off, f.num_len, f.flags), flow.n_wins, W, nexts, b.wins, data, b.off)
    assert bad is None
    opened = [flow.open(w, r, p, c) for w, r, p, c in zip(b.wins, b.rec, pkts, cids)]
    b.plain, b.auth, b.cnum = [o[0] for o in opened], [o[1] for o in opened], [o[2] for o in opened]
    b.sn_off = [9 if flow.name == "quic" else 1 + c for c in cids]
    b.why = R.commit(windows, b.wins, b.cnum, b.auth)
    b.state = [windows[w].normalised() for w in range(flow.n_wins)]
    return b


_LOOPS = {}


def loop_reference(hip, name, W, key_len):
    """the three replays of a receive loop: -> (flow, where the windows start, [Batch] * 3)"""
    if (name, W) in _LOOPS:
        return _LOOPS[name, W]
    n_wins = 3 if W >= 1024 else 9
    flow = Flow(hip, name, key_len, n_wins)
    rng = random.Random("loop %s %d" % (name, W))
    starts = flow.starts(W)
    windows = {w: R.Window(W, starts[w]) for w in range(n_wins)}
    per = N // n_wins - 6
    items = []
    for w in range(n_wins):
        nums = _fresh(rng, starts[w], per)
        assert max(nums) - min(nums) < W - 2, (name, W)                         # the whole call inside one window: replay 2 is all REPLAY
        items += [(w, x, False) for x in nums]
        items += [(w, nums[3], False), (w, nums[3], False), (w, nums[per // 2], False)]      # duplicates inside the call: three copies and two
        items += [(w, min(max(nums) + min(40 * W, 20000), flow.top), True), (w, nums[5], True)]      # forged: one far ahead, one a copy of a good packet
    while len(items) < N:
        items.append((len(items) % n_wins, max(x for w, x, forged in items if w == len(items) % n_wins and not forged) + 2, False))
    assert all(x <= flow.top for _, x, _ in items), (name, W)
    order = list(range(len(items)))
    for i in range(0, len(order) - 16, 16):                                      # the windows interleaved, the copies apart
        seg = order[i:i + 16]
        rng.shuffle(seg)
        order[i:i + 16] = seg
    rng.shuffle(order)
    items = [items[i] for i in order]
    made = _packets(flow, rng, items, 1)
    b1 = _batch(flow, W, windows, items, made, 5)
    assert R.ACCEPT in b1.why and R.REPLAY in b1.why and R.NOAUTH in b1.why
    state1 = list(b1.state)
    b2 = _batch(flow, W, windows, items, made, 5)                               # the same input again
    assert [y for y, a in zip(b2.why, b2.auth) if a] == [R.REPLAY] * sum(b2.auth) and sum(b2.auth) > N // 2 and b2.state == state1
    items3 = []
    for w in range(n_wins):
        nx = windows[w].next
        edges = [nx - W - 1, nx - W, nx - 1] + ([nx + W - 1, nx + W] if w % 3 != 2 else [])      # every third window stays where it is: its next - 1 is a REPLAY
        far = nx + 6 * W if w % 3 == 0 else None                                 # ... and every third is cleared whole
        items3 += [(w, x, False) for x in edges if 0 <= x <= flow.top] + ([(w, far, False)] if far is not None and far <= flow.top else [])
    if flow.top_win is not None:
        items3.append((flow.top_win, flow.top, False))                           # the call ends at the field's last number
    while len(items3) < N:
        w = len(items3) % n_wins
        items3.append((w, min(windows[w].next + rng.randrange(-W // 2, W), flow.top) if windows[w].next > W else windows[w].next + rng.randrange(W), rng.randrange(7) == 0))
    rng.shuffle(items3)
    b3 = _batch(flow, W, windows, items3, _packets(flow, rng, items3, 3), 11)
    assert {R.ACCEPT, R.OLD, R.REPLAY} <= set(b3.why) and b3.state != state1
    assert flow.top_win is None or b3.state[flow.top_win][0] == flow.top + 1, (name, W)
    _LOOPS[name, W] = (flow, starts, [b1, b2, b3])
    return _LOOPS[name, W]


def loop_same(hip, flow, b, got, size, label):
    assert got["num"] == [r[0] for r in b.rec], (label, "d_num")
    assert got["hi"] == [r[1] for r in b.rec], (label, "d_hi")
    err = R.same_verdicts(b.wins, b.cnum, got["why"], b.why)
    assert err is None, (label, "d_why", err)
    assert got["accept"] == [1 if y == R.ACCEPT else 0 for y in got["why"]], (label, "d_accept")
    assert got["state"] == ([s[0] for s in b.state], [s[1] for s in b.state]), (label, "rw.get()", got["state"][0], [s[0] for s in b.state])
    want = _arena([pl if y == R.ACCEPT else bytes(len(pl)) for pl, y in zip(b.plain, got["why"])], b.lead, size)
    if got["out"] != want:
        at = next(i for i, (x, y) in enumerate(zip(got["out"], want)) if x != y)
        pkt = max(i for i in range(len(b.off)) if b.off[i] <= at) if at >= b.lead else -1
        raise AssertionError("%s: output byte %d (packet %d, verdict %s) is %02x, want %02x" % (label, at, pkt, got["why"][pkt] if 0 <= pkt < len(b.wins) else None, got["out"][at], want[at]))
    assert got["status"] == ((hip.OK, 0), (hip.OK, 0)), (label, got["status"])
