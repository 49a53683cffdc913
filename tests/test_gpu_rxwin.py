"""GPU: receive windows (aesgcm_rxwin_*) -- anti-replay and number recovery on the device.  The reference is tests/rxwin_ref.py: a sequential window written from
RFC 4303 A2 that takes a call's authenticated packets in descending number order, and the recovery rules from the standards' pseudo-code.
  grid        sequences of ten commit calls of 1 .. 4097 packets (duplicates inside one wave, across waves, across workgroups) on 1, 3 and 64 windows of 64 and 1024 bits,
              numbers placed at every edge of the window, around 2^32 and at 2^64 - 2: d_why against the reference (the copies of one number as a multiset), exactly one
              accept per fresh (window, number), and the state through aesgcm_rxwin_get after every call; on 3 windows of 128, 256, 512, 2048 and 4096 bits, 257 and 4097
              packets, eight calls more that place the partial clear of [next, M) inside one ring word, up to a word boundary, over three words and around the ring's end
              (asserted from the reference's states)
  forged      d_auth = 0 with numbers far ahead leaves the state as it was
  end to end  on the key-table fixtures: ESN and XPN traffic crossing 2^32 with reordering and loss, SRTP across a sequence rollover, QUIC with the expected number from
              the window -- recover, decrypt, commit; then the same buffer again: every packet a REPLAY, the state unchanged, aesgcm_wipe_failed_dev on d_accept zeroes them
  refusals    a window out of range, a packet shorter than its number field, falling offsets: the status word, NONE, why = 4"""
import random
import struct

import pytest

import quic_fixture as Q
import rxwin_ref as R
import srtp_fixture as S
from kt_common import Sa, _layout, _u32, _u64, _up, evp, x_ref_encrypt  # noqa: F401
from util import splitmix_bytes

pytestmark = pytest.mark.gpu

N_PKTS = [1, 63, 64, 65, 255, 256, 257, 4097]


def _i32(hip, buf, n):
    return list(struct.unpack("<%di" % n, bytes(buf.download(4 * n))))


def _set(rw, sets):
    for w, nx, seen in sets:
        rw.set(w, [nx], [seen])


# every (n_pkts, W, n_wins) of 1 .. 4097 packets x 64 / 1024 bits x 1 / 3 / 64 windows, and the other ring sizes (2, 4, 8, 32 and 64 words) on 3 windows: those run
# R.ring_sequence, whose last eight calls place the partial clear of [next, M) inside one word, up to a word boundary, over three words and around the ring's end
GRID = [(n_pkts, W, n_wins) for n_wins in (1, 3, 64) for W in (64, 1024) for n_pkts in N_PKTS] + [(n_pkts, W, 3) for W in (128, 256, 512, 2048, 4096) for n_pkts in (257, 4097)]


@pytest.mark.parametrize("n_pkts, W, n_wins", GRID)
def test_commit_grid_against_the_sequential_window(hip, n_pkts, W, n_wins):
    rng = random.Random("grid %d %d %d" % (n_pkts, W, n_wins))
    first_next = (0, 2 ** 32 - W // 2, 2 ** 64 - 2)[N_PKTS.index(n_pkts) % 3]      # one window alone meets every starting point over the grid
    if W in (64, 1024):
        sets, calls = R.call_sequence(rng, n_wins, W, n_pkts=n_pkts, first_next=first_next)
        assert len(calls) == 10
    else:
        sets, calls = R.ring_sequence(rng, n_wins, W, n_pkts, first_next=first_next)
        assert len(calls) == 18
        kinds, prev = set(), {w: nx for w, nx, _ in sets}
        for c in calls:                                                         # the placements, read off the reference's states: next mod W and M - next
            for w, (nx, _) in enumerate(c[4]):
                kinds |= R.ring_move_kinds(W, prev[w] % W, nx - prev[w])
                prev[w] = nx
        assert kinds == set(R.RING_MOVES), (W, kinds)
    with hip.RxWindows(n_wins, W) as rw:
        assert rw.get() == ([0] * n_wins, [0] * n_wins)
        _set(rw, sets)
        assert rw.get() == ([s[1] for s in sets], [s[2] for s in sets])
        for k, (wins, nums, auths, why, state, bad) in enumerate(calls):
            assert len(wins) == n_pkts
            accept, got = rw.commit(wins, nums, auths)
            assert accept == [1 if y == R.ACCEPT else 0 for y in got], k
            err = R.same_verdicts(wins, nums, got, why)
            assert err is None, (k, err)
            assert rw.get() == ([s[0] for s in state], [s[1] for s in state]), k
            assert rw.status() == ((hip.EARG, bad) if bad is not None else (hip.OK, 0)), k
            assert rw.status() == (hip.OK, 0)                                   # reading cleared it


@pytest.mark.parametrize("W", [64, 4096])
def test_forged_packets_do_not_move_the_window(hip, W):
    with hip.RxWindows(3, W) as rw:
        rw.set(0, [1000, 0, 2 ** 32], [0xF0F1, 0, (1 << W) - 1])
        before = rw.get()
        wins = [0, 0, 1, 1, 2, 2, 0] * 40
        nums = [5000, 2 ** 64 - 2, 0, 7, 2 ** 32 + 5 * W, 2 ** 33, 999] * 40
        accept, why = rw.commit(wins, nums, [0] * len(wins))
        assert accept == [0] * len(wins) and why == [R.NOAUTH] * len(wins)
        assert rw.get() == before and rw.status() == (hip.OK, 0)
        # the same packets among authenticated ones: only those move it
        auths = [0] * len(wins)
        auths[6] = 1                                                            # (0, 999): seen before (bit 0 of 0xF0F1)
        auths[3] = 1                                                            # (1, 7): fresh
        accept, why = rw.commit(wins, nums, auths)
        assert [(p, y) for p, y in enumerate(why) if y] == [(3, R.ACCEPT), (6, R.REPLAY)] and accept[3] == 1 and sum(accept) == 1
        assert rw.get() == ([1000, 8, 2 ** 32], [0xF0F1, 1, (1 << W) - 1])


def test_set_refuses_bits_below_zero_and_get_round_trips(hip):
    with hip.RxWindows(5, 128) as rw:
        with pytest.raises(hip.AesGcmError):
            rw.set(0, [3], [0b1000])                                            # number -1
        with pytest.raises(hip.AesGcmError):
            rw.set(4, [1, 2])                                                   # past the last window
        rw.set(1, [3, 2 ** 64 - 1, 130], [0b101, (1 << 128) - 1, 1 << 127])
        assert rw.get(1, 3) == ([3, 2 ** 64 - 1, 130], [0b101, (1 << 128) - 1, 1 << 127])
        assert rw.get(0, 1) == ([0], [0]) and rw.get(4) == ([0], [0])
        rw.set(1, [9])                                                          # seen = NULL: nothing seen
        assert rw.get(1, 1) == ([9], [0])


# ---------------------------------------------------------------- end to end on the key-table fixtures
def _dev_call(hip, rw, fmt, wins, off, buf, decrypt, n):
    """recover -> decrypt(d) -> commit with d_accept = d_auth -> wipe on it, all on the null stream; -> (nums, his, out bytes, accept, why)"""
    d = {"win": _up(hip, _u32(wins)), "off": _up(hip, _u64(off)), "buf": _up(hip, buf), "num": _up(hip, bytes(8 * n)), "hi": _up(hip, bytes(4 * n)),
         "auth": _up(hip, b"\x07" * 4 * n), "why": _up(hip, b"\x07" * 4 * n)}
    rw.recover_dev(fmt, n, d["win"].ptr, d["buf"].ptr, d["off"].ptr, d["num"].ptr, d["hi"].ptr)
    num_for_commit = decrypt(d)
    rw.commit_dev(n, d["win"].ptr, num_for_commit, d["auth"].ptr, d["auth"].ptr, d["why"].ptr)
    hip.wipe_failed_dev(n, d["buf"].ptr, d["auth"].ptr, d_data_off=d["off"].ptr)
    hip.dev_sync()
    return (list(struct.unpack("<%dQ" % n, bytes(d["num"].download(8 * n)))), list(struct.unpack("<%dI" % n, bytes(d["hi"].download(4 * n)))),
            bytes(d["buf"].download(len(buf))), _i32(hip, d["auth"], n), _i32(hip, d["why"], n))


def _traffic(rng, start, n, W):
    """n numbers from `start` upwards with loss, reordered by less than W / 4"""
    nums, at = [], start
    for _ in range(n):
        at += 1 + (rng.randrange(4) == 0)
        nums.append(at)
    for i in range(0, n - 8, 8):
        seg = nums[i:i + 8]
        rng.shuffle(seg)
        nums[i:i + 8] = seg
    assert max(nums) - min(nums) + 16 < 8 * W
    return nums


@pytest.mark.parametrize("ext", ["esn", "xpn"])
def test_esn_and_xpn_traffic_crossing_2_32(hip, evp, ext):
    rng = random.Random("e2e " + ext)
    key_len, n_sa, W, n = 16, 3, 1024, 600
    xf = hip.WireFormatX.esp_esn(16) if ext == "esn" else hip.WireFormatX.macsec_xpn()
    rf = hip.RxFormat.esp_esn() if ext == "esn" else hip.RxFormat.macsec_xpn()
    keys, sa = splitmix_bytes(0x7E00, key_len * n_sa), Sa(n_sa, 0x7E01)
    # SA 0 and SA 1 cross 2^32 inside the call; SA 2 is deep in its second epoch
    starts = [2 ** 32 - 150, 2 ** 32 - 3, 2 ** 33 + 77]
    per = [_traffic(rng, s, n // n_sa, W) for s in starts]
    order = [(s, per[s][i]) for i in range(n // n_sa) for s in range(n_sa)]
    slots, nums = [s for s, _ in order], [x for _, x in order]
    at = xf.f.iv_off if ext == "xpn" else 4
    plain = []
    for p, x in enumerate(nums):
        f = bytearray(splitmix_bytes(0x7E10 + p, xf.f.hdr_len + rng.randrange(0, 200)) + b"\xAA" * 16)
        f[at:at + 4] = struct.pack(">I", x & 0xFFFFFFFF)                         # the lower half on the wire
        plain.append(bytes(f))
    wire = x_ref_encrypt(evp, key_len, keys, sa, xf, slots, [x >> 32 for x in nums], plain)
    off, buf = _layout(wire, 5)
    with hip.KeyTable(key_len, n_sa) as kt, hip.RxWindows(n_sa, W) as rw:
        kt.set(0, keys).set_salt(0, b"".join(sa.salt)).set_xpn(0, b"".join(sa.xsalt), b"".join(sa.ssci))
        rw.set(0, [s for s in starts], [rng.getrandbits(64) for _ in starts])   # a receiver in mid-stream: `next` just below each SA's traffic

        def decrypt(d):
            kt.frames_crypt_x_dev(1, xf, len(nums), d["win"].ptr, d["hi"].ptr, d["buf"].ptr, d["off"].ptr, d["buf"].ptr, d_auth=d["auth"].ptr)
            return d["num"].ptr
        got_num, got_hi, out, accept, why = _dev_call(hip, rw, rf, slots, off, buf, decrypt, len(nums))
        assert got_num == nums and got_hi == [x >> 32 for x in nums]
        assert accept == [1] * len(nums) and why == [R.ACCEPT] * len(nums)       # every tag verified under the recovered upper half
        _, want = _layout([f[:-16] + w[-16:] for f, w in zip(plain, wire)], 5)
        assert out == want
        state = rw.get()
        assert state[0] == [max(x) + 1 for x in per] and kt.status() == (hip.OK, 0) and rw.status() == (hip.OK, 0)
        # the same buffer a second time: every frame a replay, nothing moves, and the wipe on d_accept zeroes them
        got_num, _, out, accept, why = _dev_call(hip, rw, rf, slots, off, buf, decrypt, len(nums))
        assert got_num == nums and accept == [0] * len(nums) and why == [R.REPLAY] * len(nums)
        assert rw.get() == state
        assert out == _layout([bytes(len(w)) for w in wire], 5)[1]


def test_srtp_across_a_sequence_rollover(hip):
    rng = random.Random("e2e srtp")
    key_len, n_ssrc, W, per_ssrc = 32, 2, 512, 150
    key, salt = splitmix_bytes(0x7F00, key_len), splitmix_bytes(0x7F01, 12)     # ONE key for both SSRCs: a window is not a key slot
    starts = [(5 << 16) + 65536 - 70, (2 ** 32 - 2 << 16) + 65536 - 20]          # both roll over inside the call; the second into the last rollover counter
    per = [_traffic(rng, s, per_ssrc, W) for s in starts]
    order = [(s, per[s][i]) for i in range(per_ssrc) for s in range(n_ssrc)]
    wins, idx = [s for s, _ in order], [x for _, x in order]
    wire = []
    for p, (s, x) in enumerate(order):
        fill = splitmix_bytes(0x7F10 + p, 300)
        pkt = S.rtp_header(p % 3, None if p % 2 else p % 4, x & 0xFFFF, 1000 + p, 0xABCD0000 + s, fill) + fill[200:200 + rng.randrange(0, 90)] + b"\xAA" * 16
        wire.append(S.protect_rtp(key, salt, x >> 16, pkt))
    off, buf = _layout(wire, 3)
    n = len(wire)
    with hip.KeyTable(key_len, 1) as kt, hip.RxWindows(n_ssrc, W) as rw:
        kt.set(0, key).set_tls_iv(0, salt)
        rw.set(0, starts)
        d_slots = _up(hip, _u32([0] * n))

        def decrypt(d):
            kt.srtp_crypt_dev(1, hip.SrtpFormat.rtp(), n, d_slots.ptr, d["buf"].ptr, d["off"].ptr, d["buf"].ptr, d_roc=d["hi"].ptr, d_auth=d["auth"].ptr)
            return d["num"].ptr
        got_num, got_roc, out, accept, why = _dev_call(hip, rw, hip.RxFormat.srtp(), wins, off, buf, decrypt, n)
        assert got_num == idx and got_roc == [x >> 16 for x in idx]
        assert {x >> 16 for x in idx} == {5, 6, 2 ** 32 - 2, 2 ** 32 - 1}
        assert accept == [1] * n and why == [R.ACCEPT] * n
        want = [S.unprotect_rtp(key, salt, x >> 16, w) for x, w in zip(idx, wire)]
        assert all(ok for _, ok in want) and out == _layout([b for b, _ in want], 3)[1]
        state = rw.get()
        assert state[0] == [max(x) + 1 for x in per]
        got_num, _, out, accept, why = _dev_call(hip, rw, hip.RxFormat.srtp(), wins, off, buf, decrypt, n)
        assert accept == [0] * n and why == [R.REPLAY] * n and rw.get() == state
        assert out == _layout([bytes(len(w)) for w in wire], 3)[1]
        assert kt.status() == (hip.OK, 0) and rw.status() == (hip.OK, 0)


def test_quic_with_the_expected_number_from_the_window(hip):
    rng = random.Random("e2e quic")
    key_len, W, n_space, per_space = 16, 256, 2, 40
    keys, ivs = splitmix_bytes(0x8000, key_len * 2 * n_space), splitmix_bytes(0x8001, 12 * 2 * n_space)
    key = lambda s: keys[key_len * s:key_len * (s + 1)]
    starts = [0, 2 ** 32 - 10]
    per = [_traffic(rng, s, per_space, W) for s in starts]
    order = [(s, per[s][i]) for i in range(per_space) for s in range(n_space)]
    spaces, pns = [s for s, _ in order], [x for _, x in order]
    pn_off, wire = [], []
    for p, (s, pn) in enumerate(order):
        pn_len = 2 + p % 3                                                      # 16 bits and more: the reordering stays inside half the truncated range
        hdr = bytes([0x40 | (pn_len - 1)]) + splitmix_bytes(0x8010 + p, 8) + (pn & ((1 << 8 * pn_len) - 1)).to_bytes(pn_len, "big")
        pn_off.append(9)
        wire.append(Q.protect(key(s), ivs[12 * s:12 * s + 12], key(n_space + s), pn, 9, hdr + splitmix_bytes(0x8100 + p, 20 + rng.randrange(60)) + b"\xAA" * 16))
    off, buf = _layout(wire, 9)
    n = len(wire)
    with hip.KeyTable(key_len, 2 * n_space) as kt, hip.RxWindows(n_space, W) as rw:
        kt.set(0, keys).set_tls_iv(0, ivs)
        rw.set(0, [s + 1 if s else 0 for s in starts])
        d_hp, d_pn_off, d_pn_out = _up(hip, _u32([n_space + s for s in spaces])), _up(hip, _u32(pn_off)), _up(hip, bytes(8 * n))

        def decrypt(d):                                                         # d["num"] = the expected numbers (EXPECT); the decoded ones go to the commit
            kt.quic_crypt_dev(1, n, d["win"].ptr, d_hp.ptr, d["num"].ptr, d_pn_off.ptr, d["buf"].ptr, d["off"].ptr, d["buf"].ptr, d_pn_out=d_pn_out.ptr, d_auth=d["auth"].ptr)
            return d_pn_out.ptr
        fmt = hip.RxFormat.expect()
        nexts = rw.get()[0]
        expected, _, out, accept, why = _dev_call(hip, rw, fmt, spaces, off, buf, decrypt, n)
        assert expected == [nexts[s] for s in spaces]
        assert list(struct.unpack("<%dQ" % n, bytes(d_pn_out.download(8 * n)))) == pns
        assert accept == [1] * n and why == [R.ACCEPT] * n
        want = [Q.unprotect(key(s), ivs[12 * s:12 * s + 12], key(n_space + s), nexts[s], 9, w) for s, w in zip(spaces, wire)]
        assert all(ok and num == pn for (_, num, ok), pn in zip(want, pns)) and out == _layout([b for b, _, _ in want], 9)[1]
        state = rw.get()
        assert state[0] == [max(x) + 1 for x in per]
        expected, _, out, accept, why = _dev_call(hip, rw, fmt, spaces, off, buf, decrypt, n)
        assert expected == [state[0][s] for s in spaces]
        assert accept == [0] * n and why == [R.REPLAY] * n and rw.get() == state
        assert out == _layout([bytes(len(w)) for w in wire], 9)[1]
        assert kt.status() == (hip.OK, 0) and rw.status() == (hip.OK, 0)


# ---------------------------------------------------------------- recover: the rules and the refusals on the device
def test_recover_rules_and_refusals_against_the_reference(hip):
    rng = random.Random("recover")
    n_wins, W = 3, 64
    nexts = [0, 2 ** 32 + 5, 2 ** 64 - 2]
    F = hip.RxFormat
    with hip.RxWindows(n_wins, W) as rw:
        rw.set(0, nexts)
        for fmt in (F.macsec(), F.macsec_xpn(), F.esp(), F.esp_esn(), F.dtls12(), F.srtp(), F.srtcp(), F.srtcp(4), F.expect(), F(1, 0, 8, 0), F(2, 1, 2, 0)):
            pk = [bytes(rng.randrange(256) for _ in range(rng.randrange(0, 40))) for _ in range(300)] + [b"\xff" * 24, b"\xff" * 8, b"", b"\x00" * 20]
            wins = [rng.randrange(n_wins) for _ in pk]
            wins[3], wins[70] = n_wins, 2 ** 32 - 1                             # windows out of range
            offs = [0]
            for p in pk:
                offs.append(offs[-1] + len(p))
            data = b"".join(pk)
            assert offs[10] > 0
            offs[11] = offs[10] - 1                                              # falling offsets: packet 10
            n = len(pk)
            d = {"win": _up(hip, _u32(wins)), "off": _up(hip, _u64(offs)), "buf": _up(hip, data), "num": _up(hip, b"\x07" * 8 * n), "hi": _up(hip, b"\x07" * 4 * n)}
            rw.recover_dev(fmt, n, d["win"].ptr, d["buf"].ptr, d["off"].ptr, d["num"].ptr, d["hi"].ptr)
            hip.dev_sync()
            got = list(zip(struct.unpack("<%dQ" % n, bytes(d["num"].download(8 * n))), struct.unpack("<%dI" % n, bytes(d["hi"].download(4 * n)))))
            want, bad = R.recover((fmt.rule, fmt.num_off, fmt.num_len, fmt.flags), n_wins, W, nexts, wins, data, offs)
            assert got == want, (fmt, [(p, g, w) for p, (g, w) in enumerate(zip(got, want)) if g != w][:4])
            assert got[3] == got[70] == (R.NONE, 0xFFFFFFFF) and (fmt.rule == R.EXPECT or got[10] == (R.NONE, 0xFFFFFFFF))
            assert rw.status() == (hip.EARG, bad) and rw.status() == (hip.OK, 0)
            # what recover refused, commit refuses when it comes authenticated: why = 4, nothing accepted, the status word again
            accept, why = rw.commit(wins, [g[0] for g in got], [1] * n)
            refused = [p for p, g in enumerate(got) if g[0] == R.NONE]
            assert [p for p, y in enumerate(why) if y == R.REFUSED] == refused and all(accept[p] == 0 for p in refused)
            assert rw.status() == (hip.EARG, refused[0])
            rw.set(0, nexts)                                                     # back to where the reference stands
        assert rw.get() == (nexts, [0, 0, 0])
        # d_hi_out is optional, and EXPECT takes no packets
        nums, his = rw.recover(F.expect(), [0, 1, 2, 1])
        assert nums == [0, 2 ** 32 + 5, 2 ** 64 - 2, 2 ** 32 + 5] and his == [0, 1, 2 ** 32 - 1, 1]
        d_win, d_num = _up(hip, _u32([1, 2])), _up(hip, bytes(16))
        rw.recover_dev(F.expect(), 2, d_win.ptr, None, None, d_num.ptr, None)
        hip.dev_sync()
        assert struct.unpack("<2Q", bytes(d_num.download(16))) == (2 ** 32 + 5, 2 ** 64 - 2)
