"""GPU: IKEv2's prf+ on the device (aesgcm_prfplus_*).  SK_d values and derived keys cannot be read back, so everything is checked through what the installed slots DO:
ESP frames are encrypted on the GPU under the installed slots (KeyTable.crypt_frames, WireFormat.esp) and must equal, every byte, what the wire fixture makes over
libcrypto under the key AND the four salt bytes that ikev2_ref derives with hmac.
  grid         3 hashes x 3 key sizes at 1 / 257 / 4097 entries (below a workgroup, one lane into the second, one into the seventeenth), indices and slots permuted,
               the arrays and the byte-packed seeds between guard words, the slots not named compared before and after
  seeds        one call of 261 entries: seed lengths 1 .. 260 byte-packed, so every start alignment occurs, and one seed of 2048 bytes
  directions   i2r only, r2i only, 0xFFFFFFFF mixed per entry; not both NULL
  refusals     index out of range, unset, cleared, a slot out of range in either array, falling offsets, an empty seed, 2049 bytes: skipped whole, the old key and
               salt kept, the lowest in status(), the key table's status untouched
  shared       many Child SAs on one record
  capture      install + encrypt in one linear graph replayed three times over changed seeds
  rekey loop   TxCounters refuses at the limit, install with new nonces into fresh slots, counter reset, ESN frames across 2^32 encrypted, and decrypted under the other
               table that the same KEYMAT's same direction filled, with RxWindows: launches on one stream"""
import random
import struct

import pytest

import hip_graph as G
import ikev2_ref as IK
import pkt_grid as PG
from kt_common import Guarded, Sa, _layout, _u32, _u64, _up, evp, wire_ref_encrypt, x_ref_encrypt  # noqa: F401
from util import splitmix_bytes

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
HLS = (32, 48, 64)


def _frame(i):
    """an ESP frame before protection: SPI | sequence number | 8-byte IV field | payload | 16 placeholder bytes"""
    return splitmix_bytes(7000 + i, 16 + 5 + i % 23) + bytes(16)


def _check(hip, evp, kt, held, label=""):  # noqa: F811
    """held: {slot: (key, salt4)} -- one ESP frame per slot on the GPU against libcrypto under that key and salt, every byte"""
    slots = sorted(held)
    keys = b"".join(held[s][0] if s in held else bytes(kt.key_len) for s in range(kt.n_slots))
    salts = [held[s][1] + bytes(4) if s in held else bytes(8) for s in range(kt.n_slots)]
    frames = [_frame(i) for i in range(len(slots))]
    fmt = hip.WireFormat.esp(16)
    got, _ = kt.crypt_frames(fmt, slots, frames)
    want = wire_ref_encrypt(evp, kt.key_len, keys, salts, fmt, slots, frames)
    for i, s in enumerate(slots):
        assert bytes(got[i]) == want[i], (label, kt.key_len, "slot", s)
    assert kt.status() == (hip.OK, 0), label


def _old(kt, n_slots, seed):
    """every slot set by hand: what a slot that no entry names, or that a refused entry names, must still hold"""
    old = {s: (splitmix_bytes(seed + s, kt.key_len), splitmix_bytes(seed + 50000 + s, 4)) for s in range(n_slots)}
    kt.set(0, b"".join(old[s][0] for s in range(n_slots))).set_salt(0, b"".join(old[s][1] + bytes(4) for s in range(n_slots)))
    return old


# ---------------------------------------------------------------- the grid
@pytest.mark.parametrize("n", [1, 257, 4097])
@pytest.mark.parametrize("key_len", [16, 24, 32])
@pytest.mark.parametrize("hl", HLS)
def test_install_random_child_sas_between_guards(hip, evp, hl, key_len, n):  # noqa: F811
    """slots 0 and 2 n + 1 are set by hand and never named; the arrays and the seeds lie between guard words"""
    rng = random.Random("prfplus %d %d %d" % (hl, key_len, n))
    n_keys = max(1, n // 3)
    sk = splitmix_bytes(n + hl + key_len, hl * n_keys)
    seeds = [splitmix_bytes(90000 + 7 * i + n, rng.randrange(16, 81)) for i in range(n)]
    off = [0]
    for s in seeds:
        off.append(off[-1] + len(s))
    idx, a, b = [rng.randrange(n_keys) for _ in range(n)], list(range(1, n + 1)), list(range(n + 1, 2 * n + 1))
    rng.shuffle(a)
    rng.shuffle(b)
    with hip.IkeSaTable(hl, n_keys) as it, hip.KeyTable(key_len, 2 * n + 2) as kt:
        it.set(0, sk)
        held = {s: (splitmix_bytes(5 + e, key_len), splitmix_bytes(9 + e, 4)) for e, s in enumerate((0, 2 * n + 1))}
        for s, (k, salt) in held.items():
            kt.set(s, k).set_salt(s, salt + bytes(4))
        data = (_u32(idx), b"".join(seeds), _u32(off), _u32(a), _u32(b))
        g = [Guarded(hip, len(d)) for d in data]
        for gb, d in zip(g, data):
            gb.buf.upload(d, PG.GUARD)
        it.install_dev(kt, n, g[0].ptr, g[1].ptr, g[2].ptr, g[3].ptr, g[4].ptr)
        hip.dev_sync()
        assert [gb.read("array") for gb in g] == list(data)
        assert it.status() == (hip.OK, 0)
        for i in range(n):
            held[a[i]], held[b[i]] = IK.child_sa(hl, sk[hl * idx[i]:hl * idx[i] + hl], seeds[i], key_len)
        _check(hip, evp, kt, held, "n=%d" % n)
        for gb in g:
            gb.buf.free()


# ---------------------------------------------------------------- seed lengths and alignments
@pytest.mark.parametrize("hl,key_len", [(32, 32), (48, 16), (64, 24)])
def test_every_seed_length_to_260_byte_packed_and_one_of_2048(hip, evp, hl, key_len):  # noqa: F811
    seeds = [splitmix_bytes(300 + n, n) for n in range(1, 261)] + [splitmix_bytes(299, 2048)]
    n = len(seeds)
    starts = {sum(len(s) for s in seeds[:i]) % 4 for i in range(n)}
    assert starts == {0, 1, 2, 3}
    sk = splitmix_bytes(77 + hl, hl)
    with hip.IkeSaTable(hl, 1) as it, hip.KeyTable(key_len, 2 * n) as kt:
        it.set(0, sk).install(kt, [0] * n, seeds, list(range(n)), list(range(n, 2 * n)))
        assert it.status() == (hip.OK, 0)
        held = {}
        for i in range(n):
            held[i], held[n + i] = IK.child_sa(hl, sk, seeds[i], key_len)
        _check(hip, evp, kt, held, "lengths")


# ---------------------------------------------------------------- directions
@pytest.mark.parametrize("hl,key_len", [(32, 16), (48, 32), (64, 24)])
def test_one_direction_only(hip, evp, hl, key_len):  # noqa: F811
    n = 70
    sk = splitmix_bytes(21 + hl, hl * n)
    seeds = [splitmix_bytes(500 + i, 40 + i) for i in range(n)]
    want = lambda d, i: IK.child_sa(hl, sk[hl * i:hl * i + hl], seeds[i], key_len)[d]
    idx = list(range(n))
    with hip.IkeSaTable(hl, n) as it, hip.KeyTable(key_len, 2 * n) as kt:
        it.set(0, sk)
        old = _old(kt, 2 * n, 40)
        it.install(kt, idx, seeds, list(range(n)), None)                        # i2r only: slots n .. 2 n - 1 keep their keys and salts
        _check(hip, evp, kt, {**{i: want(0, i) for i in range(n)}, **{n + i: old[n + i] for i in range(n)}}, "i2r only")
        old = _old(kt, 2 * n, 41)
        it.install(kt, idx, seeds, None, list(range(n, 2 * n)))
        _check(hip, evp, kt, {**{i: old[i] for i in range(n)}, **{n + i: want(1, i) for i in range(n)}}, "r2i only")
        old = _old(kt, 2 * n, 42)
        a = [NONE if i % 3 == 0 else i for i in range(n)]
        b = [NONE if i % 3 == 1 else n + i for i in range(n)]
        it.install(kt, idx, seeds, a, b)
        _check(hip, evp, kt, {**{i: old[i] if a[i] == NONE else want(0, i) for i in range(n)}, **{n + i: old[n + i] if b[i] == NONE else want(1, i) for i in range(n)}}, "mixed")
        assert it.status() == (hip.OK, 0)
        with pytest.raises(hip.AesGcmError):
            it.install_dev(kt, 1, 16, 16, 16, None, None)                       # not both NULL


# ---------------------------------------------------------------- refusals
@pytest.mark.parametrize("only", [None, "r2i"])
def test_refusals_scattered_through_257_entries(hip, evp, only):  # noqa: F811
    """every refusal kind in one call; only = "r2i": the call has no i2r array, so the r2i lanes report and a bad i2r slot is nobody's"""
    n, hl, key_len = 257, 48, 24
    sk = splitmix_bytes(31, hl * n)
    seeds = [splitmix_bytes(600 + i, 2049 if i == 40 else 33 + i % 50) for i in range(n)]       # entry 40: one byte too long
    packed = b"".join(seeds)
    off = [0]
    for s in seeds:
        off.append(off[-1] + len(s))
    off[121] = off[120]                                                         # entry 120: empty (121 starts there and is longer for it)
    off[151] = off[150] - 10                                                    # entry 150: falling (151 starts ten bytes early)
    seed_of = lambda i: packed[off[i]:off[i + 1]]
    idx, a, b = list(range(n)), list(range(n)), list(range(n, 2 * n))
    idx[17], idx[64] = n + 2, n + 1                                              # out of range; unset
    a[200], b[230] = 2 * n, 2 * n + 5                                            # a slot out of range, in either array
    bad = {17, 40, 64, 100, 120, 150, 230} | ({200} if only is None else set())
    with hip.IkeSaTable(hl, n + 2) as it, hip.KeyTable(key_len, 2 * n) as kt:
        it.set(0, sk)                                                           # records n, n + 1 stay unset
        it.clear(100)                                                           # cleared
        old = _old(kt, 2 * n, 400)
        d = {k: _up(hip, v) for k, v in (("idx", _u32(idx)), ("seed", packed), ("off", _u32(off)), ("a", _u32(a)), ("b", _u32(b)))}
        it.install_dev(kt, n, d["idx"].ptr, d["seed"].ptr, d["off"].ptr, None if only else d["a"].ptr, d["b"].ptr)
        hip.dev_sync()
        assert it.status() == (hip.EARG, 17) and it.status() == (hip.OK, 0)     # the lowest index; reading clears
        assert kt.status() == (hip.OK, 0)                                       # the key table's status word is not touched
        held = dict(old)                                                        # a refused entry's slots keep their old key and salt, in both directions
        for i in range(n):
            if i not in bad:
                sa = IK.child_sa(hl, sk[hl * idx[i]:hl * idx[i] + hl], seed_of(i), key_len)
                if only is None:
                    held[a[i]] = sa[0]
                held[b[i]] = sa[1]
        _check(hip, evp, kt, held, "refusals")
        for x in d.values():
            x.free()


# ---------------------------------------------------------------- many Child SAs on one record
def test_many_child_sas_share_one_record(hip, evp):  # noqa: F811
    n, hl, key_len = 300, 64, 32
    sk = splitmix_bytes(808, hl * 2)
    seeds = [splitmix_bytes(800 + i, 64) for i in range(n)]
    idx = [0 if i % 7 else 1 for i in range(n)]
    with hip.IkeSaTable(hl, 2) as it, hip.KeyTable(key_len, 2 * n) as kt:
        it.set(0, sk).install(kt, idx, seeds, list(range(0, 2 * n, 2)), list(range(1, 2 * n, 2)))
        held = {}
        for i in range(n):
            held[2 * i], held[2 * i + 1] = IK.child_sa(hl, sk[hl * idx[i]:hl * idx[i] + hl], seeds[i], key_len)
        assert len({v for v in held.values()}) == 2 * n
        _check(hip, evp, kt, held, "shared")
        assert it.status() == (hip.OK, 0)


# ---------------------------------------------------------------- capture
def test_captured_install_and_encrypt_replays_over_changed_seeds(hip, evp):  # noqa: F811
    n, hl, key_len = 100, 48, 32
    sk = splitmix_bytes(909, hl * n)
    gens = [[splitmix_bytes(1000 * g + i, 48) for i in range(n)] for g in range(3)]
    frames = [_frame(p) for p in range(n)]
    off, buf = _layout(frames, 0, 0)
    fmt = hip.WireFormat.esp(16)
    perm = list(range(n))
    random.Random(6).shuffle(perm)
    st = G.stream_create()
    with hip.IkeSaTable(hl, n) as it, hip.KeyTable(key_len, 2 * n) as kt:
        it.set(0, sk)
        hip.dev_sync()
        d_idx, d_a, d_b = _up(hip, _u32(perm)), _up(hip, _u32(perm)), _up(hip, _u32([n + x for x in perm]))
        d_soff, d_seed = _up(hip, _u32([48 * i for i in range(n + 1)])), _up(hip, b"".join(gens[0]))
        d_pslots, d_off = _up(hip, _u32([p if p % 2 == 0 else n + p for p in range(n)])), _up(hip, _u64(off))
        d_in, d_out = _up(hip, buf), _up(hip, bytes(len(buf)))

        def enqueue():
            it.install_dev(kt, n, d_idx.ptr, d_seed.ptr, d_soff.ptr, d_a.ptr, d_b.ptr, stream=st)
            kt.frames_crypt_dev(0, fmt, n, d_pslots.ptr, d_in.ptr, d_off.ptr, d_out.ptr, stream=st)

        try:
            enqueue()                                                           # the ordinary call of each
            G.synchronize(st)
            with G.Graph(st, enqueue) as graph:
                for g in range(3):
                    d_seed.upload(b"".join(gens[g]))                            # outside the capture: entry i's seed belongs to record perm[i]
                    graph.launch()
                    out = bytes(d_out.download(len(buf)))
                    keys, salts = [None] * (2 * n), [None] * (2 * n)
                    for i in range(n):
                        sa = IK.child_sa(hl, sk[hl * perm[i]:hl * perm[i] + hl], gens[g][i], key_len)
                        for dirn, slot in ((0, perm[i]), (1, n + perm[i])):
                            keys[slot], salts[slot] = sa[dirn][0], sa[dirn][1] + bytes(4)
                    want = wire_ref_encrypt(evp, key_len, b"".join(keys), salts, fmt, [p if p % 2 == 0 else n + p for p in range(n)], frames)
                    assert out == b"".join(want), g
            assert it.status() == (hip.OK, 0) and kt.status() == (hip.OK, 0)
        finally:
            for x in (d_idx, d_a, d_b, d_soff, d_seed, d_pslots, d_off, d_in, d_out):
                x.free()
    G.stream_destroy(st)


# ---------------------------------------------------------------- the rekey loop on one stream
def test_rekey_loop_with_esn_across_2_32_on_one_stream(hip, evp):  # noqa: F811
    """an initiator's sending side and the responder's receiving side.  Generation 0 runs its counters into their limit, where assign refuses; the rekey installs the
    i2r keys of new nonces into FRESH slots of both tables, resets counters and windows to 2^32 - 3, and the frames go out with ESN across 2^32 and come in accepted"""
    n_sa, per, hl, key_len, W = 5, 6, 32, 16, 64
    n = n_sa * per
    sk = splitmix_bytes(1212, hl * n_sa)
    nonces = [[splitmix_bytes(1300 + 10 * g + s, 64) for s in range(n_sa)] for g in range(2)]
    xf, tf, rf = hip.WireFormatX.esp_esn(16), hip.TxFormat.esp_esn(), hip.RxFormat.esp_esn()
    sas = [p // per for p in range(n)]
    plain = [splitmix_bytes(1400 + p, 16 + 9 + p % 31) + b"\xAA" * 16 for p in range(n)]
    off, buf = _layout(plain, 5)
    start = 2 ** 32 - 3
    st = G.stream_create()
    with hip.IkeSaTable(hl, n_sa) as it, hip.KeyTable(key_len, 2 * n_sa) as tx, hip.KeyTable(key_len, 2 * n_sa) as rx, hip.TxCounters(n_sa, n) as tc, hip.RxWindows(n_sa, W) as rw:
        it.set(0, sk)
        tx.set(0, bytes(key_len))
        rx.set(0, bytes(key_len))                                               # one ordinary call per table before the loop (per-device state)
        hip.dev_sync()
        d = {k: _up(hip, v) for k, v in (("all", _u32(list(range(n_sa)))), ("new", _u32([n_sa + s for s in range(n_sa)])), ("soff", _u32([64 * s for s in range(n_sa + 1)])),
                                         ("seed0", b"".join(nonces[0])), ("seed1", b"\xEE" + b"".join(nonces[1])), ("ctr", _u32(sas)), ("slots", _u32(sas)),
                                         ("slots1", _u32([n_sa + s for s in sas])), ("off", _u64(off)), ("buf", buf), ("num", bytes(8 * n)), ("hi", bytes(4 * n)),
                                         ("rnum", bytes(8 * n)), ("rhi", bytes(4 * n)), ("auth", b"\x07" * 4 * n), ("why", b"\x07" * 4 * n))}
        p = lambda k: d[k].ptr
        try:
            # generation 0: keys of the first nonces in slots 0 .. n_sa - 1; every counter stands at its limit, so assign refuses every frame
            it.install_dev(tx, n_sa, p("all"), p("seed0"), p("soff"), p("all"), None, stream=st)
            tc.set(0, [100] * n_sa, [100] * n_sa, stream=st)
            tc.assign_dev(tf, n, p("ctr"), p("buf"), p("off"), p("num"), p("hi"), p("slots"), stream=st)
            G.synchronize(st)
            assert tc.status() == (hip.EARG, 0)                                 # refused at the limit: time to rekey
            assert list(struct.unpack("<%dI" % n, bytes(d["slots"].download(4 * n)))) == [NONE] * n
            # the rekey: new nonces (an odd address), fresh slots in both tables, counters and windows reset, then the traffic -- launches on one stream
            tc.set(0, [start] * n_sa, [2 ** 64 - 1] * n_sa, stream=st)
            rw.set(0, [start] * n_sa, stream=st)
            it.install_dev(tx, n_sa, p("all"), p("seed1") + 1, p("soff"), p("new"), None, stream=st)      # the initiator's outbound SA: its sending table
            it.install_dev(rx, n_sa, p("all"), p("seed1") + 1, p("soff"), p("new"), None, stream=st)      # the responder's inbound SA: the same direction of the same KEYMAT
            tc.assign_dev(tf, n, p("ctr"), p("buf"), p("off"), p("num"), p("hi"), p("slots1"), stream=st)
            tx.frames_crypt_x_dev(0, xf, n, p("slots1"), p("hi"), p("buf"), p("off"), p("buf"), stream=st)
            G.synchronize(st)
            wire_got = bytes(d["buf"].download(len(buf)))
            rw.recover_dev(rf, n, p("ctr"), p("buf"), p("off"), p("rnum"), p("rhi"), stream=st)
            rx.frames_crypt_x_dev(1, xf, n, p("slots1"), p("rhi"), p("buf"), p("off"), p("buf"), d_auth=p("auth"), stream=st)
            rw.commit_dev(n, p("ctr"), p("rnum"), p("auth"), p("auth"), p("why"), stream=st)
            G.synchronize(st)
            nums = list(struct.unpack("<%dQ" % n, bytes(d["num"].download(8 * n))))
            assert nums == [start + q % per for q in range(n)] and max(nums) > 2 ** 32
            keys, sa = [bytes(key_len)] * (2 * n_sa), Sa(2 * n_sa, 1)
            for s in range(n_sa):
                keys[n_sa + s], salt = IK.child_sa(hl, sk[hl * s:hl * s + hl], nonces[1][s], key_len)[IK.I2R]
                sa.salt[n_sa + s] = salt + bytes(4)
            numbered = [f[:4] + struct.pack(">I", x & 0xFFFFFFFF) + f[8:] for f, x in zip(plain, nums)]
            wire = x_ref_encrypt(evp, key_len, b"".join(keys), sa, xf, [n_sa + s for s in sas], [x >> 32 for x in nums], numbered)
            assert wire_got == _layout(wire, 5)[1]                              # libcrypto under ikev2_ref's key and salt and the assigned numbers: the same frames
            assert list(struct.unpack("<%dQ" % n, bytes(d["rnum"].download(8 * n)))) == nums
            assert list(struct.unpack("<%di" % n, bytes(d["auth"].download(4 * n)))) == [1] * n
            back = bytes(d["buf"].download(len(buf)))
            assert [back[off[q]:off[q + 1] - 16] for q in range(n)] == [f[:-16] for f in numbered]
            assert rw.get()[0] == [start + per] * n_sa == tc.get()[0]
            assert it.status() == (hip.OK, 0) and tx.status() == (hip.OK, 0) and rx.status() == (hip.OK, 0) and tc.status() == (hip.OK, 0)
        finally:
            for x in d.values():
                x.free()
    G.stream_destroy(st)
