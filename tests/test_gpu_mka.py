"""GPU: MACsec's MKA on the device (aesgcm_mka_*).  CAKs, KEKs and SAKs cannot be read back, so every installed slot is checked through what it DOES: MACsec frames are
encrypted on the GPU under the slots (KeyTable.crypt_frames, WireFormat.macsec) and must equal, every byte, what the wire fixture makes over libcrypto under the SAK
that mka_ref derives (AES-CMAC KDF over libcrypto's AES); the wrapped SAKs, which are public, are compared byte for byte with libcrypto's AES_wrap_key of the same.
  slots        the four (cak_len, key_len) pairs at 1 / 257 / 4097 entries (below a workgroup, one lane into the second, one into the seventeenth), indices and slots
               permuted, the arrays, the byte-packed contexts and the wrapped output between guard bytes
  contexts     one call: context lengths 1 .. 48, 2048 and key_len + 12 k + 4 for k = 1, 2, 30, byte-packed: one and two iterations, K1 (len % 16 == 0) against K2,
               a context that ends one byte into a block (len % 16 == 3), the 2048 bound, every start alignment
  two stations a key server's install with wrap feeds a second CakTable and key table whose unwrap takes those bytes on the device; the peer decrypts the server's
               frames with auth 1: both NR of the inverse cipher, both SAK sizes
  corrupted    verdict 2, an older key in the slot still at work, a fresh slot unset (its frame refused), the lowest index in status(), the neighbours installed;
               verdicts 0 / 1 / 2 mixed in one call; d_verdict NULL
  refusals     index out of range, unset, cleared, slot out of range, falling offsets, empty and over-long context: nothing an entry names is written
  shared       many entries on one record, d_wrapped NULL
  key size     a 24-byte key table is AESGCM_EARG
  capture      install + encrypt and unwrap + decrypt, each in one linear graph replayed three times over changed contexts
  rekey        TxCounters refuses at PN exhaustion, install with KN + 1 into the next AN's slot, set_salt, counter reset, encrypt; the peer unwraps, then RxWindows:
               launches on one stream"""
import random
import struct

import pytest

import hip_graph as G
import mka_ref as M
import pkt_grid as PG
from kt_common import Guarded, _layout, _u32, _u64, _up, evp, wire_ref_encrypt  # noqa: F401
from util import splitmix_bytes

pytestmark = pytest.mark.gpu

PAIRS = [(16, 16), (16, 32), (32, 16), (32, 32)]                             # (cak_len, key_len)
INSTALLED, REFUSED, BAD_ICV = 0, 1, 2


def _frame(i):
    """a MACsec frame before protection: DA SA | SecTAG with SCI (PN at byte 16) | user data | 16 placeholder bytes"""
    return splitmix_bytes(7100 + i, 28 + 5 + i % 23) + bytes(16)


def _salts(kt, seed):
    """an SCI in every slot's salt field: install and unwrap leave it alone"""
    b = splitmix_bytes(seed, 8 * kt.n_slots)
    kt.set_salt(0, b)
    return [b[8 * s:8 * s + 8] for s in range(kt.n_slots)]


def _check(hip, evp, kt, salts, held, label=""):  # noqa: F811
    """held: {slot: key} -- one MACsec frame per slot on the GPU against libcrypto under that key and the slot's SCI, every byte"""
    slots = sorted(held)
    keys = b"".join(held.get(s, bytes(kt.key_len)) for s in range(kt.n_slots))
    frames = [_frame(i) for i in range(len(slots))]
    fmt = hip.WireFormat.macsec()
    got, _ = kt.crypt_frames(fmt, slots, frames)
    want = wire_ref_encrypt(evp, kt.key_len, keys, salts, fmt, slots, frames)
    for i, s in enumerate(slots):
        assert bytes(got[i]) == want[i], (label, kt.key_len, "slot", s)
    assert kt.status() == (hip.OK, 0), label


def _offsets(ctxs):
    off = [0]
    for c in ctxs:
        off.append(off[-1] + len(c))
    return off


class _Cas:
    """n_caks CAKs with their CKNs, and the reference's view of them (the KEK once per CAK)"""

    def __init__(self, cak_len, n_caks, seed):
        b = splitmix_bytes(seed, cak_len * n_caks)
        self.caks = [b[cak_len * i:cak_len * (i + 1)] for i in range(n_caks)]
        self.ckns = [splitmix_bytes(seed + 1 + i, 1 + (i * 7) % 32) for i in range(n_caks)]
        self._kek = {}

    def into(self, table):
        table.set(0, self.caks, self.ckns)
        return table

    def kek(self, i):
        if i not in self._kek:
            self._kek[i] = M.kek(self.caks[i], self.ckns[i])
        return self._kek[i]

    def sak(self, i, ctx, key_len):
        return M.sak(self.caks[i], ctx, key_len)

    def wrapped(self, i, ctx, key_len):
        return M.wrap(self.kek(i), self.sak(i, ctx, key_len))


# ---------------------------------------------------------------- slots
@pytest.mark.parametrize("n", [1, 257, 4097])
@pytest.mark.parametrize("cak_len,key_len", PAIRS)
def test_install_between_guards(hip, evp, cak_len, key_len, n):  # noqa: F811
    """slots 0 and n + 1 are set by hand and never named; the arrays, the contexts and the wrapped output lie between guard bytes"""
    rng = random.Random("mka %d %d %d" % (cak_len, key_len, n))
    n_caks = max(1, n // 3)
    ca = _Cas(cak_len, n_caks, n + cak_len + key_len)
    ctxs = [splitmix_bytes(91000 + 7 * i + n, rng.randrange(key_len + 16, key_len + 65)) for i in range(n)]
    idx, slots = [rng.randrange(n_caks) for _ in range(n)], list(range(1, n + 1))
    rng.shuffle(slots)
    w = key_len + 8
    with hip.CakTable(cak_len, n_caks) as ct, hip.KeyTable(key_len, n + 2) as kt:
        ca.into(ct)
        salts = _salts(kt, 17 + n)
        held = {s: splitmix_bytes(5 + e, key_len) for e, s in enumerate((0, n + 1))}
        for s, k in held.items():
            kt.set(s, k)
        data = (_u32(idx), b"".join(ctxs), _u32(_offsets(ctxs)), _u32(slots))
        g = [Guarded(hip, len(d)) for d in data]
        for gb, d in zip(g, data):
            gb.buf.upload(d, PG.GUARD)
        gw = Guarded(hip, n * w + 1)                                            # (+ 1: the output starts at an odd address)
        ct.install_dev(kt, n, g[0].ptr, g[1].ptr, g[2].ptr, g[3].ptr, gw.ptr + 1)
        hip.dev_sync()
        assert [gb.read("array") for gb in g] == list(data)
        assert ct.status() == (hip.OK, 0)
        got = gw.read("wrapped")
        assert got[:1] == b"\xA7"
        for i in range(n):
            assert got[1 + i * w:1 + (i + 1) * w] == ca.wrapped(idx[i], ctxs[i], key_len), i
            held[slots[i]] = ca.sak(idx[i], ctxs[i], key_len)
        _check(hip, evp, kt, salts, held, "n=%d" % n)
        for gb in g + [gw]:
            gb.buf.free()


# ---------------------------------------------------------------- context lengths and alignments
@pytest.mark.parametrize("cak_len,key_len", PAIRS)
def test_context_lengths_byte_packed(hip, evp, cak_len, key_len):  # noqa: F811
    lens = list(range(1, 49)) + [2048] + [key_len + 12 * k + 4 for k in (1, 2, 30)]
    ctxs = [splitmix_bytes(300 + n, n) for n in lens]
    n = len(ctxs)
    off = _offsets(ctxs)
    assert {o % 16 for o in off[:-1]} == set(range(16)) and {x % 16 for x in lens} >= {0, 1, 3, 15}
    ca = _Cas(cak_len, 1, 77 + cak_len)
    with hip.CakTable(cak_len, 1) as ct, hip.KeyTable(key_len, n) as kt:
        ca.into(ct)
        salts = _salts(kt, 31)
        wrapped = ct.install(kt, [0] * n, ctxs, list(range(n)), wrapped=True)
        assert ct.status() == (hip.OK, 0)
        assert [bytes(x) for x in wrapped] == [ca.wrapped(0, c, key_len) for c in ctxs]
        _check(hip, evp, kt, salts, {i: ca.sak(0, ctxs[i], key_len) for i in range(n)}, "lengths")


# ---------------------------------------------------------------- two stations
@pytest.mark.parametrize("cak_len,key_len", PAIRS)
def test_key_server_and_peer(hip, evp, cak_len, key_len):  # noqa: F811
    """the wrapped SAKs never leave the device between the server's install and the peer's unwrap; the peer's table holds the same CAKs under other indices"""
    n, n_caks, w = 300, 7, key_len + 8
    ca = _Cas(cak_len, n_caks, 500 + cak_len + key_len)
    ctxs = [hip.mka_sak_context(splitmix_bytes(600 + i, key_len), [splitmix_bytes(700 + i + m, 12) for m in range(1 + i % 4)], i + 1) for i in range(n)]
    idx = [i % n_caks for i in range(n)]
    fmt = hip.WireFormat.macsec()
    frames = [_frame(i) for i in range(n)]
    with hip.CakTable(cak_len, n_caks) as server, hip.CakTable(cak_len, n_caks + 1) as peer, hip.KeyTable(key_len, n) as tx, hip.KeyTable(key_len, n) as rx:
        ca.into(server)
        peer.set(1, ca.caks, ca.ckns)                                           # record 0 stays unset
        sci = splitmix_bytes(41, 8 * n)
        tx.set_salt(0, sci)
        rx.set_salt(0, sci)
        d = {k: _up(hip, v) for k, v in (("idx", _u32(idx)), ("pidx", _u32([x + 1 for x in idx])), ("ctx", b"".join(ctxs)), ("off", _u32(_offsets(ctxs))),
                                         ("slots", _u32(list(range(n)))), ("rslots", _u32(list(reversed(range(n))))), ("wrapped", bytes(n * w)))}
        gv = Guarded(hip, n)
        try:
            server.install_dev(tx, n, d["idx"].ptr, d["ctx"].ptr, d["off"].ptr, d["slots"].ptr, d["wrapped"].ptr)
            peer.unwrap_dev(rx, n, d["pidx"].ptr, d["wrapped"].ptr, d["rslots"].ptr, gv.ptr)
            hip.dev_sync()
            assert gv.read("verdicts") == bytes([INSTALLED]) * n
            assert server.status() == (hip.OK, 0) and peer.status() == (hip.OK, 0)
            wire, _ = tx.crypt_frames(fmt, list(range(n)), frames)
            salts = [sci[8 * s:8 * s + 8] for s in range(n)]
            want = wire_ref_encrypt(evp, key_len, b"".join(ca.sak(idx[i], ctxs[i], key_len) for i in range(n)), salts, fmt, list(range(n)), frames)
            assert [bytes(f) for f in wire] == want
            # the peer's slot for SC i is n - 1 - i: the same SCI there
            rx.set_salt(0, b"".join(reversed(salts)))
            back, auth = rx.crypt_frames(fmt, list(reversed(range(n))), wire, decrypt=True)
            assert list(auth) == [1] * n
            assert [bytes(b)[:-16] for b in back] == [f[:-16] for f in frames]
        finally:
            for x in d.values():
                x.free()
            gv.buf.free()


# ---------------------------------------------------------------- corrupted wraps, verdicts
@pytest.mark.parametrize("verdicts", [True, False])
@pytest.mark.parametrize("cak_len,key_len", [(16, 32), (32, 16)])
def test_corrupted_wraps_and_mixed_verdicts(hip, evp, cak_len, key_len, verdicts):  # noqa: F811
    """slots 0 .. n / 2 - 1 hold an older key, the rest are fresh; verdicts False: d_verdict is NULL and the status word alone reports"""
    n, w = 257, key_len + 8
    ca = _Cas(cak_len, n + 2, 800 + cak_len)
    ctxs = [splitmix_bytes(900 + i, key_len + 16) for i in range(n)]
    idx, slots = list(range(n)), list(range(n))
    wrapped = [bytearray(ca.wrapped(i, ctxs[i], key_len)) for i in range(n)]
    corrupt = {9: 0, 64: 8 * w - 1, 130: 63, 131: 64, 255: 8 * 8 + 5, 256: 3}                 # entry: the bit flipped (in A, in the key, the last bit)
    for i, bit in corrupt.items():
        wrapped[i][bit // 8] ^= 0x80 >> (bit % 8)
    idx[17], idx[70], idx[200] = n + 5, n + 1, 100                             # out of range; unset; cleared (below)
    slots[40], slots[201] = n, 0xFFFFFFFF                                       # slot out of range
    named = {17, 70, 100, 200, 40, 201}                                         # (entry 100 names the cleared record too)
    want = [BAD_ICV if i in corrupt else REFUSED if i in named else INSTALLED for i in range(n)]
    old = {s: splitmix_bytes(1000 + s, key_len) for s in range(n // 2)}
    fmt = hip.WireFormat.macsec()
    with hip.CakTable(cak_len, n + 2) as ct, hip.KeyTable(key_len, n) as kt:
        ct.set(0, ca.caks[:n + 1], ca.ckns[:n + 1])                             # record n + 1 stays unset
        ct.clear(100)
        salts = _salts(kt, 51)
        kt.set(0, b"".join(old[s] for s in range(n // 2)))
        d = {k: _up(hip, v) for k, v in (("idx", _u32(idx)), ("wrapped", b"".join(bytes(x) for x in wrapped)), ("slots", _u32(slots)))}
        gv = Guarded(hip, n)
        try:
            ct.unwrap_dev(kt, n, d["idx"].ptr, d["wrapped"].ptr, d["slots"].ptr, gv.ptr if verdicts else None)
            hip.dev_sync()
            got = gv.read("verdicts")
            assert got == (bytes(want) if verdicts else b"\xA7" * n)
            assert ct.status() == (hip.EARG, 9) and ct.status() == (hip.OK, 0)  # the lowest index; reading clears
            assert kt.status() == (hip.OK, 0)                                   # the key table's status word is not touched
            held = dict(old)                                                    # a slot that held an older key still encrypts under it
            for i in range(n):
                if want[i] == INSTALLED:
                    held[slots[i]] = ca.sak(idx[i], ctxs[i], key_len)           # the neighbours install
            assert all(held[s] == old[s] for s in (9, 17, 40, 64, 70, 100)) and held[8] != old[8] and held[10] != old[10]
            _check(hip, evp, kt, salts, held, "corrupted")
            for s in (130, 131, 200, 255, 256):                                 # a fresh slot stays unset: the crypt call refuses its frame
                kt.crypt_frames(fmt, [s], [_frame(s)])
                assert kt.status() == (hip.EARG, 0), s
        finally:
            for x in d.values():
                x.free()
            gv.buf.free()


# ---------------------------------------------------------------- install's refusals
@pytest.mark.parametrize("cak_len,key_len", [(16, 16), (32, 32)])
def test_install_refusals_scattered_through_257_entries(hip, evp, cak_len, key_len):  # noqa: F811
    """every refusal kind in one call: skipped whole -- the slot keeps its old key, the entry's wrapped bytes keep the guard's fill"""
    n, w = 257, key_len + 8
    ca = _Cas(cak_len, n + 2, 1100 + cak_len)
    ctxs = [splitmix_bytes(1200 + i, 2049 if i == 40 else key_len + 16 + i % 50) for i in range(n)]       # entry 40: one byte too long
    packed, off = b"".join(ctxs), _offsets(ctxs)
    off[121] = off[120]                                                         # entry 120: empty (121 starts there and is longer for it)
    off[151] = off[150] - 10                                                    # entry 150: falling (151 starts ten bytes early)
    ctx_of = lambda i: packed[off[i]:off[i + 1]]
    idx, slots = list(range(n)), list(range(n))
    idx[17], idx[64] = n + 2, n + 1                                              # out of range; unset
    slots[200], slots[230] = n, 0xFFFFFFFF                                       # a slot out of range
    bad = {17, 40, 64, 100, 120, 150, 200, 230}
    old = {s: splitmix_bytes(1300 + s, key_len) for s in range(n)}
    with hip.CakTable(cak_len, n + 2) as ct, hip.KeyTable(key_len, n) as kt:
        ct.set(0, ca.caks[:n + 1], ca.ckns[:n + 1])                             # record n + 1 stays unset
        ct.clear(100)                                                           # cleared
        salts = _salts(kt, 61)
        kt.set(0, b"".join(old[s] for s in range(n)))
        d = {k: _up(hip, v) for k, v in (("idx", _u32(idx)), ("ctx", packed), ("off", _u32(off)), ("slots", _u32(slots)))}
        gw = Guarded(hip, n * w)
        try:
            ct.install_dev(kt, n, d["idx"].ptr, d["ctx"].ptr, d["off"].ptr, d["slots"].ptr, gw.ptr)
            hip.dev_sync()
            assert ct.status() == (hip.EARG, 17) and ct.status() == (hip.OK, 0)
            assert kt.status() == (hip.OK, 0)
            got = gw.read("wrapped")
            held = dict(old)
            for i in range(n):
                if i in bad:
                    assert got[i * w:(i + 1) * w] == b"\xA7" * w, i            # a refused entry's bytes there are not written
                else:
                    assert got[i * w:(i + 1) * w] == ca.wrapped(idx[i], ctx_of(i), key_len), i
                    held[slots[i]] = ca.sak(idx[i], ctx_of(i), key_len)
            _check(hip, evp, kt, salts, held, "refusals")
        finally:
            for x in d.values():
                x.free()
            gw.buf.free()


# ---------------------------------------------------------------- many entries on one record, no wrapped output
def test_many_entries_share_one_record_without_wrapped_output(hip, evp):  # noqa: F811
    n, cak_len, key_len = 300, 32, 16
    ca = _Cas(cak_len, 2, 1400)
    ctxs = [splitmix_bytes(1500 + i, 48) for i in range(n)]
    idx = [0 if i % 7 else 1 for i in range(n)]
    with hip.CakTable(cak_len, 2) as ct, hip.KeyTable(key_len, n) as kt:
        ca.into(ct)
        salts = _salts(kt, 71)
        assert ct.install(kt, idx, ctxs, list(range(n))) is ct                  # d_wrapped NULL
        held = {i: ca.sak(idx[i], ctxs[i], key_len) for i in range(n)}
        assert len(set(held.values())) == n
        _check(hip, evp, kt, salts, held, "shared")
        # one SAK for several SCs: several slots are several entries of one context
        ct.install(kt, [1] * 5, [ctxs[0]] * 5, [10, 20, 30, 40, 50])
        held.update({s: ca.sak(1, ctxs[0], key_len) for s in (10, 20, 30, 40, 50)})
        _check(hip, evp, kt, salts, held, "one SAK, five SCs")
        assert ct.status() == (hip.OK, 0)


# ---------------------------------------------------------------- MACsec has no AES-192
def test_key_table_of_24_byte_keys_is_an_argument_error(hip):
    with hip.CakTable(16, 1) as ct, hip.KeyTable(24, 4) as kt:
        ct.set(0, bytes(16), [b"ckn"])
        b = _up(hip, bytes(64))
        try:
            for call in (lambda: ct.install_dev(kt, 1, b.ptr, b.ptr, b.ptr, b.ptr, None), lambda: ct.unwrap_dev(kt, 1, b.ptr, b.ptr, b.ptr, None)):
                with pytest.raises(hip.AesGcmError) as e:
                    call()
                assert e.value.code == hip.EARG
            hip.dev_sync()
            assert ct.status() == (hip.OK, 0) and kt.status() == (hip.OK, 0)
        finally:
            b.free()


# ---------------------------------------------------------------- capture
def test_captured_install_encrypt_and_unwrap_decrypt_replay_over_changed_contexts(hip, evp):  # noqa: F811
    n, cak_len, key_len = 100, 16, 32
    w = key_len + 8
    ca = _Cas(cak_len, n, 1600)
    gens = [[splitmix_bytes(2000 * g + i, 48) for i in range(n)] for g in range(3)]
    frames = [_frame(p) for p in range(n)]
    off, buf = _layout(frames, 0, 0)
    fmt = hip.WireFormat.macsec()
    perm = list(range(n))
    random.Random(6).shuffle(perm)
    st = G.stream_create()
    with hip.CakTable(cak_len, n) as server, hip.CakTable(cak_len, n) as peer, hip.KeyTable(key_len, n) as tx, hip.KeyTable(key_len, n) as rx:
        ca.into(server)
        ca.into(peer)
        sci = splitmix_bytes(81, 8 * n)
        tx.set_salt(0, sci)
        rx.set_salt(0, sci)
        hip.dev_sync()
        d = {k: _up(hip, v) for k, v in (("idx", _u32(perm)), ("slots", _u32(perm)), ("coff", _u32([48 * i for i in range(n + 1)])), ("ctx", b"".join(gens[0])),
                                         ("pslots", _u32(list(range(n)))), ("off", _u64(off)), ("in", buf), ("wire", bytes(len(buf))), ("back", bytes(len(buf))),
                                         ("wrapped", bytes(n * w)), ("verdict", b"\x07" * n), ("auth", b"\x07" * 4 * n))}
        p = lambda k: d[k].ptr

        def send():
            server.install_dev(tx, n, p("idx"), p("ctx"), p("coff"), p("slots"), p("wrapped"), stream=st)
            tx.frames_crypt_dev(0, fmt, n, p("pslots"), p("in"), p("off"), p("wire"), stream=st)

        def receive():
            peer.unwrap_dev(rx, n, p("idx"), p("wrapped"), p("slots"), p("verdict"), stream=st)
            rx.frames_crypt_dev(1, fmt, n, p("pslots"), p("wire"), p("off"), p("back"), d_auth=p("auth"), stream=st)

        try:
            send()                                                              # the ordinary call of each
            receive()
            G.synchronize(st)
            with G.Graph(st, send) as gs, G.Graph(st, receive) as gr:
                for g in range(3):
                    d["ctx"].upload(b"".join(gens[g]))                          # outside the capture: entry i's context belongs to record and slot perm[i]
                    gs.launch()
                    wire = bytes(d["wire"].download(len(buf)))
                    keys = [None] * n
                    for i in range(n):
                        keys[perm[i]] = ca.sak(perm[i], gens[g][i], key_len)
                    want = wire_ref_encrypt(evp, key_len, b"".join(keys), [sci[8 * s:8 * s + 8] for s in range(n)], fmt, list(range(n)), frames)
                    assert wire == b"".join(want), g
                    assert bytes(d["wrapped"].download(n * w)) == b"".join(ca.wrapped(perm[i], gens[g][i], key_len) for i in range(n)), g
                    d["verdict"].upload(b"\x07" * n)
                    d["auth"].upload(b"\x07" * 4 * n)
                    gr.launch()
                    assert bytes(d["verdict"].download(n)) == bytes(n), g
                    assert list(struct.unpack("<%di" % n, bytes(d["auth"].download(4 * n)))) == [1] * n, g
                    back = bytes(d["back"].download(len(buf)))
                    assert [back[off[q]:off[q + 1] - 16] for q in range(n)] == [f[:-16] for f in frames], g
            assert server.status() == (hip.OK, 0) and peer.status() == (hip.OK, 0) and tx.status() == (hip.OK, 0) and rx.status() == (hip.OK, 0)
        finally:
            for x in d.values():
                x.free()
    G.stream_destroy(st)


# ---------------------------------------------------------------- the rekey loop on one stream
def test_rekey_loop_across_pn_exhaustion_on_one_stream(hip, evp):  # noqa: F811
    """a key server's sending side and a peer's receiving side, n_sc secure channels.  Generation 0 (KN 1, AN 0: slots 0 .. n_sc - 1) runs its counters into 2^32, where
    assign refuses; the rekey installs the SAK of KN 2 into the next AN's slots (n_sc ..), sets their SCIs, resets the counters, and the frames go out; the peer unwraps
    the distributed SAK into its own next slots and takes the frames through its windows"""
    n_sc, per, cak_len, key_len, W = 5, 6, 16, 16, 64
    n, w = n_sc * per, key_len + 8
    ca = _Cas(cak_len, 1, 1700)
    mis = [splitmix_bytes(1710 + m, 12) for m in range(3)]
    ctx = [hip.mka_sak_context(splitmix_bytes(1720 + kn, key_len), mis, kn) for kn in (1, 2)]
    fmt, tf, rf = hip.WireFormat.macsec(), hip.TxFormat.macsec(), hip.RxFormat.macsec()
    scs = [q // per for q in range(n)]
    plain = [splitmix_bytes(1800 + q, 28 + 9 + q % 31) + b"\xAA" * 16 for q in range(n)]
    off, buf = _layout(plain, 5)
    sci = splitmix_bytes(1730, 8 * n_sc)
    st = G.stream_create()
    with hip.CakTable(cak_len, 1) as server, hip.CakTable(cak_len, 1) as peer, hip.KeyTable(key_len, 2 * n_sc) as tx, hip.KeyTable(key_len, 2 * n_sc) as rx, \
            hip.TxCounters(n_sc, n) as tc, hip.RxWindows(n_sc, W) as rw:
        ca.into(server)
        ca.into(peer)
        tx.set(0, bytes(key_len))
        rx.set(0, bytes(key_len))                                               # one ordinary call per table before the loop (per-device state)
        hip.dev_sync()
        d = {k: _up(hip, v) for k, v in (("zero", _u32([0] * n_sc)), ("an0", _u32(list(range(n_sc)))), ("an1", _u32([n_sc + s for s in range(n_sc)])),
                                         ("ctx0", ctx[0] * n_sc), ("ctx1", b"\xEE" + ctx[1] * n_sc), ("coff", _u32([len(ctx[0]) * s for s in range(n_sc + 1)])),
                                         ("ctr", _u32(scs)), ("slots", _u32(scs)), ("slots1", _u32([n_sc + s for s in scs])), ("off", _u64(off)), ("buf", buf),
                                         ("num", bytes(8 * n)), ("rnum", bytes(8 * n)), ("auth", b"\x07" * 4 * n), ("why", b"\x07" * 4 * n),
                                         ("wrapped", bytes(n_sc * w)), ("verdict", b"\x07" * n_sc))}
        p = lambda k: d[k].ptr
        try:
            # generation 0: the SAK of KN 1 in the slots of AN 0; every counter stands at 2^32, so assign refuses every frame
            server.install_dev(tx, n_sc, p("zero"), p("ctx0"), p("coff"), p("an0"), None, stream=st)
            tc.set(0, [2 ** 32] * n_sc, [2 ** 64 - 1] * n_sc, stream=st)
            tc.assign_dev(tf, n, p("ctr"), p("buf"), p("off"), p("num"), None, p("slots"), stream=st)
            G.synchronize(st)
            assert tc.status() == (hip.EARG, 0)                                 # PN exhaustion: time to rekey
            assert list(struct.unpack("<%dI" % n, bytes(d["slots"].download(4 * n)))) == [0xFFFFFFFF] * n
            # the rekey: KN 2 (the context at an odd address) into the next AN's slots with wrap, the SCIs, the counters back to 1, then the traffic
            server.install_dev(tx, n_sc, p("zero"), p("ctx1") + 1, p("coff"), p("an1"), p("wrapped"), stream=st)
            tx.set_salt(n_sc, sci, stream=st)
            tc.set(0, [1] * n_sc, [2 ** 32] * n_sc, stream=st)
            tc.assign_dev(tf, n, p("ctr"), p("buf"), p("off"), p("num"), None, p("slots1"), stream=st)
            tx.frames_crypt_dev(0, fmt, n, p("slots1"), p("buf"), p("off"), p("buf"), stream=st)
            # the peer: the distributed SAK into its next slots, their SCIs, the windows back to 1, then the frames
            peer.unwrap_dev(rx, n_sc, p("zero"), p("wrapped"), p("an1"), p("verdict"), stream=st)
            rx.set_salt(n_sc, sci, stream=st)
            rw.set(0, [1] * n_sc, stream=st)
            G.synchronize(st)
            wire_got = bytes(d["buf"].download(len(buf)))
            rw.recover_dev(rf, n, p("ctr"), p("buf"), p("off"), p("rnum"), None, stream=st)
            rx.frames_crypt_dev(1, fmt, n, p("slots1"), p("buf"), p("off"), p("buf"), d_auth=p("auth"), stream=st)
            rw.commit_dev(n, p("ctr"), p("rnum"), p("auth"), p("auth"), p("why"), stream=st)
            G.synchronize(st)
            nums = list(struct.unpack("<%dQ" % n, bytes(d["num"].download(8 * n))))
            assert nums == [1 + q % per for q in range(n)]
            sak1 = ca.sak(0, ctx[1], key_len)
            assert bytes(d["wrapped"].download(n_sc * w)) == ca.wrapped(0, ctx[1], key_len) * n_sc and bytes(d["verdict"].download(n_sc)) == bytes(n_sc)
            numbered = [f[:16] + struct.pack(">I", x) + f[20:] for f, x in zip(plain, nums)]
            salts = [bytes(8)] * n_sc + [sci[8 * s:8 * s + 8] for s in range(n_sc)]
            wire = wire_ref_encrypt(evp, key_len, bytes(key_len) * n_sc + sak1 * n_sc, salts, fmt, [n_sc + s for s in scs], numbered)
            assert wire_got == _layout(wire, 5)[1]                              # libcrypto under mka_ref's SAK and the assigned numbers: the same frames
            assert list(struct.unpack("<%dQ" % n, bytes(d["rnum"].download(8 * n)))) == nums
            assert list(struct.unpack("<%di" % n, bytes(d["auth"].download(4 * n)))) == [1] * n
            back = bytes(d["buf"].download(len(buf)))
            assert [back[off[q]:off[q + 1] - 16] for q in range(n)] == [f[:-16] for f in numbered]
            assert rw.get()[0] == [1 + per] * n_sc == tc.get()[0]
            assert server.status() == (hip.OK, 0) and peer.status() == (hip.OK, 0) and tx.status() == (hip.OK, 0) and rx.status() == (hip.OK, 0) and tc.status() == (hip.OK, 0)
        finally:
            for x in d.values():
                x.free()
    G.stream_destroy(st)
