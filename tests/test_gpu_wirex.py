"""GPU: wire frames with 64-bit numbers (aesgcm_keytab_frames_crypt_x_dev) -- MACsec XPN (IEEE 802.1AEbw: nonce = salt96 XOR (SSCI32 | PN64), the PN's upper half not
in the frame) and ESP with extended sequence numbers (RFC 4303 / RFC 4106 section 5: AAD = SPI | seq-hi | seq-lo, seq-hi not in the frame).  The oracle is libcrypto
(oracle/evp_batch.c, evp_frames_crypt): nonce and AAD of every frame are built here from the standards' formulas in plain Python and handed over as IV and AAD arrays.
Random populations, every byte of the buffer compared, canaries included; where the number goes; the XPN state's life cycle and stream ordering; refusals; and, labelled
as such, two comparisons of the library with itself (ext 0 against the base call, XPN with a zero salt against the classic MACsec nonce).
No published XPN vector is among the fixtures, so none is used."""
import random
import struct

import pytest

from kt_common import CANARY, _collect, _layout, _u32, _u64, _up, evp  # noqa: F401
from kt_common import Sa, x_ref_encrypt as _ref_encrypt
from util import splitmix_bytes

pytestmark = pytest.mark.gpu


def _make_frames(rng, xf, n, seed, max_payload=1514, aligned=False):
    """n plaintext frames: random header, random payload of 0 .. max_payload bytes (aligned: the frame a multiple of 16 bytes), the ICV's bytes as placeholders"""
    hdr_len, tag_len = xf.f.hdr_len, xf.f.tag_len
    lens = [rng.randrange(0, max_payload + 1) for _ in range(n)]
    for i, x in enumerate((0, 1, 15, 16, 17, max_payload)):
        if i < n:
            lens[-1 - i] = x
    if aligned:
        lens = [x + (-(hdr_len + x + tag_len)) % 16 for x in lens]
    blob = splitmix_bytes(seed, sum(lens) + n * hdr_len)
    frames, at = [], 0
    for x in lens:
        frames.append(blob[at:at + hdr_len + x] + b"\xAA" * tag_len)
        at += hdr_len + x
    return frames


def _make_his(rng, n):
    """random upper halves; the two ends of the range are always among them"""
    his = [rng.getrandbits(32) for _ in range(n)]
    his[0] = 0
    his[-1] = 0xFFFFFFFF
    if n > 2:
        his[n // 2] = 0xFFFFFFFF
        his[1] = 0
    return his


def _run(hip, kt, decrypt, xf, slots, his, off, buf, inplace, out_fill=CANARY, sync=True):
    n = len(slots)
    d = {"slots": _up(hip, _u32(slots)), "in": _up(hip, buf), "off": _up(hip, _u64(off)), "hi": _up(hip, _u32(his)) if his is not None else None}
    d["out"] = d["in"] if inplace else _up(hip, bytes([out_fill]) * len(buf))
    d["auth"] = _up(hip, b"\x07" * 4 * n) if decrypt else None
    kt.frames_crypt_x_dev(decrypt, xf, n, d["slots"].ptr, d["hi"].ptr if his is not None else None, d["in"].ptr, d["off"].ptr, d["out"].ptr,
                          d_auth=d["auth"].ptr if decrypt else None)
    d["nbytes"], d["n"] = len(buf), n
    return _collect(hip, d) if sync else d


def _table(hip, key_len, n_slots, seed):
    keys = splitmix_bytes(seed, key_len * n_slots)
    sa = Sa(n_slots, seed + 1)
    kt = hip.KeyTable(key_len, n_slots)
    kt.set(0, keys)
    kt.set_salt(0, b"".join(sa.salt))
    kt.set_xpn(0, b"".join(sa.xsalt), b"".join(sa.ssci))
    return kt, keys, sa


def _fmt_of(hip, name):
    X = hip.WireFormatX
    return {"xpn": lambda: X.macsec_xpn(), "xpn_nosci": lambda: X.macsec_xpn(sci=False), "xpn_auth": lambda: X.macsec_xpn(sci=False, auth_only=True),
            "xpn_auth_sci": lambda: X.macsec_xpn(sci=True, auth_only=True),
            "esn16": lambda: X.esp_esn(16), "esn12": lambda: X.esp_esn(12), "esn8": lambda: X.esp_esn(8)}[name]()


def _both_ways(hip, evp, kt, keys, sa, key_len, xf, slots, his, frames, lead, inplace):
    """encrypt against libcrypto, every byte of the buffer; then libcrypto's frames back to the plaintext with every ICV accepted (the ICV's bytes stay)"""
    n = len(frames)
    off, buf = _layout(frames, lead)
    want = _ref_encrypt(evp, key_len, keys, sa, xf, slots, his, frames)
    _, want_buf = _layout(want, off[0])
    out, _, _ = _run(hip, kt, False, xf, slots, his, off, buf, inplace)
    if out != want_buf:                                                  # name the first frame that differs
        for p in range(n):
            assert out[off[p]:off[p + 1]] == want[p], (p, len(frames[p]), his[p])
    assert out == want_buf
    back, auth, _ = _run(hip, kt, True, xf, slots, his, off, want_buf, inplace)
    tl = xf.f.tag_len
    _, plain_buf = _layout([f[:-tl] + w[-tl:] for f, w in zip(frames, want)], off[0])
    assert back == plain_buf
    assert auth == [1] * n
    assert kt.status() == (hip.OK, 0)


# ---------------------------------------------------------------- 1. random populations against libcrypto, every byte compared
POPULATIONS = [
    # key_len, format, frames, slots, aligned, in place
    (16, "xpn", 1, 1, False, True),
    (24, "xpn", 63, 7, True, False),
    (32, "xpn", 4097, 64, False, False),
    (16, "xpn_nosci", 4097, 64, True, True),
    (24, "xpn_auth", 4097, 16, False, False),
    (32, "xpn_auth_sci", 63, 3, True, True),
    (16, "esn16", 4097, 64, False, True),
    (24, "esn12", 4097, 33, True, False),
    (32, "esn8", 63, 5, False, True),
    (24, "esn8", 1, 2, True, False),
    (32, "xpn", 300000, 64, False, True),             # the launch ordered by falling frame length class
    (16, "esn16", 300000, 64, False, False),
]


@pytest.mark.parametrize("key_len, fmt_name, n, n_slots, aligned, inplace", POPULATIONS)
def test_random_frames_vs_libcrypto(hip, evp, key_len, fmt_name, n, n_slots, aligned, inplace):
    rng = random.Random("x %d %s %d" % (key_len, fmt_name, n))
    xf = _fmt_of(hip, fmt_name)
    kt, keys, sa = _table(hip, key_len, n_slots, 0x1F00 + key_len + n)
    try:
        slots = [rng.randrange(n_slots) for _ in range(n)]
        slots[0], slots[-1] = 0, n_slots - 1
        frames = _make_frames(rng, xf, n, 0x1F10 + n + key_len, aligned=aligned)
        _both_ways(hip, evp, kt, keys, sa, key_len, xf, slots, _make_his(rng, n), frames, 32 if aligned else 13, inplace)
    finally:
        kt.close()


@pytest.mark.parametrize("lanes", [8, 16, 64])
@pytest.mark.parametrize("fmt_name, key_len", [("xpn", 32), ("esn12", 24), ("xpn_auth", 16), ("esn16", 32)])
def test_forced_shapes_vs_libcrypto(hip, evp, lanes, fmt_name, key_len):
    """every kernel shape on one small population (the debug build's batch_lanes knob)"""
    with hip.debug_library() as dbg:
        dbg.force(batch_lanes=lanes)
        rng = random.Random("shape %d %s" % (lanes, fmt_name))
        xf = _fmt_of(hip, fmt_name)
        n, n_slots = 300, 9
        kt, keys, sa = _table(hip, key_len, n_slots, 0x1E00 + lanes)
        try:
            slots = [rng.randrange(n_slots) for _ in range(n)]
            frames = _make_frames(rng, xf, n, 0x1E10 + lanes, max_payload=700)
            _both_ways(hip, evp, kt, keys, sa, key_len, xf, slots, _make_his(rng, n), frames, 7, lanes == 16)
        finally:
            kt.close()


# ---------------------------------------------------------------- 2. the number goes where the standard says
def test_hi_enters_the_nonce_for_xpn_and_only_the_aad_for_esn(hip, evp):
    rng = random.Random(22)
    key_len, n_slots, n = 32, 8, 400
    kt, keys, sa = _table(hip, key_len, n_slots, 0x1D00)
    try:
        slots = [rng.randrange(n_slots) for _ in range(n)]
        his = [rng.randrange(0, 0xFFFFFFFF) for _ in range(n)]
        his[0], his[1] = 0, 0xFFFFFFFE
        his1 = [h + 1 for h in his]
        for name in ("xpn", "esn12"):
            xf = _fmt_of(hip, name)
            hdr, tl = xf.f.hdr_len, xf.f.tag_len
            frames = _make_frames(rng, xf, n, 0x1D10, max_payload=300)
            frames = [f if len(f) >= hdr + 16 + tl else f[:hdr] + b"\x11" * 16 + f[hdr:] for f in frames]         # at least one block of payload each
            off, buf = _layout(frames, 3)
            a, _, _ = _run(hip, kt, False, xf, slots, his, off, buf, True)
            b, _, _ = _run(hip, kt, False, xf, slots, his1, off, buf, True)
            for p in range(n):
                fa, fb = a[off[p]:off[p + 1]], b[off[p]:off[p + 1]]
                assert fa[:hdr] == fb[:hdr] == frames[p][:hdr]
                assert fa[-tl:] != fb[-tl:], (name, p)
                if name == "xpn":
                    assert fa[hdr:-tl] != fb[hdr:-tl], p                  # another nonce: another keystream
                else:
                    assert fa[hdr:-tl] == fb[hdr:-tl], p                  # the same nonce: the number is authenticated, nothing else
            # decrypt with a wrong number on chosen frames: exactly those fail
            wrong = {0, 1, 77, 200, n - 1}
            hisw = [(h ^ 0x00010000) if p in wrong else h for p, h in enumerate(his)]
            back, auth, _ = _run(hip, kt, True, xf, slots, hisw, off, a, False, out_fill=0x3C)
            assert auth == [0 if p in wrong else 1 for p in range(n)], name
            for p in range(n):
                if p not in wrong:
                    assert back[off[p]:off[p + 1] - tl] == frames[p][:-tl], p
            assert kt.status() == (hip.OK, 0)
    finally:
        kt.close()


# ---------------------------------------------------------------- 3. the XPN state: apart from the classic salt, zero when fresh and after clear, stream-ordered
def test_xpn_state_and_classic_salt_are_independent(hip, evp):
    rng = random.Random(33)
    key_len, n_slots, n = 16, 6, 200
    kt, keys, sa = _table(hip, key_len, n_slots, 0x1C00)
    try:
        slots = [rng.randrange(n_slots) for _ in range(n)]
        his = _make_his(rng, n)
        xf, base = _fmt_of(hip, "xpn"), hip.WireFormatX(hip.WireFormat.macsec(), 0, 0)
        frames = _make_frames(rng, xf, n, 0x1C10, max_payload=200)
        off, buf = _layout(frames, 9)
        want_x = _layout(_ref_encrypt(evp, key_len, keys, sa, xf, slots, his, frames), 9)[1]
        want_c = _layout(_ref_encrypt(evp, key_len, keys, sa, base, slots, his, frames), 9)[1]
        assert _run(hip, kt, False, xf, slots, his, off, buf, True)[0] == want_x
        assert _run(hip, kt, False, base, slots, None, off, buf, True)[0] == want_c
        kt.set_salt(0, bytes(8 * n_slots))                                  # the classic salts change: XPN output does not
        assert _run(hip, kt, False, xf, slots, his, off, buf, True)[0] == want_x
        kt.set_salt(0, b"".join(sa.salt))
        kt.set_xpn(0, bytes(12 * n_slots), bytes(4 * n_slots))              # the XPN state changes: classic output does not
        assert _run(hip, kt, False, base, slots, None, off, buf, True)[0] == want_c
        assert kt.status() == (hip.OK, 0)
    finally:
        kt.close()


def test_xpn_state_is_zero_when_fresh_and_after_clear_and_survives_set(hip, evp):
    rng = random.Random(34)
    key_len, n_slots, n = 24, 4, 60
    xf = _fmt_of(hip, "xpn_nosci")
    keys = splitmix_bytes(0x1B00, key_len * n_slots)
    sa = Sa(n_slots, 0x1B01)
    zero = Sa(n_slots, 0)
    zero.xsalt, zero.ssci = [bytes(12)] * n_slots, [bytes(4)] * n_slots
    slots = [p % n_slots for p in range(n)]
    his = _make_his(rng, n)
    frames = _make_frames(rng, xf, n, 0x1B10, max_payload=120)
    off, buf = _layout(frames, 0)
    with hip.KeyTable(key_len, n_slots) as kt:
        kt.set(0, keys)
        kt.set_salt(0, b"".join(sa.salt))                                   # (the classic salt is not the XPN state)
        assert _run(hip, kt, False, xf, slots, his, off, buf, True)[0] == _layout(_ref_encrypt(evp, key_len, keys, zero, xf, slots, his, frames), 0)[1]
        kt.set_xpn(0, sa.xsalt, sa.ssci)                                    # lists of entries
        assert _run(hip, kt, False, xf, slots, his, off, buf, True)[0] == _layout(_ref_encrypt(evp, key_len, keys, sa, xf, slots, his, frames), 0)[1]
        new_keys = splitmix_bytes(0x1B20, key_len * n_slots)
        kt.set(0, new_keys)                                                 # new keys, by set and by set_dev: the XPN state stays
        d_slots, d_keys = _up(hip, _u32([2])), _up(hip, keys[:key_len])
        kt.set_dev(1, d_slots.ptr, d_keys.ptr)
        mixed = new_keys[:2 * key_len] + keys[:key_len] + new_keys[3 * key_len:]
        assert _run(hip, kt, False, xf, slots, his, off, buf, True)[0] == _layout(_ref_encrypt(evp, key_len, mixed, sa, xf, slots, his, frames), 0)[1]
        kt.clear(1, 2)
        kt.set(1, mixed[key_len:3 * key_len])                               # slots 1 and 2 again: their XPN state is zero now
        part = Sa(n_slots, 0x1B01)
        part.xsalt[1] = part.xsalt[2] = bytes(12)
        part.ssci[1] = part.ssci[2] = bytes(4)
        assert _run(hip, kt, False, xf, slots, his, off, buf, True)[0] == _layout(_ref_encrypt(evp, key_len, mixed, part, xf, slots, his, frames), 0)[1]
        kt.set_xpn(2, sa.xsalt[2], sa.ssci[2])                              # one slot, as bytes
        part.xsalt[2], part.ssci[2] = sa.xsalt[2], sa.ssci[2]
        assert _run(hip, kt, False, xf, slots, his, off, buf, True)[0] == _layout(_ref_encrypt(evp, key_len, mixed, part, xf, slots, his, frames), 0)[1]
        assert kt.status() == (hip.OK, 0)


def test_set_xpn_and_crypt_are_stream_ordered(hip, evp):
    key_len, n_slots, n = 32, 8, 500
    xf = _fmt_of(hip, "xpn")
    kt, keys, sa = _table(hip, key_len, n_slots, 0x1A00)
    try:
        rng = random.Random(35)
        frames = _make_frames(rng, xf, n, 0x1A10, max_payload=600)
        slots = [rng.randrange(n_slots) for _ in range(n)]
        his = _make_his(rng, n)
        off, buf = _layout(frames, 2)
        sb = Sa(n_slots, 0x1A01)
        sb.xsalt = [bytes(x ^ 0x5A for x in s) for s in sa.xsalt]
        sb.ssci = [bytes(x ^ 0xA5 for x in s) for s in sa.ssci]
        d1 = _run(hip, kt, False, xf, slots, his, off, buf, False, sync=False)
        kt.set_xpn(0, sb.xsalt, sb.ssci)                                    # the null stream throughout, nothing waited for
        d2 = _run(hip, kt, False, xf, slots, his, off, buf, False, sync=False)
        kt.set_xpn(3, [sa.xsalt[3]], [sa.ssci[3]])
        d3 = _run(hip, kt, False, xf, slots, his, off, buf, False, sync=False)
        r1, r2, r3 = _collect(hip, d1)[0], _collect(hip, d2)[0], _collect(hip, d3)[0]
        sc = Sa(n_slots, 0x1A01)
        sc.xsalt, sc.ssci = list(sb.xsalt), list(sb.ssci)
        sc.xsalt[3], sc.ssci[3] = sa.xsalt[3], sa.ssci[3]
        for got, s in ((r1, sa), (r2, sb), (r3, sc)):
            want = _ref_encrypt(evp, key_len, keys, s, xf, slots, his, frames)
            assert got == bytes([CANARY]) * 2 + b"".join(want) + bytes([CANARY]) * 37
        assert kt.status() == (hip.OK, 0)
    finally:
        kt.close()


# ---------------------------------------------------------------- 4. refusals
@pytest.mark.parametrize("fmt_name", ["xpn", "esn16"])
@pytest.mark.parametrize("case", ["short", "unset", "cleared", "slot_range", "falling"])
def test_refused_frames(hip, evp, case, fmt_name):
    rng = random.Random(case + fmt_name)
    key_len, n_slots, n = 24, 16, 80
    xf = _fmt_of(hip, fmt_name)
    hdr, tl = xf.f.hdr_len, xf.f.tag_len
    kt, keys, sa = _table(hip, key_len, n_slots, 0x1900)
    try:
        slots = [rng.randrange(1, n_slots) for _ in range(n)]
        his = _make_his(rng, n)
        frames = _make_frames(rng, xf, n, 0x1910, max_payload=200)
        refused = set()
        if case == "short":
            frames[7] = frames[7][:hdr + tl - 1]                             # one byte less than the shortest frame
            frames[31] = b""
            frames[32] = frames[32][:1]
            refused = {7, 31, 32}
        elif case == "unset":
            kt.close()
            kt = hip.KeyTable(key_len, n_slots)
            kt.set(1, keys[key_len:])                                        # slot 0 never set
            kt.set_salt(0, b"".join(sa.salt))                                # salts and XPN state alone do not make a slot usable
            kt.set_xpn(0, sa.xsalt, sa.ssci)
            slots[12] = slots[40] = 0
            refused = {12, 40}
        elif case == "cleared":
            kt.clear(5, 2)
            slots = [s if s not in (5, 6) else 7 for s in slots]
            slots[3], slots[4], slots[79] = 5, 6, 6
            refused = {3, 4, 79}
        elif case == "slot_range":
            slots[9], slots[10], slots[60] = n_slots, 0xFFFFFFFF, n_slots + 77
            refused = {9, 10, 60}
        off, buf = _layout(frames, 11)
        if case == "falling":
            # the last two entries: [A, A - 3) falls, [A - 3, A + 7) is too short -- both refused; the bytes they name belong to frame n - 3 and to nobody
            off[n - 1] = off[n - 2] - 3
            off[n] = off[n - 1] + 10
            refused = {n - 2, n - 1}
        ok = [p for p in range(n) if p not in refused]
        ref = dict(zip(ok, _ref_encrypt(evp, key_len, keys, sa, xf, [slots[p] for p in ok], [his[p] for p in ok], [frames[p] for p in ok])))
        for inplace, fill in ((True, None), (False, 0x3C)):
            want = bytearray(buf if inplace else bytes([fill]) * len(buf))
            for p in ok:
                want[off[p]:off[p + 1]] = ref[p]
            out, _, _ = _run(hip, kt, False, xf, slots, his, off, buf, inplace, out_fill=fill or 0)
            assert out == bytes(want), (case, inplace)
            assert kt.status() == (hip.EARG, min(refused)), case
            assert kt.status() == (hip.OK, 0)
            enc = bytearray(buf)
            for p in ok:
                enc[off[p]:off[p + 1]] = ref[p]
            back, auth, _ = _run(hip, kt, True, xf, slots, his, off, bytes(enc), inplace, out_fill=fill or 0)
            assert auth == [0 if p in refused else 1 for p in range(n)], case
            wantp = bytearray(enc if inplace else bytes([fill]) * len(buf))
            for p in ok:
                wantp[off[p]:off[p + 1]] = frames[p][:-tl] + ref[p][-tl:]
            assert back == bytes(wantp), (case, inplace)
            assert kt.status() == (hip.EARG, min(refused)), case
    finally:
        kt.close()


def test_call_level_refusals_with_a_table(hip):
    with hip.KeyTable(16, 2) as kt:
        kt.set(0, bytes(32))
        d = _up(hip, bytes(256))
        for xf in (_fmt_of(hip, "xpn"), _fmt_of(hip, "esn16")):
            with pytest.raises(hip.AesGcmError) as e:
                kt.frames_crypt_x_dev(False, xf, 1, d.ptr, None, d.ptr, d.ptr, d.ptr)              # ext != 0 without d_hi
            assert e.value.code == hip.EARG
        with pytest.raises(hip.AesGcmError) as e:
            kt.frames_crypt_x_dev(False, hip.WireFormatX(hip.WireFormat.macsec(), 3, 0), 1, d.ptr, d.ptr, d.ptr, d.ptr, d.ptr)
        assert e.value.code == hip.EARG
        with pytest.raises(hip.AesGcmError) as e:
            kt.set_xpn(1, bytes(24), bytes(8))                                                       # past the last slot
        assert e.value.code == hip.EARG
        hip.dev_sync()
        assert kt.status() == (hip.OK, 0)


# ---------------------------------------------------------------- 5. EQUIVALENCE (library against library)
def test_ext_0_is_the_base_call_bit_for_bit(hip):
    """the library against itself: what the bytes must BE is test_gpu_wire.py's business for the base call"""
    rng = random.Random(55)
    key_len, n_slots, n = 32, 64, 3000
    kt, keys, sa = _table(hip, key_len, n_slots, 0x1800)
    try:
        for base in (hip.WireFormat.macsec(), hip.WireFormat.esp(12), hip.WireFormat.macsec(sci=False, auth_only=True)):
            xf = hip.WireFormatX(base, 0, 0)
            slots = [rng.randrange(n_slots) for _ in range(n)]
            frames = _make_frames(rng, xf, n, 0x1810)
            off, buf = _layout(frames, 5)
            for decrypt in (False, True):
                got, gauth, _ = _run(hip, kt, decrypt, xf, slots, None, off, buf, False, out_fill=0x3C)       # d_hi NULL: ignored
                got2, _, _ = _run(hip, kt, decrypt, xf, slots, [7] * n, off, buf, False, out_fill=0x3C)      # ... and ignored when given
                d = {"slots": _up(hip, _u32(slots)), "in": _up(hip, buf), "off": _up(hip, _u64(off)), "out": _up(hip, b"\x3C" * len(buf)),
                     "auth": _up(hip, b"\x07" * 4 * n) if decrypt else None, "nbytes": len(buf), "n": n}
                kt.frames_crypt_dev(decrypt, base, n, d["slots"].ptr, d["in"].ptr, d["off"].ptr, d["out"].ptr, d_auth=d["auth"].ptr if decrypt else None)
                want, wauth, _ = _collect(hip, d)
                assert got == want and got2 == want and gauth == wauth
                buf = want if not decrypt else buf
        assert kt.status() == (hip.OK, 0)
    finally:
        kt.close()


def test_xpn_with_a_zero_salt_is_the_classic_macsec_nonce(hip):
    """the library against itself: XPN with a zero XPN salt, ssci = salt8[0:4] and hi = be32(salt8[4:8]) builds the nonce salt8 | PN, which is the classic MACsec call's
    under salt8"""
    rng = random.Random(56)
    key_len, n_slots, n = 24, 16, 2000
    kt, keys, sa = _table(hip, key_len, n_slots, 0x1700)
    try:
        kt.set_xpn(0, bytes(12 * n_slots), b"".join(s[:4] for s in sa.salt))
        for sci, auth_only in ((True, False), (False, True)):
            xf = hip.WireFormatX.macsec_xpn(sci=sci, auth_only=auth_only)
            base = hip.WireFormatX(hip.WireFormat.macsec(sci=sci, auth_only=auth_only), 0, 0)
            slots = [rng.randrange(n_slots) for _ in range(n)]
            his = [struct.unpack(">I", sa.salt[s][4:8])[0] for s in slots]
            frames = _make_frames(rng, xf, n, 0x1710)
            off, buf = _layout(frames, 5)
            a, _, _ = _run(hip, kt, False, xf, slots, his, off, buf, True)
            b, _, _ = _run(hip, kt, False, base, slots, None, off, buf, True)
            assert a == b
            pa, autha, _ = _run(hip, kt, True, xf, slots, his, off, b, True)
            assert autha == [1] * n and pa[off[0]:off[1] - 16] == frames[0][:-16]
        assert kt.status() == (hip.OK, 0)
    finally:
        kt.close()


def test_crypt_frames_takes_a_format_with_hi(hip, evp):
    """the host convenience: a WireFormatX together with hi"""
    key_len, n_slots = 16, 3
    kt, keys, sa = _table(hip, key_len, n_slots, 0x1600)
    try:
        rng = random.Random(57)
        for name in ("xpn", "esn8"):
            xf = _fmt_of(hip, name)
            frames = _make_frames(rng, xf, 12, 0x1610, max_payload=90)
            slots = [p % n_slots for p in range(12)]
            his = _make_his(rng, 12)
            out, auth = kt.crypt_frames(xf, slots, frames, hi=his)
            assert auth is None and out == _ref_encrypt(evp, key_len, keys, sa, xf, slots, his, frames)
            back, auth = kt.crypt_frames(xf, slots, out, decrypt=True, hi=his)
            assert auth == [1] * 12 and [b[:-xf.f.tag_len] for b in back] == [f[:-xf.f.tag_len] for f in frames]
            with pytest.raises(hip.AesGcmError):
                kt.crypt_frames(xf, slots, frames)                          # a format with an extension and no hi
        with pytest.raises(hip.AesGcmError):
            kt.crypt_frames(hip.WireFormat.macsec(), [0], [bytes(60)], hi=[1])
    finally:
        kt.close()
