"""GPU: key tables on frames in wire format (aesgcm_keytab_frames_crypt_dev) -- one byte-packed buffer of frames header | payload | ICV, the nonce from the
slot's salt and header bytes.  The published MACsec vectors as wire frames in every kernel shape; random populations of MACsec and ESP frames against libcrypto
(oracle/evp_batch.c), every frame and every byte around the frames compared; bit-identity with aesgcm_keytab_crypt_dev on the split form of the same frames (the one
comparison against the library itself, labelled); containment, tampering and aesgcm_wipe_failed_dev, refusals, the salt's life cycle and stream ordering."""
import random

import pytest

from kt_common import CANARY, _collect, _layout, _u32, _u64, _up, evp  # noqa: F401
from kt_common import wire_fields as _fields, wire_ref_encrypt as _ref_encrypt, wire_split as _split
from util import golden, splitmix_bytes

pytestmark = pytest.mark.gpu


def _make_frames(rng, fmt, n, seed, max_payload=1514, aligned=False):
    """n plaintext frames: random header, random payload of 0 .. max_payload bytes (aligned: the frame a multiple of 16 bytes), the ICV's bytes as placeholders"""
    aad_len, hdr_len, iv_off, salt_len, tag_len, auth_only = _fields(fmt)
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


def _run(hip, kt, decrypt, fmt, slots, off, buf, inplace, out_fill=CANARY, sync=True):
    n = len(slots)
    d = {"slots": _up(hip, _u32(slots)), "in": _up(hip, buf), "off": _up(hip, _u64(off))}
    d["out"] = d["in"] if inplace else _up(hip, bytes([out_fill]) * len(buf))
    d["auth"] = _up(hip, b"\x07" * 4 * n) if decrypt else None
    kt.frames_crypt_dev(decrypt, fmt, n, d["slots"].ptr, d["in"].ptr, d["off"].ptr, d["out"].ptr, d_auth=d["auth"].ptr if decrypt else None)
    d["nbytes"], d["n"] = len(buf), n
    return _collect(hip, d) if sync else d


def _table(hip, key_len, n_slots, seed):
    keys = splitmix_bytes(seed, key_len * n_slots)
    sb = splitmix_bytes(seed + 1, 8 * n_slots)
    salts = [sb[8 * s:8 * s + 8] for s in range(n_slots)]
    kt = hip.KeyTable(key_len, n_slots)
    kt.set(0, keys)
    kt.set_salt(0, sb)
    return kt, keys, salts


# ---------------------------------------------------------------- 1. the published MACsec vectors as wire frames, every shape
@pytest.fixture(params=["default", "lanes8", "lanes16", "lanes64"])
def shape(request, hip):
    lanes = {"lanes8": 8, "lanes16": 16, "lanes64": 64}.get(request.param)
    if lanes is None:
        yield None
        return
    with hip.debug_library() as dbg:
        dbg.force(batch_lanes=lanes)
        yield lanes


def test_macsec_kats_as_frames(hip, shape):
    vecs = {v["name"]: v for v in golden("kat.json")["vectors"]}
    v = vecs["readme_251_aes128"]
    aad, pt, ct, tag = (bytes.fromhex(v[k]) for k in ("aad", "pt", "ct", "tag"))
    assert len(aad) == 28 and v["iv"] == "12153524c0895e81" + aad[16:20].hex()
    with hip.KeyTable(16, 4) as kt:
        kt.set(2, bytes.fromhex(v["key"]))
        kt.set_salt(2, bytes.fromhex("12153524c0895e81"))
        fmt = hip.WireFormat.macsec()
        out, auth = kt.crypt_frames(fmt, [2], [aad + pt + bytes(16)])
        assert out[0] == aad + ct + tag and auth is None
        assert out[0][-16:].hex().upper().startswith("4F8D55E7")
        back, auth = kt.crypt_frames(fmt, [2], out, decrypt=True)
        assert back[0] == aad + pt + tag and auth == [1]
        assert kt.status() == (hip.OK, 0)
    v = vecs["readme_257_aes256"]
    aad, tag = bytes.fromhex(v["aad"]), bytes.fromhex(v["tag"])
    assert v["pt"] == "" and v["iv"] == "f0761e8dcd3d0001" + aad[16:20].hex()
    with hip.KeyTable(32, 2) as kt:
        kt.set(1, bytes.fromhex(v["key"]))
        kt.set_salt(1, [bytes.fromhex("f0761e8dcd3d0001")])
        fmt = hip.WireFormat.macsec(sci=False, auth_only=True)
        out, _ = kt.crypt_frames(fmt, [1], [aad + bytes(16)])
        assert out[0] == aad + tag
        back, auth = kt.crypt_frames(fmt, [1], out, decrypt=True)
        assert back[0] == aad + tag and auth == [1]
        assert kt.status() == (hip.OK, 0)


# ---------------------------------------------------------------- 2. random populations against libcrypto, every byte compared
def _fmt_of(hip, name):
    return {"macsec": lambda: hip.WireFormat.macsec(), "macsec_nosci": lambda: hip.WireFormat.macsec(sci=False),
            "macsec_auth": lambda: hip.WireFormat.macsec(sci=False, auth_only=True),
            "esp16": lambda: hip.WireFormat.esp(16), "esp12": lambda: hip.WireFormat.esp(12), "esp8": lambda: hip.WireFormat.esp(8)}[name]()


POPULATIONS = [
    # key_len, format, frames, slots, aligned, in place
    (16, "macsec", 1, 1, False, True),
    (24, "macsec", 63, 7, True, False),
    (32, "macsec", 4097, 64, False, False),
    (16, "macsec", 4097, 64, True, True),
    (16, "esp16", 4097, 64, False, True),
    (24, "esp12", 4097, 33, True, False),
    (32, "esp8", 63, 5, False, True),
    (24, "esp8", 1, 2, True, False),
    (32, "macsec_nosci", 4097, 64, False, True),
    (16, "macsec_auth", 4097, 16, False, False),
    (24, "macsec_auth", 63, 3, True, True),
    (32, "macsec", 300000, 64, False, True),          # the launch ordered by falling frame length class
    (16, "esp16", 300000, 64, False, False),
]


@pytest.mark.parametrize("key_len, fmt_name, n, n_slots, aligned, inplace", POPULATIONS)
def test_random_frames_vs_libcrypto(hip, evp, key_len, fmt_name, n, n_slots, aligned, inplace):
    rng = random.Random("%d %s %d" % (key_len, fmt_name, n))
    fmt = _fmt_of(hip, fmt_name)
    kt, keys, salts = _table(hip, key_len, n_slots, 0xF00 + key_len + n)
    try:
        slots = [rng.randrange(n_slots) for _ in range(n)]
        slots[0], slots[-1] = 0, n_slots - 1
        frames = _make_frames(rng, fmt, n, 0xF10 + n + key_len, aligned=aligned)
        off, buf = _layout(frames, 32 if aligned else 13)
        want = _ref_encrypt(evp, key_len, keys, salts, fmt, slots, frames)
        _, want_buf = _layout(want, off[0])
        out, _, _ = _run(hip, kt, False, fmt, slots, off, buf, inplace)
        if out != want_buf:                                                  # name the first frame that differs
            for p in range(n):
                assert out[off[p]:off[p + 1]] == want[p], (p, len(frames[p]))
        assert out == want_buf
        # ... and back: libcrypto's frames decrypt to the plaintext with every ICV accepted (the ICV's bytes stay)
        back, auth, _ = _run(hip, kt, True, fmt, slots, off, want_buf, inplace)
        body = fmt.tag_len
        _, plain_buf = _layout([f[:-body] + w[-body:] for f, w in zip(frames, want)], off[0])
        assert back == plain_buf
        assert auth == [1] * n
        assert kt.status() == (hip.OK, 0)
    finally:
        kt.close()


# ---------------------------------------------------------------- 3. EQUIVALENCE (library against library): the split form through aesgcm_keytab_crypt_dev
@pytest.mark.parametrize("key_len, fmt_name", [(32, "macsec"), (16, "esp12"), (24, "macsec_auth")])
def test_bit_identical_to_the_split_form(hip, key_len, fmt_name):
    """the same frames as five parallel arrays through aesgcm_keytab_crypt_dev: ciphertext and (truncated) tag bit for bit.  This compares the library with
    itself; what the bytes must BE is test_random_frames_vs_libcrypto's business."""
    rng = random.Random(key_len)
    fmt = _fmt_of(hip, fmt_name)
    n, n_slots = 3000, 64
    kt, keys, salts = _table(hip, key_len, n_slots, 0xE00 + key_len)
    try:
        slots = [rng.randrange(n_slots) for _ in range(n)]
        frames = _make_frames(rng, fmt, n, 0xE10 + key_len)
        off, buf = _layout(frames, 5)
        out, _, _ = _run(hip, kt, False, fmt, slots, off, buf, True)
        parts = [_split(fmt, salts[s], f) for s, f in zip(slots, frames)]
        cts, tags = kt.crypt(slots, [x[0] for x in parts], [x[1] for x in parts], [x[2] for x in parts])
        for p in range(n):
            f = frames[p]
            front = len(f) - fmt.tag_len - len(cts[p])
            assert out[off[p]:off[p + 1]] == f[:front] + cts[p] + tags[p][:fmt.tag_len], p
    finally:
        kt.close()


# ---------------------------------------------------------------- 4. containment
def test_nothing_outside_the_frames_is_written(hip, evp):
    """canaries in front of the first frame, behind the last and BETWEEN frames (the gaps are entries too short to be frames: refused, untouched); out of place every
    byte of an accepted frame is defined -- header copied, on decrypt the ICV as well"""
    rng = random.Random(4)
    key_len, n_slots = 32, 9
    for fmt_name in ("macsec", "esp12", "macsec_auth"):
        fmt = _fmt_of(hip, fmt_name)
        kt, keys, salts = _table(hip, key_len, n_slots, 0xD00)
        try:
            real = _make_frames(rng, fmt, 200, 0xD10, max_payload=300)
            entries, is_gap = [], []
            for f in real:
                entries.append(f); is_gap.append(False)
                entries.append(bytes([CANARY]) * rng.randrange(1, fmt.hdr_len + 8)); is_gap.append(True)      # shorter than hdr_len + tag_len
            n = len(entries)
            slots = [rng.randrange(n_slots) for _ in range(n)]
            off, buf = _layout(entries, 29)
            want_real = _ref_encrypt(evp, key_len, keys, salts, fmt, [s for s, g in zip(slots, is_gap) if not g], real)
            it = iter(want_real)
            want = [e if g else next(it) for e, g in zip(entries, is_gap)]
            for inplace, fill in ((True, CANARY), (False, 0x3C)):
                gaps = [bytes([fill]) * len(e) if g else w for e, g, w in zip(entries, is_gap, want)]
                want_buf = bytes([fill]) * 29 + b"".join(gaps) + bytes([fill]) * 37
                out, _, _ = _run(hip, kt, False, fmt, slots, off, buf, inplace, out_fill=fill)
                assert out == want_buf, (fmt_name, inplace)
                assert kt.status() == (hip.EARG, 1)
                # decrypt of libcrypto's frames: plaintext, header and ICV in the output; gaps refused with auth 0
                _, enc_buf = _layout(want, 29)
                back, auth, _ = _run(hip, kt, True, fmt, slots, off, enc_buf, inplace, out_fill=fill)
                plain = [bytes([fill]) * len(e) if g else e[:-fmt.tag_len] + w[-fmt.tag_len:] for e, g, w in zip(entries, is_gap, want)]
                assert back == bytes([fill]) * 29 + b"".join(plain) + bytes([fill]) * 37, (fmt_name, inplace)
                assert auth == [0 if g else 1 for g in is_gap]
                assert kt.status() == (hip.EARG, 1)
        finally:
            kt.close()


# ---------------------------------------------------------------- 5. tampering and fail-closed
def test_tampered_frames_fail_alone_and_are_wiped(hip, evp):
    rng = random.Random(5)
    key_len, n_slots, n = 16, 12, 600
    # ESP with four more header bytes behind the IV field: bytes 16 .. 19 are neither authenticated nor nonce
    fmt = hip.WireFormat(8, 20, 8, 4, 12, 0)
    assert fmt.check() == hip.OK
    kt, keys, salts = _table(hip, key_len, n_slots, 0xC00)
    try:
        slots = [1 + rng.randrange(n_slots - 1) for _ in range(n)]
        slots[50] = slots[51] = 0                                            # slot 0: its salt changes below
        frames = _make_frames(rng, fmt, n, 0xC10, max_payload=400)
        frames = [f if len(f) > 32 else f[:20] + b"\x11" + f[20:] for f in frames]     # a payload byte to flip
        off, _ = _layout(frames, 3)
        enc = [bytearray(f) for f in _ref_encrypt(evp, key_len, keys, salts, fmt, slots, frames)]
        flips = {10: 3, 20: 9, 30: 12, 40: 17, 60: 20, 70: -1, 80: -12}     # SPI, IV field (nonce), IV field, pass-through header, payload, ICV's last and first byte
        for p, at in flips.items():
            enc[p][at] ^= 0x10
        must_fail = {10, 20, 30, 60, 70, 80}                                 # NOT 40: bytes 16 .. 19 are not covered by anything
        _, enc_buf = _layout([bytes(e) for e in enc], 3)
        back, auth, d = _run(hip, kt, True, fmt, slots, off, enc_buf, False, out_fill=0x3C)
        assert auth == [0 if p in must_fail else 1 for p in range(n)]
        for p in range(n):
            if p not in must_fail:
                assert back[off[p] + 20:off[p + 1] - 12] == frames[p][20:-12], p
        assert back[off[40]:off[40] + 20] == bytes(enc[40][:20])             # the flipped pass-through byte passes through
        hip.wipe_failed_dev(n, d["out"].ptr, d["auth"].ptr, d_data_off=d["off"].ptr)
        hip.dev_sync()
        wiped = bytes(d["out"].download(len(enc_buf)))
        for p in range(n):
            seg = wiped[off[p]:off[p + 1]]
            assert seg == (bytes(len(seg)) if p in must_fail else back[off[p]:off[p + 1]]), p
        assert wiped[:3] == back[:3] and wiped[off[n]:] == back[off[n]:]
        # another salt in slot 0: exactly its frames fail
        kt.set_salt(0, bytes(a ^ 0x80 if i == 2 else a for i, a in enumerate(salts[0])))
        _, clean_buf = _layout(_ref_encrypt(evp, key_len, keys, salts, fmt, slots, frames), 3)
        _, auth, _ = _run(hip, kt, True, fmt, slots, off, clean_buf, True)
        assert auth == [0 if s == 0 else 1 for s in slots]
        assert kt.status() == (hip.OK, 0)
    finally:
        kt.close()


# ---------------------------------------------------------------- 6. refusals and the salt's life cycle
@pytest.mark.parametrize("case", ["short", "unset", "cleared", "slot_range", "falling"])
def test_refused_frames(hip, evp, case):
    rng = random.Random(case)
    key_len, n_slots, n = 24, 16, 80
    fmt = hip.WireFormat.macsec()
    kt, keys, salts = _table(hip, key_len, n_slots, 0xB00)
    try:
        slots = [rng.randrange(1, n_slots) for _ in range(n)]
        frames = _make_frames(rng, fmt, n, 0xB10, max_payload=200)
        refused = set()
        if case == "short":
            frames[7] = frames[7][:43]                                       # 28 + 16 = 44 is the shortest frame
            frames[31] = b""
            frames[32] = frames[32][:1]
            refused = {7, 31, 32}
        elif case == "unset":
            kt.close()
            kt = hip.KeyTable(key_len, n_slots)
            kt.set(1, keys[key_len:])                                        # slot 0 never set
            kt.set_salt(0, b"".join(salts))                                  # a salt alone does not make a slot usable
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
        ref = dict(zip(ok, _ref_encrypt(evp, key_len, keys, salts, fmt, [slots[p] for p in ok], [frames[p] for p in ok])))
        for inplace, fill in ((True, None), (False, 0x3C)):
            want = bytearray(buf if inplace else bytes([fill]) * len(buf))
            for p in ok:
                want[off[p]:off[p + 1]] = ref[p]
            out, _, _ = _run(hip, kt, False, fmt, slots, off, buf, inplace, out_fill=fill or 0)
            assert out == bytes(want), (case, inplace)
            assert kt.status() == (hip.EARG, min(refused)), case
            assert kt.status() == (hip.OK, 0)
            enc = bytearray(buf)
            for p in ok:
                enc[off[p]:off[p + 1]] = ref[p]
            back, auth, _ = _run(hip, kt, True, fmt, slots, off, bytes(enc), inplace, out_fill=fill or 0)
            assert auth == [0 if p in refused else 1 for p in range(n)], case
            wantp = bytearray(enc if inplace else bytes([fill]) * len(buf))
            for p in ok:
                wantp[off[p]:off[p + 1]] = frames[p][:-16] + ref[p][-16:]
            assert back == bytes(wantp), (case, inplace)
            assert kt.status() == (hip.EARG, min(refused)), case
    finally:
        kt.close()


def test_salt_survives_set_and_is_zero_after_clear(hip, evp):
    key_len, n_slots = 16, 4
    fmt = hip.WireFormat.macsec()
    kt, keys, salts = _table(hip, key_len, n_slots, 0xA00)
    try:
        rng = random.Random(6)
        frames = _make_frames(rng, fmt, 40, 0xA10, max_payload=100)
        slots = [p % n_slots for p in range(40)]
        off, buf = _layout(frames, 0)
        new_keys = splitmix_bytes(0xA20, key_len * n_slots)
        kt.set(0, new_keys)                                                  # new keys, the salts stay
        out, _, _ = _run(hip, kt, False, fmt, slots, off, buf, True)
        assert out == _layout(_ref_encrypt(evp, key_len, new_keys, salts, fmt, slots, frames), 0)[1]
        d_slots, d_keys = _up(hip, _u32([2])), _up(hip, keys[:key_len])
        kt.set_dev(1, d_slots.ptr, d_keys.ptr)                              # ... and through set_dev
        mixed = new_keys[:2 * key_len] + keys[:key_len] + new_keys[3 * key_len:]
        out, _, _ = _run(hip, kt, False, fmt, slots, off, buf, True)
        assert out == _layout(_ref_encrypt(evp, key_len, mixed, salts, fmt, slots, frames), 0)[1]
        kt.clear(1, 2)
        kt.set(1, mixed[key_len:3 * key_len])                                # slots 1 and 2 again: their salts are zero now
        zsalts = [salts[0], bytes(8), bytes(8), salts[3]]
        out, _, _ = _run(hip, kt, False, fmt, slots, off, buf, True)
        assert out == _layout(_ref_encrypt(evp, key_len, mixed, zsalts, fmt, slots, frames), 0)[1]
        assert kt.status() == (hip.OK, 0)
        # a fresh table's salts are zero; four-byte salts use the first four bytes of the slot's eight
        with hip.KeyTable(key_len, n_slots) as fresh:
            fresh.set(0, keys)
            out, _, _ = _run(hip, fresh, False, fmt, slots, off, buf, True)
            assert out == _layout(_ref_encrypt(evp, key_len, keys, [bytes(8)] * n_slots, fmt, slots, frames), 0)[1]
            esp = hip.WireFormat.esp(8)
            fresh.set_salt(1, [b"\x01\x02\x03\x04", b"\xf1\xf2\xf3\xf4\xf5"])
            eframes = _make_frames(rng, esp, 40, 0xA30, max_payload=100)
            eoff, ebuf = _layout(eframes, 1)
            out, _, _ = _run(hip, fresh, False, esp, slots, eoff, ebuf, True)
            s4 = [bytes(8), b"\x01\x02\x03\x04" + bytes(4), b"\xf1\xf2\xf3\xf4\xf5" + bytes(3), bytes(8)]
            assert out == _layout(_ref_encrypt(evp, key_len, keys, s4, esp, slots, eframes), 1)[1]
    finally:
        kt.close()


# ---------------------------------------------------------------- 7. salt and crypt calls on one stream, no host synchronisation
def test_salt_and_crypt_are_stream_ordered(hip, evp):
    key_len, n_slots, n = 32, 8, 500
    fmt = hip.WireFormat.esp(16)
    kt, keys, salts = _table(hip, key_len, n_slots, 0x900)
    try:
        rng = random.Random(7)
        frames = _make_frames(rng, fmt, n, 0x910, max_payload=600)
        slots = [rng.randrange(n_slots) for _ in range(n)]
        off, buf = _layout(frames, 2)
        salts_b = [bytes(x ^ 0x5A for x in s) for s in salts]
        d1 = _run(hip, kt, False, fmt, slots, off, buf, False, sync=False)
        kt.set_salt(0, b"".join(salts_b))                                    # the null stream throughout, nothing waited for
        d2 = _run(hip, kt, False, fmt, slots, off, buf, False, sync=False)
        kt.set_salt(3, [salts[3]])
        d3 = _run(hip, kt, False, fmt, slots, off, buf, False, sync=False)
        r1, r2, r3 = _collect(hip, d1)[0], _collect(hip, d2)[0], _collect(hip, d3)[0]
        salts_c = salts_b[:3] + [salts[3]] + salts_b[4:]
        for got, sl in ((r1, salts), (r2, salts_b), (r3, salts_c)):
            want = _ref_encrypt(evp, key_len, keys, sl, fmt, slots, frames)
            assert got == bytes([CANARY]) * 2 + b"".join(want) + bytes([CANARY]) * 37
        assert kt.status() == (hip.OK, 0)
    finally:
        kt.close()
