"""GPU: key tables (aesgcm_keytab_*) -- slots of key material built on the device once, a slot named per packet: KATs through slots, every key size against
the oracle, bit-identity with the batch entry points given the gathered keys (every shape, the sorted path), key rotation on one stream, refused packets,
keys set from device memory."""
import random
import struct

import pytest

from kt_common import _u32, _u64, _up
from util import golden, splitmix_bytes

pytestmark = pytest.mark.gpu


def _var_call(hip, kt, decrypt, slots, ivs, aad_blob, aoff, blob, doff, out_fill=None, expect=None, inplace=False, sync=True):
    """one offset-array call; -> (out bytes, tags, auth or None), buffers kept alive until synchronised"""
    n = len(slots)
    d = {"slots": _up(hip, _u32(slots)), "ivs": _up(hip, ivs), "aad": _up(hip, aad_blob), "aoff": _up(hip, _u64(aoff)),
         "in": _up(hip, blob), "doff": _up(hip, _u64(doff)), "tags": _up(hip, b"\xee" * 16 * n)}
    d["out"] = d["in"] if inplace else _up(hip, bytes([out_fill or 0]) * len(blob))
    if expect is not None:
        d["exp"] = _up(hip, expect)
    d["auth"] = _up(hip, b"\x07" * 4 * n) if decrypt else None
    kt.crypt_dev(decrypt, n, d["slots"].ptr, d["ivs"].ptr, d["in"].ptr, d["doff"].ptr, d["out"].ptr, d["tags"].ptr, d_aad=d["aad"].ptr,
                 d_aad_off=d["aoff"].ptr, d_expect_tags=d["exp"].ptr if expect is not None else None, d_auth=d["auth"].ptr if decrypt else None)
    if not sync:
        return d
    return _collect(hip, d, len(blob), n)


def _collect(hip, d, nbytes, n):
    hip.dev_sync()
    out = bytes(d["out"].download(nbytes)) if nbytes else b""
    tags = bytes(d["tags"].download(16 * n))
    auth = list(struct.unpack("<%di" % n, bytes(d["auth"].download(4 * n)))) if d.get("auth") is not None else None
    return out, tags, auth


def _offsets(lens, start=0):
    off = [start]
    for x in lens:
        off.append(off[-1] + x)
    return off


# ---------------------------------------------------------------- 1. KATs through slots
def test_kats_through_slots(hip):
    vecs = golden("kat.json")["vectors"]
    assert len(vecs) == 12
    by_len = {}
    for i, v in enumerate(vecs):
        by_len.setdefault(len(v["key"]) // 2, []).append(i)
    tables = {kl: hip.KeyTable(kl, len(ix) + 3) for kl, ix in by_len.items()}
    try:
        for kl, ix in by_len.items():
            for s, i in enumerate(ix):
                tables[kl].set(s + 2, bytes.fromhex(vecs[i]["key"]))          # slot s + 2: not slot 0, not in order of the call
            ivs = [bytes.fromhex(vecs[i]["iv"]) for i in ix]
            aads = [bytes.fromhex(vecs[i]["aad"]) for i in ix]
            pts = [bytes.fromhex(vecs[i]["pt"]) for i in ix]
            cts, tags = tables[kl].crypt([s + 2 for s in range(len(ix))], ivs, aads, pts)
            for s, i in enumerate(ix):
                assert cts[s].hex() == vecs[i]["ct"], vecs[i]["name"]
                assert tags[s].hex() == vecs[i]["tag"], vecs[i]["name"]
                if vecs[i]["name"] == "readme_251_aes128":
                    assert tags[s].hex().upper().startswith("4F8D55E7") and tags[s].hex().upper().endswith("B880")
            back, tags2, auth = tables[kl].crypt([s + 2 for s in range(len(ix))], ivs, aads, cts, decrypt=True, tags=tags)
            assert back == pts and tags2 == tags and auth == [1] * len(ix)
            assert tables[kl].status() == (hip.OK, 0)
    finally:
        for t in tables.values():
            t.close()


# ---------------------------------------------------------------- 2. every key size against the oracle; decrypt in place; wipe
@pytest.mark.parametrize("key_len", [16, 24, 32])
def test_random_slots_vs_oracle(hip, orc, key_len):
    rng = random.Random(key_len)
    n_slots, n = 1000, 3000
    keys = splitmix_bytes(0x4B00 + key_len, key_len * n_slots)
    dlens = [0, 1, 15, 16, 17, 64, 100, 255, 256, 1000, 1514, 1600]
    slots = [rng.randrange(n_slots) for _ in range(n)]
    slots[0], slots[1], slots[2], slots[3] = 0, n_slots - 1, 0, n_slots - 1
    lens = [rng.choice(dlens) for _ in range(n)]
    alens = [rng.randrange(41) for _ in range(n)]
    ivs = splitmix_bytes(0x1700 + key_len, 12 * n)
    blob = splitmix_bytes(0xDA7A + key_len, sum(lens))
    aad_blob = splitmix_bytes(0xAAD + key_len, sum(alens))
    doff, aoff = _offsets(lens), _offsets(alens)
    with hip.KeyTable(key_len, n_slots) as kt:
        kt.set(0, keys[:key_len * 600])
        kt.set(600, keys[key_len * 600:])                                  # two calls through the staging buffer
        ct, tags, _ = _var_call(hip, kt, False, slots, ivs, aad_blob, aoff, blob, doff)
        fast = {}
        want_ct, want_tags = [], []
        for p in range(n):
            s = slots[p]
            if s not in fast:
                fast[s] = orc.Fast(keys[key_len * s:key_len * (s + 1)])
            c, t = fast[s].encrypt(ivs[12 * p:12 * p + 12], aad_blob[aoff[p]:aoff[p + 1]], blob[doff[p]:doff[p + 1]])
            want_ct.append(c); want_tags.append(t)
        assert ct == b"".join(want_ct)
        assert tags == b"".join(want_tags)
        # decrypt in place, one tag in 100 tampered
        bad = set(range(7, n, 100))
        exp = bytearray(tags)
        for p in bad:
            exp[16 * p] ^= 0x01
        d = _var_call(hip, kt, True, slots, ivs, aad_blob, aoff, ct, doff, expect=bytes(exp), inplace=True, sync=False)
        back, tags2, auth = _collect(hip, d, len(blob), n)
        assert back == blob and tags2 == tags
        assert auth == [0 if p in bad else 1 for p in range(n)]
        # aesgcm_wipe_failed_dev zeroes exactly the failed packets
        hip.wipe_failed_dev(n, d["out"].ptr, d["auth"].ptr, d_data_off=d["doff"].ptr)
        hip.dev_sync()
        wiped = bytes(d["out"].download(len(blob)))
        for p in range(n):
            seg = wiped[doff[p]:doff[p + 1]]
            assert seg == (bytes(len(seg)) if p in bad else blob[doff[p]:doff[p + 1]]), p
        assert kt.status() == (hip.OK, 0)


# ---------------------------------------------------------------- 3. bit-identical with the batch entry points, every shape
@pytest.fixture(params=["default", "lanes8", "lanes16", "lanes64"])
def shape(request, hip):
    lanes = {"lanes8": 8, "lanes16": 16, "lanes64": 64}.get(request.param)
    if lanes is None:
        yield None
        return
    with hip.debug_library() as dbg:
        dbg.force(batch_lanes=lanes)
        yield lanes


def _fixed_pair(hip, kt, keys, key_len, slots, pkt_len, aad_len, misalign=0):
    n = len(slots)
    ivs = splitmix_bytes(0x51 + pkt_len, 12 * n)
    data = splitmix_bytes(0x52 + pkt_len, pkt_len * n)
    aad = splitmix_bytes(0x53 + pkt_len, aad_len * n)
    gathered = b"".join(keys[key_len * s:key_len * (s + 1)] for s in slots)
    d_in = _up(hip, b"\x00" * misalign + data)
    d_o1, d_o2 = _up(hip, bytes(len(data) + misalign)), _up(hip, bytes(len(data) + misalign))
    d_ivs, d_aad, d_slots, d_keys = _up(hip, ivs), _up(hip, aad), _up(hip, _u32(slots)), _up(hip, gathered)
    d_t1, d_t2 = _up(hip, bytes(16 * n)), _up(hip, bytes(16 * n))
    kt.crypt_dev(False, n, d_slots.ptr, d_ivs.ptr, d_in.ptr + misalign, None, d_o1.ptr + misalign, d_t1.ptr, d_aad=d_aad.ptr if aad_len else None,
                 pkt_len=pkt_len, aad_len=aad_len)
    hip.batch_crypt_dev(False, n, key_len, d_keys.ptr, d_ivs.ptr, d_in.ptr + misalign, pkt_len, d_o2.ptr + misalign, d_t2.ptr,
                        d_aad=d_aad.ptr if aad_len else None, aad_len=aad_len)
    hip.dev_sync()
    assert bytes(d_t1.download()) == bytes(d_t2.download())
    assert bytes(d_o1.download()) == bytes(d_o2.download())
    return bytes(d_o1.download())[misalign:], bytes(d_t1.download()), ivs, data, aad


def test_fixed_records_match_batch(hip, orc, shape):
    rng = random.Random(3)
    key_len = 16
    keys = splitmix_bytes(0x777, key_len * 1024)
    with hip.KeyTable(key_len, 1024) as kt:
        kt.set(0, keys)
        slots = [rng.randrange(1024) for _ in range(4096)]
        ct, tags, ivs, data, _ = _fixed_pair(hip, kt, keys, key_len, slots, 4096, 0)           # cfg5's shape: 4096 x 4 KiB
        for p in (0, 1, 4095):
            c, t = orc.Fast(keys[16 * slots[p]:16 * slots[p] + 16]).encrypt(ivs[12 * p:12 * p + 12], b"", data[4096 * p:4096 * (p + 1)])
            assert ct[4096 * p:4096 * (p + 1)] == c and tags[16 * p:16 * p + 16] == t
    for key_len, pkt_len, aad_len, n, mis in ((24, 1000, 13, 777, 0), (32, 33, 0, 300, 0), (16, 1500, 28, 513, 3), (32, 4096, 0, 130, 5), (24, 17, 40, 64, 1)):
        keys = splitmix_bytes(0x888 + key_len, key_len * 97)
        with hip.KeyTable(key_len, 97) as kt:
            kt.set(0, keys)
            slots = [rng.randrange(97) for _ in range(n)]
            _fixed_pair(hip, kt, keys, key_len, slots, pkt_len, aad_len, misalign=mis)
            assert kt.status() == (hip.OK, 0)


def _var_pair(hip, kt, keys, key_len, slots, lens, alens, seed, misalign=0):
    n = len(slots)
    ivs = splitmix_bytes(seed, 12 * n)
    blob = splitmix_bytes(seed + 1, sum(lens))
    aad_blob = splitmix_bytes(seed + 2, sum(alens))
    doff, aoff = _offsets(lens), _offsets(alens)
    gathered = b"".join(keys[key_len * s:key_len * (s + 1)] for s in slots)
    d_in = _up(hip, b"\x00" * misalign + blob)
    d_o1, d_o2 = _up(hip, bytes(len(blob) + misalign)), _up(hip, bytes(len(blob) + misalign))
    d_ivs, d_aad, d_slots, d_keys = _up(hip, ivs), _up(hip, aad_blob), _up(hip, _u32(slots)), _up(hip, gathered)
    d_doff, d_aoff = _up(hip, _u64(doff)), _up(hip, _u64(aoff))
    d_t1, d_t2 = _up(hip, bytes(16 * n)), _up(hip, bytes(16 * n))
    kt.crypt_dev(False, n, d_slots.ptr, d_ivs.ptr, d_in.ptr + misalign, d_doff.ptr, d_o1.ptr + misalign, d_t1.ptr, d_aad=d_aad.ptr, d_aad_off=d_aoff.ptr)
    hip.batch_crypt_var_dev(False, n, key_len, d_keys.ptr, d_ivs.ptr, d_in.ptr + misalign, d_doff.ptr, d_o2.ptr + misalign, d_t2.ptr,
                            d_aad=d_aad.ptr, d_aad_off=d_aoff.ptr)
    hip.dev_sync()
    t1 = bytes(d_t1.download())
    assert t1 == bytes(d_t2.download())
    o1 = bytes(d_o1.download())
    assert o1 == bytes(d_o2.download())
    return o1[misalign:], t1, ivs, blob, aad_blob, doff, aoff


def test_frames_match_batch(hip, shape):
    rng = random.Random(11)
    for key_len, n, mis in ((16, 2000, 0), (32, 1500, 7), (24, 999, 0)):
        keys = splitmix_bytes(0x999 + key_len, key_len * 64)
        with hip.KeyTable(key_len, 64) as kt:
            kt.set(0, keys)
            slots = [rng.randrange(64) for _ in range(n)]
            lens = [rng.randrange(64, 1515) for _ in range(n)]
            alens = [28] * n
            _var_pair(hip, kt, keys, key_len, slots, lens, alens, 0x4000 + key_len, misalign=mis)
            assert kt.status() == (hip.OK, 0)


def test_sorted_path_300k_frames(hip, orc):
    """300 000 frames take the order by falling length class (from 262144 for AES-128, 98304 for the longer keys): in full against the batch path, a seeded
    sample against the oracle"""
    rng = random.Random(300)
    n = 300000
    for key_len in (16, 32):
        keys = splitmix_bytes(0xAAA + key_len, key_len * 64)
        with hip.KeyTable(key_len, 64) as kt:
            kt.set(0, keys)
            slots = [rng.randrange(64) for _ in range(n)]
            lens = [rng.randrange(64, 1515) for _ in range(n)]
            alens = [28] * n
            ct, tags, ivs, blob, aad_blob, doff, aoff = _var_pair(hip, kt, keys, key_len, slots, lens, alens, 0x5000 + key_len)
            for p in sorted(random.Random(key_len).sample(range(n), 200)) + [0, n - 1]:
                s = slots[p]
                c, t = orc.Fast(keys[key_len * s:key_len * (s + 1)]).encrypt(ivs[12 * p:12 * p + 12], aad_blob[aoff[p]:aoff[p + 1]], blob[doff[p]:doff[p + 1]])
                assert ct[doff[p]:doff[p + 1]] == c and tags[16 * p:16 * p + 16] == t, p


# ---------------------------------------------------------------- 4. rotation on one stream
def test_rotation_on_one_stream(hip, orc):
    key_a, key_b = splitmix_bytes(0xA, 32), splitmix_bytes(0xB, 32)
    others = splitmix_bytes(0xC, 32 * 16)
    slots = [7, 1, 7, 2, 3, 7, 0, 15]
    n = len(slots)
    lens = [60, 0, 1514, 16, 100, 33, 64, 1]
    alens = [28, 0, 16, 28, 3, 40, 28, 28]
    ivs = splitmix_bytes(0x1D, 12 * n)
    blob = splitmix_bytes(0x1E, sum(lens))
    aad_blob = splitmix_bytes(0x1F, sum(alens))
    doff, aoff = _offsets(lens), _offsets(alens)

    def want(p, key7):
        key = key7 if slots[p] == 7 else others[32 * slots[p]:32 * slots[p] + 32]
        return orc.Fast(key).encrypt(ivs[12 * p:12 * p + 12], aad_blob[aoff[p]:aoff[p + 1]], blob[doff[p]:doff[p + 1]])

    with hip.KeyTable(32, 16) as kt:
        kt.set(0, others)
        kt.set(7, key_a)
        d1 = _var_call(hip, kt, False, slots, ivs, aad_blob, aoff, blob, doff, sync=False)
        kt.set(7, key_b)                                                  # same (null) stream, no host synchronisation in between
        d2 = _var_call(hip, kt, False, slots, ivs, aad_blob, aoff, blob, doff, sync=False)
        kt.clear(7)
        d3 = _var_call(hip, kt, False, slots, ivs, aad_blob, aoff, blob, doff, out_fill=0x5A, sync=False)
        r1, r2, r3 = _collect(hip, d1, len(blob), n), _collect(hip, d2, len(blob), n), _collect(hip, d3, len(blob), n)
        for p in range(n):
            c, t = want(p, key_a)
            assert r1[0][doff[p]:doff[p + 1]] == c and r1[1][16 * p:16 * p + 16] == t, p
            c, t = want(p, key_b)
            assert r2[0][doff[p]:doff[p + 1]] == c and r2[1][16 * p:16 * p + 16] == t, p
            if slots[p] == 7:
                assert r3[0][doff[p]:doff[p + 1]] == b"\x5a" * lens[p] and r3[1][16 * p:16 * p + 16] == bytes(16), p
            else:
                assert r3[0][doff[p]:doff[p + 1]] == c and r3[1][16 * p:16 * p + 16] == t, p
        assert kt.status() == (hip.EARG, 0)                               # packet 0 names slot 7
        assert kt.status() == (hip.OK, 0)                                 # reading cleared it


# ---------------------------------------------------------------- 5. refusals
def _refusal_case(hip, orc, case):
    key_len, n_slots, n = 16, 32, 48
    rng = random.Random(case)
    keys = splitmix_bytes(0x5E7, key_len * n_slots)
    slots = [rng.randrange(n_slots) for _ in range(n)]
    slots = [s if s != 3 else 4 for s in slots]                          # slot 3 is never set
    lens = [rng.randrange(0, 300) for _ in range(n)]
    alens = [rng.randrange(1, 41) for _ in range(n)]
    lens[0] = 40
    refused = set()
    doff, aoff = _offsets(lens, start=128), _offsets(alens)
    if case == "slot_range":
        slots[5], slots[9], slots[30] = n_slots, 0xFFFFFFFF, n_slots + 1000
        refused = {5, 9, 30}
    elif case == "unset":
        slots[7], slots[20] = 3, 3
        refused = {7, 20}
    elif case == "falling":
        doff[0] = 128 + 72                                                # packet 0: [200, 168) falls (the bytes below 200 belong to nobody)
        aoff[11] = aoff[10] - 1                                           # packet 10's AAD falls; packet 11's AAD starts a byte early
        refused = {0, 10}
    elif case == "too_long":
        doff[n] = doff[n - 1] + (1 << 28)                                 # the last packet: 2^28 bytes of data
        aoff_last = aoff[n - 1]
        refused = {n - 1}
        aoff[n] = aoff_last + 1
    elif case == "aad_too_long":
        aoff[n] = aoff[n - 1] + (1 << 28)
        refused = {n - 1}
    ivs = splitmix_bytes(0x1111, 12 * n)
    span = max(doff[p + 1] for p in range(n) if p not in refused or case != "too_long")
    span = max(span, max(doff[:n]))
    blob = splitmix_bytes(0x2222, span)
    aad_blob = splitmix_bytes(0x3333, max(aoff[p + 1] for p in range(n) if p not in refused or case != "aad_too_long") + 64)
    want_out = bytearray(b"\x5a" * len(blob))
    want_tags = []
    for p in range(n):
        if p in refused:
            want_tags.append(bytes(16))
            continue
        c, t = orc.Fast(keys[key_len * slots[p]:key_len * (slots[p] + 1)]).encrypt(ivs[12 * p:12 * p + 12], aad_blob[aoff[p]:aoff[p + 1]], blob[doff[p]:doff[p + 1]])
        want_out[doff[p]:doff[p + 1]] = c
        want_tags.append(t)
    with hip.KeyTable(key_len, n_slots) as kt:
        kt.set(0, keys[:3 * key_len])
        kt.set(4, keys[4 * key_len:])
        out, tags, _ = _var_call(hip, kt, False, slots, ivs, aad_blob, aoff, blob, doff, out_fill=0x5A)
        assert out == bytes(want_out), case
        assert [tags[16 * p:16 * p + 16] for p in range(n)] == want_tags, case
        assert kt.status() == (hip.EARG, min(refused)), case
        # decrypt of the oracle's ciphertext (the refused packets' ranges hold 0x5A): the same packets refused, auth 0 for them only
        ct = bytes(want_out)
        out2, tags2, auth = _var_call(hip, kt, True, slots, ivs, aad_blob, aoff, ct, doff, out_fill=0x5A, expect=b"".join(want_tags))
        assert auth == [0 if p in refused else 1 for p in range(n)], case
        assert [tags2[16 * p:16 * p + 16] for p in range(n)] == want_tags, case
        for p in range(n):
            if p not in refused:
                assert out2[doff[p]:doff[p + 1]] == blob[doff[p]:doff[p + 1]], (case, p)
            elif case in ("slot_range", "unset"):
                assert out2[doff[p]:doff[p + 1]] == b"\x5a" * lens[p], (case, p)
        assert kt.status() == (hip.EARG, min(refused)), case


@pytest.mark.parametrize("case", ["slot_range", "unset", "falling", "too_long", "aad_too_long"])
def test_refused_packets(hip, orc, case):
    _refusal_case(hip, orc, case)


# ---------------------------------------------------------------- 6. keys from device memory
def test_set_dev_matches_set(hip):
    rng = random.Random(6)
    key_len, n_slots, n = 24, 200, 700
    keys = splitmix_bytes(0x6E7, key_len * n_slots)
    order = list(range(n_slots))
    rng.shuffle(order)
    dev_keys = b"".join(keys[key_len * s:key_len * (s + 1)] for s in order)
    slots = [rng.randrange(n_slots) for _ in range(n)]
    lens = [rng.randrange(0, 700) for _ in range(n)]
    alens = [rng.randrange(0, 30) for _ in range(n)]
    ivs = splitmix_bytes(0x6E8, 12 * n)
    blob = splitmix_bytes(0x6E9, sum(lens))
    aad_blob = splitmix_bytes(0x6EA, sum(alens))
    doff, aoff = _offsets(lens), _offsets(alens)
    with hip.KeyTable(key_len, n_slots) as a, hip.KeyTable(key_len, n_slots) as b:
        a.set(0, keys)
        d_slots = _up(hip, _u32(order + [n_slots + 3]))                  # one entry past the table: skipped and reported
        d_keys = _up(hip, dev_keys + bytes(key_len))
        b.set_dev(n_slots + 1, d_slots.ptr, d_keys.ptr)
        ra = _var_call(hip, a, False, slots, ivs, aad_blob, aoff, blob, doff)
        rb = _var_call(hip, b, False, slots, ivs, aad_blob, aoff, blob, doff)
        assert ra[0] == rb[0] and ra[1] == rb[1]
        assert a.status() == (hip.OK, 0)
        assert b.status() == (hip.EARG, n_slots)
