"""GPU: SSH binary packets in wire format through key tables (aesgcm_keytab_ssh_crypt_dev; RFC 5647 7.1 - 7.3, OpenSSH PROTOCOL 1.6: packet_length[4] | body | tag,
AAD = the length field, nonce = the slot's IV with its last eight bytes incremented once per packet) and SSH's key derivation on the device (aesgcm_sshkdf_*,
lib.SshKexTable; RFC 4253 7.2).  The reference is tests/ssh_fixture.py: nonce, AAD and KDF from the RFCs' formulas in Python, the AEAD by libcrypto, the hash by
hashlib -- no published vector is at hand (tests/COVERAGE_ssh.md).  Every case runs between guard bytes and compares every byte of the buffer, in place and out of
place, encrypt and then decrypt.
  packets      every body size x the three key sizes x 1 / 257 / 4097 packets (each lane shape); the counter's carries against an XOR of the same inputs; one refusal
               of every kind among good packets; a tampered length field, body or tag, and the wipe; a captured assign + encrypt replayed three times
  SshKexTable  3 hashes x 3 key sizes at 1 / 257 / 4097 entries, through the packets the installed slots encrypt; the padding edges of both block sizes; one
               direction only; refusals of every kind; a re-exchange; a captured install + encrypt"""
import random
import struct

import pytest

import hip_graph as G
import ssh_fixture as SSH
from kt_common import CANARY, _collect, _layout, _u32, _u64, _up, evp  # noqa: F401
from util import splitmix_bytes

pytestmark = pytest.mark.gpu

BODIES = (16, 32, 48, 112, 128, 144, 1008, 1024, 32768)
COUNTS = (1, 257, 4097)
KEY_LENS = (16, 24, 32)
NONE = 0xFFFFFFFF


def _run(hip, kt, decrypt, slots, seqs, off, buf, inplace, out_fill=CANARY):
    n = len(slots)
    d = {"slots": _up(hip, _u32(slots)), "in": _up(hip, buf), "off": _up(hip, _u64(off)), "seq": _up(hip, _u64(seqs))}
    d["out"] = d["in"] if inplace else _up(hip, bytes([out_fill]) * len(buf))
    d["auth"] = _up(hip, b"\x07" * 4 * n) if decrypt else None
    kt.ssh_crypt_dev(decrypt, n, d["slots"].ptr, d["seq"].ptr, d["in"].ptr, d["off"].ptr, d["out"].ptr, d_auth=d["auth"].ptr if decrypt else None)
    d["nbytes"], d["n"] = len(buf), n
    return _collect(hip, d)


def _table(hip, key_len, n_slots, seed, ivs=None):
    keys = splitmix_bytes(seed, key_len * n_slots)
    if ivs is None:
        ib = splitmix_bytes(seed + 1, 12 * n_slots)
        ivs = [ib[12 * s:12 * s + 12] for s in range(n_slots)]
    kt = hip.KeyTable(key_len, n_slots)
    kt.set(0, keys)
    kt.set_tls_iv(0, b"".join(ivs))
    return kt, keys, ivs


def _both_ways(hip, evp, kt, keys, ivs, key_len, slots, seqs, pkts, lead, inplace):
    """encrypt against the fixture, every byte of the buffer; then the fixture's packets back to the plaintext with every tag accepted (the tag's bytes stay)"""
    n = len(pkts)
    off, buf = _layout(pkts, lead)
    want = SSH.ref_encrypt(evp, key_len, keys, ivs, slots, seqs, pkts)
    _, want_buf = _layout(want, lead)
    out, _, _ = _run(hip, kt, False, slots, seqs, off, buf, inplace)
    if out != want_buf:                                                  # name the first packet that differs
        for p in range(n):
            assert out[off[p]:off[p + 1]] == want[p], (p, len(pkts[p]), seqs[p])
    assert out == want_buf
    back, auth, _ = _run(hip, kt, True, slots, seqs, off, want_buf, inplace)
    _, plain_buf = _layout([r[:-16] + w[-16:] for r, w in zip(pkts, want)], lead)
    assert back == plain_buf
    assert auth == [1] * n
    assert kt.status() == (hip.OK, 0)
    return want


# ---------------------------------------------------------------- packets
@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("key_len", KEY_LENS)
def test_every_body_size_key_size_and_lane_shape(hip, evp, key_len, n):
    """1 packet: 8 lanes per packet; 257: 16; 4097: 64 (the plan is by count).  One packet: the longest body; otherwise every body size in turn, the longest once"""
    rng = random.Random("ssh %d %d" % (key_len, n))
    bodies = [32768] if n == 1 else [BODIES[p % 8] for p in range(n)]
    if n > 1:
        bodies[n // 2] = 32768
    n_slots = min(n, 64)
    kt, keys, ivs = _table(hip, key_len, n_slots, 0x55100 + 16 * key_len + n)
    try:
        slots = [rng.randrange(n_slots) for _ in range(n)]
        slots[0], slots[-1] = 0, n_slots - 1
        seqs = [rng.getrandbits(64) if p % 3 == 0 else rng.randrange(1 << 20) for p in range(n)]
        inplace = (key_len // 8 + COUNTS.index(n)) % 2 == 0
        _both_ways(hip, evp, kt, keys, ivs, key_len, slots, seqs, SSH.make_packets(0x55110 + n + key_len, bodies), 16 if key_len == 24 else 13, inplace)
    finally:
        kt.close()


@pytest.mark.parametrize("inplace", [True, False])
def test_counter_carries_and_the_fixed_field(hip, evp, inplace):
    """ctr0 = 00000000 FFFFFFFF with 0, 1, 2 (the low word's carry) and FFFFFFFF FFFFFFFE with 1, 2, 3 (the wrap at 2^64: the fixed field must stay).  An XOR nonce of
    the same inputs gives other tags where a carry runs -- were it not so, these cases would prove nothing"""
    key_len = 32
    ivs = [bytes.fromhex("a1b2c3d4" "00000000ffffffff"), bytes.fromhex("ffffffff" "fffffffffffffffe")]
    kt, keys, _ = _table(hip, key_len, 2, 0x55200, ivs)
    try:
        slots, seqs = [0, 0, 0, 1, 1, 1], [0, 1, 2, 1, 2, 3]
        pkts = SSH.make_packets(0x55210, [16, 48, 32, 16, 144, 32])
        want = _both_ways(hip, evp, kt, keys, ivs, key_len, slots, seqs, pkts, 5, inplace)
        xored = SSH.ref_encrypt(evp, key_len, keys, ivs, slots, seqs, pkts, nonce=SSH.nonce_xor)
        carries = [p for p in range(6) if SSH.nonce_of(ivs[slots[p]], seqs[p]) != SSH.nonce_xor(ivs[slots[p]], seqs[p])]
        assert carries == [1, 2, 4, 5]
        for p in carries:
            assert want[p][-16:] != xored[p][-16:] and want[p][4:-16] != xored[p][4:-16], p
        assert [SSH.nonce_of(ivs[1], s)[:4] for s in (1, 2, 3)] == [b"\xff" * 4] * 3 and SSH.nonce_of(ivs[1], 2)[4:] == bytes(8)
    finally:
        kt.close()


def test_one_refusal_of_every_kind_among_good_packets(hip, evp):
    rng = random.Random("ssh refusals")
    key_len, n_slots, m = 16, 8, 30
    kt, keys, ivs = _table(hip, key_len, n_slots, 0x55300)
    try:
        kt.clear(6)                                                          # a cleared slot, which only packet 5 names
        pkts = SSH.make_packets(0x55310, [16 * rng.randrange(1, 9) for _ in range(m)])
        slots = [rng.randrange(6) for _ in range(m)]
        seqs = [rng.getrandbits(64) for _ in range(m)]
        slots[3] = n_slots                                                   # slot out of range
        slots[5] = 6                                                         # slot unset
        pkts[8] = splitmix_bytes(0x55311, 35)                                # L < 36
        pkts[9] = struct.pack(">I", 0) + b"\xAA" * 16                        # ... no body at all, the field right
        pkts[11] = struct.pack(">I", 24) + splitmix_bytes(0x55312, 24) + b"\xAA" * 16       # B % 16 != 0, the field right
        pkts[14] = struct.pack(">I", len(pkts[14]) - 20 + 16) + pkts[14][4:]                # a length field that says one block more
        pkts[15] = b"\x80" + pkts[15][1:]                                                   # ... and one with a high byte set
        off, buf = _layout(pkts, 11)
        # two more entries: [A, A - 3) falls; [A - 3, A - 3 + 2^28) is too long -- neither is read, so neither needs its bytes to exist
        off += [off[m] - 3]
        off += [off[m + 1] + (1 << 28)]
        slots += [0, 1]
        seqs += [7, 8]
        n = m + 2
        refused = {3, 5, 8, 9, 11, 14, 15, m, m + 1}
        ok = [p for p in range(n) if p not in refused]
        ref = dict(zip(ok, SSH.ref_encrypt(evp, key_len, keys, ivs, [slots[p] for p in ok], [seqs[p] for p in ok], [pkts[p] for p in ok])))
        for inplace, fill in ((True, None), (False, 0x3C)):
            want = bytearray(buf if inplace else bytes([fill]) * len(buf))
            for p in ok:
                want[off[p]:off[p + 1]] = ref[p]
            out, _, _ = _run(hip, kt, False, slots, seqs, off, buf, inplace, out_fill=fill or 0)
            assert out == bytes(want), inplace
            assert kt.status() == (hip.EARG, 3)                              # the lowest refused index
            assert kt.status() == (hip.OK, 0)
            enc = bytearray(buf)
            for p in ok:
                enc[off[p]:off[p + 1]] = ref[p]
            back, auth, _ = _run(hip, kt, True, slots, seqs, off, bytes(enc), inplace, out_fill=fill or 0)
            assert auth == [0 if p in refused else 1 for p in range(n)]
            wantp = bytearray(enc if inplace else bytes([fill]) * len(buf))
            for p in ok:
                wantp[off[p]:off[p + 1]] = pkts[p][:-16] + ref[p][-16:]
            assert back == bytes(wantp), inplace
            assert kt.status() == (hip.EARG, 3)
    finally:
        kt.close()


def test_tampering_and_wipe(hip, evp):
    """a flipped bit in the length field (the packet is refused: the field no longer says the body's length), the body or the tag fails that packet alone, and
    aesgcm_wipe_failed_dev zeroes exactly those"""
    rng = random.Random("ssh tamper")
    key_len, n_slots, n = 32, 5, 40
    kt, keys, ivs = _table(hip, key_len, n_slots, 0x55400)
    try:
        pkts = SSH.make_packets(0x55410, [16 * rng.randrange(1, 12) for _ in range(n)])
        slots = [rng.randrange(n_slots) for _ in range(n)]
        seqs = [rng.getrandbits(64) for _ in range(n)]
        off, _ = _layout(pkts, 9)
        encs = SSH.ref_encrypt(evp, key_len, keys, ivs, slots, seqs, pkts)
        _, ebuf = _layout(encs, 9)
        tam = bytearray(ebuf)
        hits = {0: 4, 4: -1, 10: 3, 20: 0, 38: -16, 30: 9, 33: 2}             # body, the tag's last and first byte, the length field's four bytes
        for p, b in hits.items():
            tam[(off[p] if b >= 0 else off[p + 1]) + b] ^= 0x10
        back, auth, d = _run(hip, kt, True, slots, seqs, off, bytes(tam), False, out_fill=0x3C)
        assert auth == [0 if p in hits else 1 for p in range(n)]
        for p in range(n):
            if p not in hits:
                assert back[off[p]:off[p + 1]] == pkts[p][:-16] + encs[p][-16:], p
        for p in (10, 20, 33):                                               # refused: nothing of them was written
            assert back[off[p]:off[p + 1]] == b"\x3C" * len(pkts[p]), p
        assert back[:9] == b"\x3C" * 9 and back[off[n]:] == b"\x3C" * 37
        assert kt.status() == (hip.EARG, 10)
        hip.wipe_failed_dev(n, d["out"].ptr, d["auth"].ptr, d_data_off=d["off"].ptr)
        hip.dev_sync()
        wiped = bytes(d["out"].download(len(ebuf)))
        for p in range(n):
            assert wiped[off[p]:off[p + 1]] == (back[off[p]:off[p + 1]] if auth[p] else bytes(off[p + 1] - off[p])), p
        assert wiped[:9] == b"\x3C" * 9 and wiped[off[n]:] == b"\x3C" * 37
    finally:
        kt.close()


def test_call_level_refusals_and_crypt_ssh(hip, evp):
    key_len, n_slots = 16, 3
    kt, keys, ivs = _table(hip, key_len, n_slots, 0x55500)
    try:
        d = _up(hip, bytes(256))
        for args in ((False, 1, d.ptr, None, d.ptr, d.ptr, d.ptr), (True, 1, d.ptr, d.ptr, d.ptr, d.ptr, d.ptr)):      # no d_seq; decrypt without d_auth
            with pytest.raises(hip.AesGcmError) as e:
                kt.ssh_crypt_dev(*args)
            assert e.value.code == hip.EARG
        pkts = SSH.make_packets(0x55510, [16, 32, 48, 64, 16, 128, 80])
        slots, seqs = [p % n_slots for p in range(7)], [0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 64 - 1, 5, 6]
        out, auth = kt.crypt_ssh(slots, seqs, pkts)
        assert auth is None and out == SSH.ref_encrypt(evp, key_len, keys, ivs, slots, seqs, pkts)
        back, auth = kt.crypt_ssh(slots, seqs, out, decrypt=True)
        assert auth == [1] * 7 and [b[:-16] for b in back] == [r[:-16] for r in pkts]
        assert kt.status() == (hip.OK, 0)
    finally:
        kt.close()


def test_captured_assign_and_encrypt_replayed_three_times(hip, evp):
    """send counters reset to 0 at key install hand each packet the count of the packets sent before it under its key: assign (number only) + encrypt in one graph"""
    rng = random.Random("ssh capture")
    key_len, n_slots, n = 32, 6, 200
    kt, keys, ivs = _table(hip, key_len, n_slots, 0x55600)
    pkts = SSH.make_packets(0x55610, [16 * rng.randrange(1, 10) for _ in range(n)])
    slots = [rng.randrange(n_slots) for _ in range(n)]
    off, buf = _layout(pkts, 7)
    st = G.stream_create()
    bufs = []
    try:
        with hip.TxCounters(n_slots, n) as tx:
            tx.set(0, [0] * n_slots, [1 << 40] * n_slots)                        # a connection's counter is its slot's number here
            hip.dev_sync()
            d_slots, d_off, d_in, d_out, d_num = _up(hip, _u32(slots)), _up(hip, _u64(off)), _up(hip, buf), _up(hip, bytes([CANARY]) * len(buf)), _up(hip, bytes(8 * n))
            bufs = [d_slots, d_off, d_in, d_out, d_num]
            fmt = hip.TxFormat.number_only()

            def enqueue():
                tx.assign_dev(fmt, n, d_slots.ptr, None, None, d_num.ptr, stream=st)
                kt.ssh_crypt_dev(0, n, d_slots.ptr, d_num.ptr, d_in.ptr, d_off.ptr, d_out.ptr, stream=st)

            sent = [0] * n_slots

            def expect():
                seqs = []
                for s in slots:
                    seqs.append(sent[s])
                    sent[s] += 1
                return _layout(SSH.ref_encrypt(evp, key_len, keys, ivs, slots, seqs, pkts), 7)[1]

            enqueue()                                                            # the ordinary call of each, before the capture
            G.synchronize(st)
            assert bytes(d_out.download(len(buf))) == expect()
            with G.Graph(st, enqueue) as graph:
                for r in range(3):
                    graph.launch()
                    assert bytes(d_out.download(len(buf))) == expect(), r
            assert tx.status() == (hip.OK, 0) and kt.status() == (hip.OK, 0)
    finally:
        for x in bufs:
            x.free()
        kt.close()
        G.stream_destroy(st)


# ---------------------------------------------------------------- SshKexTable
def _records(rng, hl, n, lens):
    return [(rng.getrandbits(8 * ln).to_bytes(ln, "big"), rng.getrandbits(8 * hl).to_bytes(hl, "big")) for ln in (lens[i % len(lens)] for i in range(n))]


def _check_slots(hip, evp, kt, key_len, n_slots, material, seed):
    """material: {slot: (key, iv)} of the installed slots; every other slot must still be unset.  Every slot encrypts one packet, in place: the installed ones as the
    fixture says under their derived key and IV, the others' packets are refused and untouched"""
    pkts = SSH.make_packets(seed, [16 * (1 + s % 3) for s in range(n_slots)])
    slots, seqs = list(range(n_slots)), [(s * 0x9E3779B97F4A7C15) & SSH.MASK64 if s % 2 else s for s in range(n_slots)]
    ok = sorted(material)
    dense = {s: i for i, s in enumerate(ok)}
    ref = SSH.ref_encrypt(evp, key_len, b"".join(material[s][0] for s in ok), [material[s][1] for s in ok], [dense[s] for s in ok], [seqs[s] for s in ok], [pkts[s] for s in ok])
    want = list(pkts)
    for s, r in zip(ok, ref):
        want[s] = r
    off, buf = _layout(pkts, 3)
    out, _, _ = _run(hip, kt, False, slots, seqs, off, buf, True)
    if out != _layout(want, 3)[1]:
        for s in range(n_slots):
            assert out[off[s]:off[s + 1]] == want[s], (s, s in material)
    assert out == _layout(want, 3)[1]
    unset = [s for s in range(n_slots) if s not in material]
    assert kt.status() == ((hip.EARG, unset[0]) if unset else (hip.OK, 0))


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("key_len", KEY_LENS)
@pytest.mark.parametrize("hl", (32, 48, 64))
def test_install_every_hash_and_key_size(hip, evp, hl, key_len, n):
    """n connections, both directions of each into 2n slots in a shuffled order; records by the host's set (even runs) or set_dev"""
    rng = random.Random("sshkdf %d %d %d" % (hl, key_len, n))
    recs = _records(rng, hl, n, (37, 1, 133, 64, 260, 97))
    perm = list(range(n))
    rng.shuffle(perm)
    c2s, s2c = [2 * perm[i] for i in range(n)], [2 * perm[i] + 1 for i in range(n)]
    with hip.SshKexTable(hl, n, max_secret_len=260) as sk, hip.KeyTable(key_len, 2 * n) as kt:
        if (hl + key_len + n) % 2 == 0:
            sk.set(0, [r[0] for r in recs], [r[1] for r in recs])
        else:
            packed, soff = b"".join(r[0] for r in recs), [0]
            for r in recs:
                soff.append(soff[-1] + len(r[0]))
            bufs = [_up(hip, _u32(list(range(n)))), _up(hip, packed), _up(hip, _u32(soff)), _up(hip, b"".join(r[1] for r in recs))]
            sk.set_dev(n, *[b.ptr for b in bufs])
            hip.dev_sync()
            for b in bufs:
                b.free()
        sk.install(kt, list(range(n)), c2s, s2c)
        assert sk.status() == (hip.OK, 0)
        material = {}
        for i, (secret, sid) in enumerate(recs):
            material[c2s[i]], material[s2c[i]] = SSH.derive(hl, secret, sid, key_len)
        _check_slots(hip, evp, kt, key_len, 2 * n, material, 0x55700 + n)


@pytest.mark.parametrize("hl", (32, 48, 64))
def test_secret_lengths_at_the_padding_edges_of_both_block_sizes(hip, evp, hl):
    lens = (1, 55, 56, 63, 64, 111, 112, 119, 120, 127, 128, 129, 300, 2048)
    rng = random.Random("sshkdf edges %d" % hl)
    n, key_len = len(lens), (16, 24, 32)[hl // 16 - 2]
    recs = _records(rng, hl, n, lens)
    with hip.SshKexTable(hl, n, max_secret_len=2048) as sk, hip.KeyTable(key_len, 2 * n) as kt:
        sk.set(0, [r[0] for r in recs], [r[1] for r in recs])
        sk.install(kt, list(range(n)), list(range(n)), list(range(n, 2 * n)))
        assert sk.status() == (hip.OK, 0)
        material = {}
        for i, (secret, sid) in enumerate(recs):
            material[i], material[n + i] = SSH.derive(hl, secret, sid, key_len)
        _check_slots(hip, evp, kt, key_len, 2 * n, material, 0x55800)


def test_one_direction_refusals_and_a_re_exchange(hip, evp):
    hl, key_len, n_recs, n_slots = 32, 16, 8, 24
    rng = random.Random("sshkdf refusals")
    recs = _records(rng, hl, n_recs, (40, 70, 100))
    with hip.SshKexTable(hl, n_recs, max_secret_len=100) as sk, hip.KeyTable(key_len, n_slots) as kt:
        with pytest.raises(hip.AesGcmError) as e:
            sk.set(0, [bytes(101)], [bytes(hl)])                                 # longer than max_secret_len: nothing stored
        assert e.value.code == hip.EARG
        with pytest.raises(hip.AesGcmError) as e:
            sk.set(0, [b""], [bytes(hl)])
        assert e.value.code == hip.EARG
        sk.set(0, [r[0] for r in recs[:6]], [r[1] for r in recs[:6]])            # records 6 and 7 stay unset
        sk.clear(5)
        material = {}

        def dv(r):
            return SSH.derive(hl, recs[r][0], recs[r][1], key_len)
        # one direction only: an array missing, and entries that name no slot
        sk.install(kt, [0, 1], c2s_slots=[0, 1])
        material[0], material[1] = dv(0)[0], dv(1)[0]
        sk.install(kt, [0, 1], s2c_slots=[2, NONE])
        material[2] = dv(0)[1]
        sk.install(kt, [2, 3], c2s_slots=[NONE, 4], s2c_slots=[5, NONE])
        material[5], material[4] = dv(2)[1], dv(3)[0]
        assert sk.status() == (hip.OK, 0)
        # refusals, skipped whole: record out of range, unset, cleared; a slot out of range in either array -- the good entries between them are installed
        sk.install(kt, [4, n_recs, 6, 5, 1, 2, 3], c2s_slots=[6, 7, 8, 9, 10, n_slots, 12], s2c_slots=[13, 14, 15, 16, 17, 18, n_slots + 5])
        assert sk.status() == (hip.EARG, 1) and sk.status() == (hip.OK, 0)
        material[6], material[13] = dv(4)
        material[10], material[17] = dv(1)
        sk.install(kt, [2, 5], s2c_slots=[19, 20])                               # the reporter where the call has no client-to-server array
        assert sk.status() == (hip.EARG, 1)
        material[19] = dv(2)[1]
        # set_dev's refusals: record out of range, an empty secret, one too long, falling offsets
        bufs = [_up(hip, _u32([6, n_recs, 7, 7, 7])), _up(hip, bytes(range(200)) + bytes(200)), _up(hip, _u32([0, 50, 60, 60, 161, 150])), _up(hip, bytes(5 * hl))]
        sk.set_dev(5, *[b.ptr for b in bufs])
        hip.dev_sync()
        assert sk.status() == (hip.EARG, 1)
        for b in bufs:
            b.free()
        sk.install(kt, [6, 7], c2s_slots=[21, 22])
        assert sk.status() == (hip.EARG, 1)                                      # record 7 was never stored
        material[21] = SSH.derive(hl, bytes(range(50)), bytes(hl), key_len)[0]
        # a re-exchange: the new K | H under the same session identifier, installed into fresh slots; the old slots keep the old keys until they are cleared
        secret2 = rng.getrandbits(8 * 88).to_bytes(88, "big")
        sk.set(0, [secret2], [recs[0][1]])
        sk.install(kt, [0], c2s_slots=[11], s2c_slots=[23])
        material[11], material[23] = SSH.derive(hl, secret2, recs[0][1], key_len)
        assert material[11] != material[0] and sk.status() == (hip.OK, 0)
        _check_slots(hip, evp, kt, key_len, n_slots, material, 0x55900)


def test_captured_install_and_encrypt_replays_over_changed_secrets(hip, evp):
    n, hl, key_len = 100, 48, 32
    rng = random.Random("sshkdf capture")
    gens = [_records(rng, hl, n, (33, 64, 129, 200)) for _ in range(3)]
    pkts = SSH.make_packets(0x55A00, [16 * (1 + p % 5) for p in range(n)])
    off, buf = _layout(pkts, 0, 0)
    perm = list(range(n))
    rng.shuffle(perm)
    pslots = [p if p % 2 == 0 else n + p for p in range(n)]
    seqs = [p * 977 for p in range(n)]
    st = G.stream_create()
    with hip.SshKexTable(hl, n, max_secret_len=200) as sk, hip.KeyTable(key_len, 2 * n) as kt:
        sk.set(0, [r[0] for r in gens[0]], [r[1] for r in gens[0]])
        hip.dev_sync()
        bufs = [_up(hip, _u32(perm)), _up(hip, _u32(perm)), _up(hip, _u32([n + x for x in perm])), _up(hip, _u32(pslots)), _up(hip, _u64(seqs)), _up(hip, _u64(off)),
                _up(hip, buf), _up(hip, bytes(len(buf)))]
        d_idx, d_a, d_b, d_pslots, d_seq, d_off, d_in, d_out = bufs

        def enqueue():
            sk.install_dev(kt, n, d_idx.ptr, d_a.ptr, d_b.ptr, stream=st)
            kt.ssh_crypt_dev(0, n, d_pslots.ptr, d_seq.ptr, d_in.ptr, d_off.ptr, d_out.ptr, stream=st)

        try:
            enqueue()                                                           # the ordinary call of each
            G.synchronize(st)
            with G.Graph(st, enqueue) as graph:
                for g in range(3):
                    sk.set(0, [r[0] for r in gens[g]], [r[1] for r in gens[g]])  # outside the capture
                    hip.dev_sync()
                    graph.launch()
                    out = bytes(d_out.download(len(buf)))
                    keys, ivs = [None] * (2 * n), [None] * (2 * n)
                    for i in range(n):                                          # entry i installs record perm[i] into slots perm[i] and n + perm[i]
                        (keys[perm[i]], ivs[perm[i]]), (keys[n + perm[i]], ivs[n + perm[i]]) = SSH.derive(hl, gens[g][perm[i]][0], gens[g][perm[i]][1], key_len)
                    assert out == b"".join(SSH.ref_encrypt(evp, key_len, b"".join(keys), ivs, pslots, seqs, pkts)), g
            assert sk.status() == (hip.OK, 0) and kt.status() == (hip.OK, 0)
        finally:
            for x in bufs:
                x.free()
    G.stream_destroy(st)
