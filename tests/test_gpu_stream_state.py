"""GPU: the state of a message under way can leave its context (round 6) -- aesgcm_stream_export / aesgcm_stream_import / aesgcm_stream_update_dev.
The RTL holds that state in its Y register (src/gcm_ghash.vhd:174-186) and its block counter (src/aes_icb.vhd:97-100) and cannot hand it out, nor can the
pycryptodome model (tb/gcm_model.py); SURVEY.md 5 (checkpoint / resume) and 8(f2) name it as what a pipeline around the core has to carry.  Here a message of
unknown total length moves between contexts, between the host-buffer and the device-pointer form of the call, and between PROCESSES through a file; ciphertext and
tag always equal the oracle's one-shot result."""
import json
import os
import random
import struct
import subprocess
import sys

import pytest

from oracle import oracle as O
from util import splitmix_bytes

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cuts(rng, n, pieces):
    """pieces - 1 random 16-byte boundaries inside [0, n)"""
    pts = sorted(set(16 * rng.randrange(0, n // 16 + 1) for _ in range(pieces - 1)))
    return [0] + pts + [n]


@pytest.mark.parametrize("klen,n,aad_len,pieces", [(16, 1000, 0, 3), (24, 70000, 20, 4), (32, (3 << 20) + 5, 37, 5), (32, 16 * 4096, 16, 2), (16, 0, 9, 2), (32, (24 << 20) + 16 * 3 + 1, 0, 3)])
def test_split_at_random_block_boundaries_across_two_contexts(hip, orc, klen, n, aad_len, pieces):
    """every piece on the other context: export from the one that did the last piece, import into the other -- host-buffer updates for small pieces, device-pointer
    updates (any size: cyclic rows and dealt chunks for the multi-MiB pieces) for the rest; encrypt, then decrypt the same way"""
    rng = random.Random(8000 + n % 1000 + klen)
    key, iv, aad, pt = splitmix_bytes(8001 + klen, klen), splitmix_bytes(8002, 12), splitmix_bytes(8003, aad_len), splitmix_bytes(8004 + n % 97, n)
    want_ct, want_tag = orc.Fast(key).encrypt(iv, aad, pt)
    ctxs = [hip.Context(key), hip.Context(key)]
    d_in, d_out = hip.DeviceBuffer(max(n, 16)), hip.DeviceBuffer(max(n, 16))
    for dec in (False, True):
        src, want = (want_ct, pt) if dec else (pt, want_ct)
        if n:
            d_in.upload(src)
        cuts = _cuts(rng, n, pieces)
        ctxs[0].stream_begin(iv, decrypt=dec)
        a_cut = aad_len // 2 // 16 * 16                          # the AAD in two beats as well, the second on the other context
        if aad_len:
            ctxs[0].stream_aad(aad[:a_cut])
            ctxs[1].stream_import(ctxs[0].stream_export())
            ctxs[1].stream_aad(aad[a_cut:])
            ctxs[0], ctxs[1] = ctxs[1], ctxs[0]
            with pytest.raises(hip.AesGcmError):                 # the context the state came from still has its session open: importing back into it is refused ...
                ctxs[1].stream_import(ctxs[0].stream_export())
            ctxs[1].stream_final()                               # ... until it is closed
        out = bytearray(n)
        for k in range(len(cuts) - 1):
            lo, hi = cuts[k], cuts[k + 1]
            c = ctxs[0]
            if hi - lo <= 4096 and rng.random() < 0.5:
                out[lo:hi] = c.stream_update(src[lo:hi])
            else:
                c.stream_update_dev(d_in.ptr + lo, hi - lo, d_out.ptr + lo)
                hip.dev_sync()
                out[lo:hi] = d_out.download(hi - lo, lo)
            if k + 2 < len(cuts):                                # hand over
                blob = c.stream_export()
                assert len(blob) == 64 and key not in blob and key[:8] not in blob
                ctxs[1].stream_import(blob)
                c.stream_final()                                 # the old context's session: closed with whatever tag it would have had
                ctxs[0], ctxs[1] = ctxs[1], ctxs[0]
        tag = ctxs[0].stream_final()
        assert bytes(out) == want and tag == want_tag, (dec, n, cuts)


def test_refusals(hip, orc):
    key, other_key, iv = splitmix_bytes(8100, 32), splitmix_bytes(8101, 32), splitmix_bytes(8102, 12)
    a, b, c = hip.Context(key), hip.Context(key), hip.Context(other_key)
    with pytest.raises(hip.AesGcmError) as ei:
        a.stream_export()                                        # no session
    assert ei.value.code == hip.ESTATE
    a.stream_begin(iv)
    a.stream_aad(b"header")
    a.stream_update(bytes(64))
    blob = a.stream_export()
    with pytest.raises(hip.AesGcmError) as ei:
        c.stream_import(blob)                                    # another key
    assert ei.value.code == hip.EARG
    for i in (0, 1, 20, 40, 63):
        bad = bytearray(blob); bad[i] ^= 0x10
        with pytest.raises(hip.AesGcmError) as ei:
            b.stream_import(bytes(bad))                          # damaged
        assert ei.value.code == hip.EARG
    b.stream_import(blob)
    with pytest.raises(hip.AesGcmError) as ei:
        b.stream_import(blob)                                    # a session is open
    assert ei.value.code == hip.ESTATE
    with pytest.raises(hip.AesGcmError) as ei:
        b.stream_aad(b"more")                                    # the imported state knows that data has begun
    assert ei.value.code == hip.ESTATE
    d = hip.DeviceBuffer(64)
    with pytest.raises(hip.AesGcmError) as ei:
        b.stream_update_dev(d.ptr + 4, 32, d.ptr)                # alignment
    assert ei.value.code == hip.EALIGN
    # both go on from the same point and agree with the oracle
    tail = splitmix_bytes(8103, 100)
    want_ct, want_tag = orc.Fast(key).encrypt(iv, b"header", bytes(64) + tail)
    for x in (a, b):
        assert x.stream_update(tail) == want_ct[64:] and x.stream_final() == want_tag
    a.stream_begin(iv)
    with pytest.raises(hip.AesGcmError) as ei:
        a.encrypt_pipelined(iv, b"", bytes(100))                 # the pipelined path keeps its state in the same slot: refused inside an open session
    assert ei.value.code == hip.ESTATE
    a.stream_final()
    assert a.encrypt_pipelined(iv, b"header", bytes(64) + tail) == (want_ct, want_tag)      # ... and is itself a session that closes behind it
    a.stream_begin(iv)
    a.stream_final()
    # blobs whose fields disagree, with a valid sum check (it is no signature: anyone can recompute it) -- refused, and the genuine blob still taken afterwards
    a.stream_begin(iv)
    a.stream_aad(b"thirteen byte")                               # ragged AAD: bit 1 of byte 2 set, no data yet
    ragged_aad = a.stream_export()
    a.stream_final()
    a.stream_begin(iv)
    a.stream_aad(bytes(16))
    a.stream_update(bytes(64))                                   # data begun, aligned: bit 0 alone
    aligned_data = a.stream_export()
    a.stream_final()
    assert ragged_aad[2] == 2 and aligned_data[2] == 1
    for genuine, flags in ((ragged_aad, 0), (aligned_data, 3), (aligned_data, 0)):
        bad = bytearray(genuine)
        bad[2] = flags                                           # ragged AAD without the ragged bit / the ragged bit on aligned data / data 0 with len 64
        bad[60:64] = struct.pack("<I", _blob_sum(bad))
        with pytest.raises(hip.AesGcmError) as ei:
            b.stream_import(bytes(bad))
        assert ei.value.code == hip.EARG, (genuine.hex(), flags)
        b.stream_import(genuine)
        b.stream_final()


def _blob_sum(blob):
    """the blob's sum check over its first 60 bytes (aesgcm_abi.hip blob_sum)"""
    s = 0x5EC0DE5
    for x in blob[:60]:
        s = (((s << 5) | (s >> 27)) & 0xFFFFFFFF) ^ x
    return s


def _gf_inverse(x):
    """x^(2^128 - 2) in GCM's field (bytes in GCM's order), by square and multiply with the oracle's gfmul"""
    r, p = b"\x80" + bytes(15), x                              # r = 1
    e = (1 << 128) - 2
    while e:
        if e & 1:
            r = O.gfmul(r, p)
        p = O.gfmul(p, p)
        e >>= 1
    return r


@pytest.mark.parametrize("klen", [16, 32])
def test_the_exported_state_gives_the_authentication_key(hip, klen):
    """what include/aesgcm.h says of the blob: it holds no key, but it is worth H.  The running value is in the library's form (sum X_i H^(n-1-i)), so after two
    AAD blocks it is X0 H ^ X1, and H = (Y ^ X1) X0^-1 -- from the blob and the public AAD alone"""
    key, iv = splitmix_bytes(8200 + klen, klen), splitmix_bytes(8201, 12)
    x0, x1 = splitmix_bytes(8202, 16), splitmix_bytes(8203, 16)
    ctx = hip.Context(key)
    ctx.stream_begin(iv)
    ctx.stream_aad(x0 + x1)
    blob = ctx.stream_export()
    ctx.stream_final()
    y = blob[32:48]
    h = O.gfmul(bytes(a ^ b for a, b in zip(y, x1)), _gf_inverse(x0))
    assert O.gfmul(x0, _gf_inverse(x0)) == b"\x80" + bytes(15)
    assert h == ctx.h()


def _session(hip, ctx, blockers, steps, iv, aad, src, d_in, d_out, dec, fresh):
    """one session of `ctx` through `steps`, nothing synchronised on the host between them.  ("dev", n, k): the next n bytes by stream_update_dev on the stream of
    blockers[k] (None: the context's own) behind a long encryption queued there first -- any step not ordered behind the chunk overtakes it; ("host", n): the next n
    bytes by stream_update; ("move",): export, import into `fresh`, go on there.  Returns (output bytes of the host steps by offset, the context that closes, tag)"""
    ctx.stream_begin(iv, decrypt=dec)
    if aad:
        ctx.stream_aad(aad)
    host_out, pos = {}, 0
    for st in steps:
        if st[0] == "dev":
            n, k = st[1], st[2]
            stream = None
            if k is not None:
                other, big = blockers[k]
                other.encrypt_dev(iv, big.ptr, big.nbytes, big.ptr, stream=other.stream(), want_tag=False)
                stream = other.stream()
            ctx.stream_update_dev(d_in.ptr + pos, n, d_out.ptr + pos, stream=stream)
            pos += n
        elif st[0] == "host":
            host_out[pos] = ctx.stream_update(src[pos:pos + st[1]])
            pos += st[1]
        else:
            fresh.stream_import(ctx.stream_export())
            ctx.stream_final()
            ctx = fresh
    return host_out, ctx.stream_final()


MB = 1 << 20
SEQUENCES = {
    "dev_then_final": [("dev", 5 * MB + 16 * 3 + 7, 0)],
    "three_streams": [("dev", 16 * 1000, 0), ("dev", 5 * MB, 1), ("dev", 16 * 77 + 9, None)],
    "dev_then_host_tail": [("dev", 5 * MB, 0), ("host", 1000 + 5)],
    "dev_then_export_import": [("dev", 3 * MB, 0), ("move",), ("dev", 16 * 9 + 1, 1)],
}


@pytest.mark.parametrize("seq", sorted(SEQUENCES))
def test_a_session_fed_from_other_streams_is_ordered(hip, orc, seq):
    """aesgcm_stream_update_dev on a CALLER's stream, the session's other steps on the context's: the library orders them on the device (an event recorded behind
    every step, waited for by the next).  Three sessions at once (AES-128 / 192 / 256, AAD of 0 / 13 / 28 bytes), each fed from the streams of other contexts that
    are busy with a 1 GiB encryption when the chunk is queued; ciphertext and tag against the oracle, both directions"""
    steps = SEQUENCES[seq]
    n = sum(st[1] for st in steps if st[0] != "move")
    blockers = []
    for k in range(3):
        other = hip.Context(splitmix_bytes(8300 + k, 32))
        big = hip.DeviceBuffer(1 << 30)
        big.fill_splitmix64(8310 + k)
        blockers.append((other, big))
    sessions = []
    for j, (klen, aad_len) in enumerate(((16, 0), (24, 13), (32, 28))):
        key, iv, aad = splitmix_bytes(8320 + j, klen), splitmix_bytes(8330 + j, 12), splitmix_bytes(8340 + j, aad_len)
        pt = splitmix_bytes(8350 + j, n)
        ct, tag = orc.Fast(key).encrypt(iv, aad, pt)
        sessions.append(dict(ctx=hip.Context(key), fresh=hip.Context(key), iv=iv, aad=aad, pt=pt, ct=ct, tag=tag,
                             d_in=hip.DeviceBuffer(n + 16), d_out=hip.DeviceBuffer(n + 16)))
    hip.dev_sync()
    for dec in (False, True):
        for j, s in enumerate(sessions):
            s["d_in"].upload(s["ct"] if dec else s["pt"])
            s["d_out"].upload(bytes(n + 16))
        results = []
        for j, s in enumerate(sessions):
            mine = blockers[j:] + blockers[:j]                   # session j's "stream 0" is blocker j's, "stream 1" the next one's
            results.append(_session(hip, s["ctx"], mine, steps, s["iv"], s["aad"], s["pt"] if not dec else s["ct"], s["d_in"], s["d_out"], dec, s["fresh"]))
        hip.dev_sync()
        for j, (s, (host_out, tag)) in enumerate(zip(sessions, results)):
            got = bytearray(s["d_out"].download(n))
            for pos, b in host_out.items():
                got[pos:pos + len(b)] = b
            want = s["pt"] if dec else s["ct"]
            assert tag == s["tag"], (seq, dec, j, "tag")
            assert bytes(got) == want, (seq, dec, j, "data")


CHILD = r"""
import json, sys
sys.path.insert(0, %(root)r)
import aesgcm_amd
from aesgcm_amd import lib
key, iv, aad = (bytes.fromhex(x) for x in sys.argv[1:4])
head = open(sys.argv[4], "rb").read()
c = lib.Context(key)
c.stream_begin(iv)
c.stream_aad(aad)
d = lib.DeviceBuffer(max(len(head), 16)); d.upload(head)
c.stream_update_dev(d.ptr, len(head), d.ptr)
blob = c.stream_export()
json.dump({"blob": blob.hex(), "ct": bytes(d.download(len(head))).hex()}, open(sys.argv[5], "w"))
"""


def test_across_two_processes_through_a_file(hip, orc, tmp_path):
    """process 1 absorbs the AAD and the first 1 MiB + 48 bytes on device pointers, writes the 64-byte state and its ciphertext to a file and exits; this process
    imports the state into a fresh context and finishes the message"""
    key, iv, aad = splitmix_bytes(8200, 32), splitmix_bytes(8201, 12), splitmix_bytes(8202, 28)
    pt = splitmix_bytes(8203, (1 << 20) + 48 + 70001)
    cut = (1 << 20) + 48
    path, head = str(tmp_path / "state.json"), str(tmp_path / "head.bin")
    with open(head, "wb") as fh:
        fh.write(pt[:cut])
    p = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT}, key.hex(), iv.hex(), aad.hex(), head, path], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    st = json.load(open(path))
    c = hip.Context(key)
    c.stream_import(bytes.fromhex(st["blob"]))
    rest = c.stream_update(pt[cut:])
    tag = c.stream_final()
    assert (bytes.fromhex(st["ct"]) + rest, tag) == orc.Fast(key).encrypt(iv, aad, pt)
