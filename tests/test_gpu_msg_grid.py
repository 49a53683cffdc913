"""GPU: single messages on caller-owned device memory -- aesgcm_encrypt_dev / aesgcm_decrypt_dev in every launch shape of the planner, aesgcm_shard_crypt_dev,
aesgcm_stream_update_dev and aesgcm_keystream_dev -- on the grid of tests/msg_grid.py: every message, shard, chunk and keystream run between canary bytes, every
arena compared WHOLE after the calls, inputs and AADs shown unchanged.  The reference is the CPU oracle (orc.Fast), never another GPU path, computed once per
shape and key size.  What the calls promise and this file holds them to (include/aesgcm.h): exactly `len` bytes of d_in and `aad_len` of d_aad are read, exactly
`len` bytes of d_out written -- a decrypt that failed verification with wipe_on_auth_fail zeroes exactly those -- and no slack behind a ragged end is needed.
Every call is shown to have taken the shape its case names (aesgcm_ctx_last_launch, aesgcm_ctx_split) where it is made; tests/fake_hip/msg_grid_drive.py holds
the same cells to their launch logs without a device."""
import numpy as np
import pytest

import grid_legs as GL
import msg_grid as MG
import pkt_grid as PG
from kt_common import Guarded, up_arena as _up
from util import splitmix_bytes

pytestmark = pytest.mark.gpu
_ARENAS = []                      # (shape, key size, leg) of every arena compared: the count the summary of a run names
_KEPT = {}                        # a leg's downloaded arena, for test_perturbed_references_are_reported


@pytest.fixture(scope="module")
def u(hip):
    return MG.units(hip)


def _context(hip, key, opts):
    c = hip.Context(key)
    for o, v in opts:
        c.set_option(o, v)
    return c


def _down(hip, d):
    hip.dev_sync()
    return bytes(d.download(d.size))


def _took(ctx, s, R, i, u, label):
    """the call just made took the shape the case names"""
    e = MG.expected(s, R.lens[i], R.aads[i], u)
    assert ctx.last_launch() == e["launch"], (label, "last_launch", ctx.last_launch(), e["launch"], R.grid.cell(i))
    assert e["split"] is None or ctx.split(R.lens[i]) == e["split"], (label, "split", ctx.split(R.lens[i]), e["split"], R.grid.cell(i))


def _legs(hip, orc, u, name, klen):
    s = MG.SHAPE[name]
    R = MG.reference(orc, name, klen, u)
    n, at, S = R.n, R.in_at, MG.SHIFT
    ctx = _context(hip, R.keys[0], s.opts)
    iv = lambda i: R.ivs[12 * i:12 * i + 12]
    tag = lambda t, i: t[16 * i:16 * i + 16]
    d_aad = _up(hip, R.aad_arena)
    aad = lambda i: dict(d_aad=d_aad.ptr + R.aad_at[i] if R.aads[i] else None, aad_len=R.aads[i])
    forged = set(R.forged)
    ct_arena = GL._assemble(R, R.pt_arena, at, "ct")                     # the oracle's ciphertext between the input's guards
    name = "%s AES-%d" % (name, 8 * klen)

    def compare(leg, d_buf, want, shift, keep=False):
        got = _down(hip, d_buf)
        MG.same(R, got, want, at, shift, name + " " + leg)
        _ARENAS.append((name, leg))
        if keep:
            _KEPT[name] = (R, got, want, at, shift)

    def unchanged(leg, d_in, arena):
        MG.same(R, _down(hip, d_in), arena, at, 0, name + " " + leg + " (input arena)")
        GL._same(R, d_aad, R.aad_arena, R.aad_at, 0, name + " " + leg + " (AAD arena)")

    # encrypt out of place; one message enqueued without a wait, its tag collected by aesgcm_last_tag
    d_pt, d_out, tags = _up(hip, R.pt_arena), _up(hip, GL._canary(R.size_out, S)), []
    for i in range(n):
        if i == n // 2:
            ctx.encrypt_dev(iv(i), d_pt.ptr + at[i], R.lens[i], d_out.ptr + S + at[i], want_tag=False, **aad(i))
            tags.append(ctx.last_tag())
        else:
            tags.append(ctx.encrypt_dev(iv(i), d_pt.ptr + at[i], R.lens[i], d_out.ptr + S + at[i], **aad(i)))
        _took(ctx, s, R, i, u, name + " enc")
    compare("enc out of place", d_out, GL._assemble(R, GL._canary(R.size_out, S), at, "ct", shift=S), S, keep=True)
    MG.tags_same(R, b"".join(tags), name + " enc out of place")
    unchanged("enc out of place", d_pt, R.pt_arena)
    # encrypt in place
    d_io = _up(hip, R.pt_arena)
    tags = [ctx.encrypt_dev(iv(i), d_io.ptr + at[i], R.lens[i], d_io.ptr + at[i], **aad(i)) for i in range(n)]
    compare("enc in place", d_io, ct_arena, 0)
    MG.tags_same(R, b"".join(tags), name + " enc in place")
    # decrypt the oracle's ciphertext out of place with the true tags
    d_ct, d_out, tags = _up(hip, ct_arena), _up(hip, GL._canary(R.size_out, S)), []
    for i in range(n):
        tags.append(ctx.decrypt_dev(iv(i), d_ct.ptr + at[i], R.lens[i], d_out.ptr + S + at[i], tag=tag(R.tags, i), **aad(i)))
        _took(ctx, s, R, i, u, name + " dec")
    compare("dec out of place", d_out, GL._assemble(R, GL._canary(R.size_out, S), at, "pt", shift=S), S)
    MG.tags_same(R, b"".join(tags), name + " dec out of place")
    unchanged("dec out of place", d_ct, ct_arena)

    def forged_leg(leg, wipe, d_in, d_dst, shift, want):
        """one tag in seven forged: those calls raise, the others do not; with the wipe exactly `len` zeros in the forged messages' places"""
        ctx.set_option("wipe_on_auth_fail", int(wipe))
        for i in range(n):
            try:
                ctx.decrypt_dev(iv(i), d_in.ptr + at[i], R.lens[i], d_dst.ptr + shift + at[i], tag=tag(R.bad_tags, i), **aad(i))
                raised = False
            except hip.AuthenticationError:
                raised = True
            assert raised == (i in forged), (name, leg, "AuthenticationError", raised, R.grid.cell(i))
        ctx.set_option("wipe_on_auth_fail", 0)
        compare(leg, d_dst, want, shift)

    d_out = _up(hip, GL._canary(R.size_out, S))
    forged_leg("dec out of place, forged, unwiped", False, d_ct, d_out, S, GL._assemble(R, GL._canary(R.size_out, S), at, "pt", shift=S))
    d_out = _up(hip, GL._canary(R.size_out, S))
    forged_leg("dec out of place, forged, wiped", True, d_ct, d_out, S, GL._assemble(R, GL._canary(R.size_out, S), at, "pt", shift=S, wiped=True))
    unchanged("dec out of place, forged, wiped", d_ct, ct_arena)
    d_io = _up(hip, ct_arena)
    forged_leg("dec in place, forged, wiped", True, d_io, d_io, 0, GL._assemble(R, R.pt_arena, at, "pt", wiped=True))
    GL._same(R, d_aad, R.aad_arena, R.aad_at, 0, name + " dec in place (AAD arena)")
    ctx.close()


@pytest.mark.parametrize("klen", MG.KEY_SIZES)
@pytest.mark.parametrize("name", [s.name for s in MG.SHAPES])
def test_whole_messages_in_every_launch_shape(hip, orc, u, name, klen):
    """every message of the shape's grid: encrypt out of place and in place, decrypt with the true tags, and with one tag in seven forged unwiped, wiped out of
    place and wiped in place -- six arenas compared whole, the input and AAD arenas shown unchanged, every call's shape asserted"""
    _legs(hip, orc, u, name, klen)


# ---------------------------------------------------------------------------------------------- shards
@pytest.mark.parametrize("how", sorted(MG.SHARD_OPTS))
def test_a_shard_writes_its_own_range_only(hip, orc, u, how):
    """40 KiB + 9 bytes with a 33-byte AAD over 3 and 5 ranks whose first blocks are no multiples of 256, under the forced dealt and the forced cyclic options, the
    ranks in falling and in rising order: the whole output arena after EVERY rank -- that rank's range alone may have changed --, the input unchanged, then the tag"""
    n, al = MG.SHARD_LEN, MG.SHARD_AAD
    sl = MG.Slots([n], ["the message"])
    lo = sl.in_at[0]
    for klen in MG.KEY_SIZES:
        key, iv = splitmix_bytes(0x5A4D00 + klen, klen), splitmix_bytes(0x5A4D01, 12)
        aad, pt = splitmix_bytes(0x5A4D02, al), splitmix_bytes(0x5A4D03 + klen, n)
        ct, want_tag = orc.Fast(key).encrypt(iv, aad, pt)
        ctx = _context(hip, key, MG.SHARD_OPTS[how])
        aad_arena = MG.Slots([al]).arena(PG.CANARY_IN, {0: aad})
        d_aad = _up(hip, aad_arena)
        for ranks in (3, 5):
            rng = MG.shard_ranges(ranks, u)
            for dec in (False, True):
                src, dst = (ct, pt) if dec else (pt, ct)
                in_arena = sl.arena(PG.CANARY_IN, {0: src})
                for order in (range(ranks - 1, -1, -1), range(ranks)):
                    label = "shards %s AES-%d %d ranks %s %s" % (how, 8 * klen, ranks, "dec" if dec else "enc", "falling" if order[0] else "rising")
                    d_in, d_out, parts = _up(hip, in_arena), _up(hip, sl.arena(PG.CANARY_OUT)), Guarded(hip, 16 * ranks)
                    want = sl.arena(PG.CANARY_OUT)
                    for r in order:
                        first, ln = rng[r]
                        sh, sb = ctx.split(ln, first)
                        assert sb > 0 and sh == (-first) % u["A"], (label, r, sh, sb)
                        ctx.shard_crypt_dev(dec, iv, d_in.ptr + lo + 16 * first, ln, d_out.ptr + lo + 16 * first, first, n, parts.ptr + 16 * r,
                                            d_aad=d_aad.ptr + PG.GUARD if r == 0 else None, aad_len=al if r == 0 else 0)
                        want[lo + 16 * first:lo + 16 * first + ln] = np.frombuffer(dst[16 * first:16 * first + ln], dtype=np.uint8)
                        MG.same(sl, _down(hip, d_out), want, sl.in_at, 0, "%s after rank %d (blocks %d .. %d)" % (label, r, first, first + (ln + 15) // 16))
                        _ARENAS.append((label, r))
                    parts.read(label)
                    assert ctx.shard_finalize_dev(iv, parts.ptr, ranks, al, n) == want_tag, label
                    MG.same(sl, _down(hip, d_in), in_arena, sl.in_at, 0, label + " (input arena)")
        assert _down(hip, d_aad) == aad_arena.tobytes(), "the AAD arena changed"
        ctx.close()


# ---------------------------------------------------------------------------------------------- streaming chunks
@pytest.mark.parametrize("how", sorted(MG.STREAM_OPTS))
def test_a_streaming_chunk_writes_its_own_slot_only(hip, orc, u, how):
    """sessions of 1, 2 and 4 chunks on and beside a row and the body's alignment with a ragged last chunk, every chunk's output in a guarded slot of its own: the
    whole arena after EVERY chunk, the input unchanged, stream_final against the oracle; encrypt and decrypt, by k_main and under the forced dealt and cyclic options"""
    for klen in MG.KEY_SIZES:
        key, iv, aad = splitmix_bytes(0x57E400 + klen, klen), splitmix_bytes(0x57E401, 12), splitmix_bytes(0x57E402, MG.STREAM_AAD)
        f = orc.Fast(key)
        for sizes in MG.stream_sessions(u):
            sl = MG.Slots(list(sizes), ["chunk %d of %r" % (k, sizes) for k in range(len(sizes))])
            pt = splitmix_bytes(0x57E403 + len(sizes), sum(sizes))
            ct, want_tag = f.encrypt(iv, aad, pt)
            cuts = [sum(sizes[:k]) for k in range(len(sizes) + 1)]
            for dec in (False, True):
                src, dst = (ct, pt) if dec else (pt, ct)
                label = "session %s AES-%d %r %s" % (how, 8 * klen, sizes, "dec" if dec else "enc")
                in_arena = sl.arena(PG.CANARY_IN, {k: src[cuts[k]:cuts[k + 1]] for k in range(len(sizes))})
                d_in, d_out, want = _up(hip, in_arena), _up(hip, sl.arena(PG.CANARY_OUT)), sl.arena(PG.CANARY_OUT)
                ctx = _context(hip, key, MG.STREAM_OPTS[how])
                ctx.stream_begin(iv, decrypt=dec)
                ctx.stream_aad(aad)
                for k, sz in enumerate(sizes):
                    ctx.stream_update_dev(d_in.ptr + sl.in_at[k], sz, d_out.ptr + sl.in_at[k])
                    want[sl.in_at[k]:sl.in_at[k] + sz] = np.frombuffer(dst[cuts[k]:cuts[k + 1]], dtype=np.uint8)
                    MG.same(sl, _down(hip, d_out), want, sl.in_at, 0, "%s after chunk %d" % (label, k))
                    _ARENAS.append((label, k))
                assert ctx.stream_final() == want_tag, label
                MG.same(sl, _down(hip, d_in), in_arena, sl.in_at, 0, label + " (input arena)")
                ctx.close()


# ---------------------------------------------------------------------------------------------- keystream
@pytest.mark.parametrize("klen", MG.KEY_SIZES)
def test_keystream_runs_between_guards(hip, orc, klen):
    """nblocks 1 2 63 64 65 255 256 257 from blocks 0, 1, 255 and 2^32 - 3, each run between guards, against the oracle's keystream; a run that would wrap the
    counter is refused and writes nothing"""
    key, iv = splitmix_bytes(0x4B5300 + klen, klen), splitmix_bytes(0x4B5301, 12)
    f, ctx = orc.Fast(key), hip.Context(key)
    runs = [(first, nb) for first in MG.KS_FIRST for nb in MG.KS_NBLOCKS]
    sl = MG.Slots([16 * nb for _f, nb in runs], ["%d blocks from %d" % (nb, first) for first, nb in runs])
    d_out, parts = _up(hip, sl.arena(PG.CANARY_OUT)), {}
    for k, (first, nb) in enumerate(runs):
        if MG.ks_fits(first, nb):
            ctx.keystream_dev(iv, first, nb, d_out.ptr + sl.in_at[k])
            parts[k] = f.keystream(iv, first, nb)
        else:
            with pytest.raises(hip.AesGcmError):
                ctx.keystream_dev(iv, first, nb, d_out.ptr + sl.in_at[k])
    assert len(parts) == 3 * len(MG.KS_NBLOCKS) + 1                      # from 2^32 - 3 one block alone fits
    MG.same(sl, _down(hip, d_out), sl.arena(PG.CANARY_OUT, parts), sl.in_at, 0, "keystream AES-%d" % (8 * klen))
    _ARENAS.append(("keystream", klen))


# ---------------------------------------------------------------------------------------------- the comparison itself
def test_perturbed_references_are_reported(hip, orc, u):
    """the arena comparison raises and names the message and its cell when the expected arena is wrong in one byte inside a message, in the first guard byte
    behind it or in the last guard byte in front of it, and when one bit of a tag is; no further GPU run: the arena is the one a leg downloaded"""
    name = "cyc_close1 AES-128"
    if name not in _KEPT:
        _legs(hip, orc, u, "cyc_close1", 16)
    R, got, want, at, shift = _KEPT[name]
    MG.same(R, got, want, at, shift, "as it was")
    for i in (1, R.n // 2, R.n - 2):
        for what, arena, tags, words in MG.perturbations(R, want, at, shift, i):
            with pytest.raises(AssertionError) as e:
                if arena is not None:
                    MG.same(R, got, arena, at, shift, what)
                else:
                    MG.tags_same(R, R.tags, what, tags=tags)
            assert all(w in str(e.value) for w in words), (what, words, str(e.value))


def test_every_arena_was_compared():
    """(runs last) the (shape, key size, leg) arenas compared in this run, for the record: six per shape and key size when the whole file ran"""
    whole = [a for a in _ARENAS if isinstance(a[1], str)]
    print("arenas compared: %d of whole messages, %d in all" % (len(whole), len(_ARENAS)))
    assert len(whole) % 6 == 0
