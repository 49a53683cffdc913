"""What the key-table tests share: for the GPU tests of the family (tests/test_gpu_keytab.py, _wire, _wirex, _tls, _quic, _dtls, _srtp) the upload and packing helpers, the layout of
packets between guard bytes, the libcrypto handle and each family's expected frames from libcrypto (wire_ref_encrypt, x_ref_encrypt, tls_ref_encrypt: nonce and AAD
by the standards' formulas in plain Python), and for tests/test_gpu_kt_grid.py and tests/test_kt_grid_cpu.py the reference of a grid of tests/kt_grid.py
(grid_reference); for their CPU counterparts (tests/test_keytab_cpu.py, ...) the census of a family's gfx950 listing and what every
kernel of the family owes it.  Helpers that differ per family (_run, _ref_encrypt, _table, _make_*) stay in the family's file."""
import ctypes
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import dtls_fixture as D
import kt_grid as KG
import pkt_grid as PG
import quic_fixture as Q
import srtp_fixture as S
import tls_fixture as T
from util import splitmix_bytes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "aes-gcm-128-192-256-bits_amd", "csrc")

CANARY = 0xC5
TRAIL = 37


def _up(hip, data):
    b = hip.DeviceBuffer(max(len(data), 16))
    if data:
        b.upload(data)
    return b


def _u32(v):
    return struct.pack("<%dI" % len(v), *v)


def _u64(v):
    return struct.pack("<%dQ" % len(v), *v)


@pytest.fixture(scope="module")
def evp():
    from oracle import cpu_baseline
    return cpu_baseline.evp_batch_lib()


def _layout(pkts, lead, trail=TRAIL):
    off = [lead]
    for r in pkts:
        off.append(off[-1] + len(r))
    return off, bytes([CANARY]) * lead + b"".join(pkts) + bytes([CANARY]) * trail


def _collect(hip, d):
    """what a wire-format _run left in d: -> (the whole output buffer, auth or None, d)"""
    hip.dev_sync()
    out = bytes(d["out"].download(d["nbytes"]))
    auth = list(struct.unpack("<%di" % d["n"], bytes(d["auth"].download(4 * d["n"])))) if d["auth"] is not None else None
    return out, auth, d


def asm_census(family):
    """`make -C csrc asm_<family>`, then tools/isa_census.py over the listing -> {kernel: ...}; skips where there is no hipcc"""
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    subprocess.run(["make", "-C", CSRC, "-s", "asm_" + family], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_census
    return isa_census.census(os.path.join(CSRC, "aesgcm_%s.gfx950.s" % family))


def assert_in_budget(census, body="k_"):
    """every kernel: no scratch, at most the 128 registers of a 1024-lane workgroup; those that run the block loop (names starting with `body`): no scratch
    instruction at the loop depth where the AES rounds read their tables"""
    for name, k in census.items():
        assert k["scratch"] == 0, (name, k["scratch"])
        assert k["vgpr"] <= 128, (name, k["vgpr"])
        if name.startswith(body):
            depths = [d for d, ops in k["depth"].items() if ops.get("ds_read", 0) >= 16]
            assert depths, name
            assert all(k["depth"][d].get("scratch", 0) == 0 for d in depths), (name, k["depth"])


# ---------------------------------------------------------------------------------------------- expected frames from libcrypto
def evp_by_slot(evp, key_len, keys, slots, parts, frames, tag_len):
    """the expected wire frames from libcrypto: parts[p] = (nonce, aad, payload) of frame p; per slot one evp_frames_crypt call over that slot's frames; a frame's
    bytes in front of its payload pass through, the tag's first tag_len bytes follow the ciphertext"""
    by = {}
    for p, s in enumerate(slots):
        by.setdefault(s, []).append(p)
    out = [None] * len(frames)
    for s, ps in by.items():
        ivs, aads, datas = [parts[p][0] for p in ps], [parts[p][1] for p in ps], [parts[p][2] for p in ps]
        assert all(len(v) == 12 for v in ivs)
        aoff, doff = [0], [0]
        for a, d in zip(aads, datas):
            aoff.append(aoff[-1] + len(a)); doff.append(doff[-1] + len(d))
        aad, data = b"".join(aads), b"".join(datas)
        ct = ctypes.create_string_buffer(max(len(data), 1))
        tags = ctypes.create_string_buffer(16 * len(ps))
        rc = evp.evp_frames_crypt(len(ps), key_len, keys[key_len * s:key_len * (s + 1)], b"".join(ivs), aad or b"\0", _u64(aoff), 0, data or b"\0", _u64(doff), 0,
                                  ctypes.addressof(ct), ctypes.addressof(tags))
        assert rc == 0
        ctb, tgb = ct.raw, tags.raw
        for i, p in enumerate(ps):
            f = frames[p]
            front = len(f) - tag_len - (doff[i + 1] - doff[i])
            out[p] = f[:front] + ctb[doff[i]:doff[i + 1]] + tgb[16 * i:16 * i + tag_len]
    return out


def wire_fields(fmt):
    return fmt.aad_len, fmt.hdr_len, fmt.iv_off, fmt.salt_len, fmt.tag_len, bool(fmt.flags & 1)


def wire_split(fmt, salt, f):
    """one wire frame -> (nonce, aad, payload) as the format defines them"""
    aad_len, hdr_len, iv_off, salt_len, tag_len, auth_only = wire_fields(fmt)
    body = len(f) - tag_len
    nonce = salt[:salt_len] + f[iv_off:iv_off + 12 - salt_len]
    return nonce, (f[:body] if auth_only else f[:aad_len]), (b"" if auth_only else f[hdr_len:body])


def wire_ref_encrypt(evp, key_len, keys, salts, fmt, slots, frames):
    return evp_by_slot(evp, key_len, keys, slots, [wire_split(fmt, salts[s], f) for s, f in zip(slots, frames)], frames, fmt.tag_len)


def _xor(a, b):
    return bytes(x ^ y for x, y in zip(a, b))


class Sa:
    """what the slots hold besides their keys: the classic 8-byte salt, the 12-byte XPN salt and the SSCI"""

    def __init__(self, n_slots, seed):
        sb, xb, cb = splitmix_bytes(seed, 8 * n_slots), splitmix_bytes(seed + 1, 12 * n_slots), splitmix_bytes(seed + 2, 4 * n_slots)
        self.salt = [sb[8 * s:8 * s + 8] for s in range(n_slots)]
        self.xsalt = [xb[12 * s:12 * s + 12] for s in range(n_slots)]
        self.ssci = [cb[4 * s:4 * s + 4] for s in range(n_slots)]


def x_split(xf, sa, slot, hi, f):
    """one wire frame with a 64-bit number -> (nonce, aad, payload) by the standards' formulas"""
    b = xf.f
    body = len(f) - b.tag_len
    auth_only = bool(b.flags & 1)
    if xf.ext == 1:          # 802.1AEbw: salt XOR (SSCI | PN), the PN big-endian = hi, then the SecTAG's PN field
        nonce = _xor(sa.xsalt[slot], sa.ssci[slot] + struct.pack(">I", hi) + f[b.iv_off:b.iv_off + 4])
        aad = f[:body] if auth_only else f[:b.aad_len]
    elif xf.ext == 2:        # RFC 4106: salt | IV field; RFC 4303: SPI | seq-hi | seq-lo
        nonce = sa.salt[slot][:4] + f[b.iv_off:b.iv_off + 8]
        aad = f[0:4] + struct.pack(">I", hi) + f[4:8]
    else:
        nonce = sa.salt[slot][:b.salt_len] + f[b.iv_off:b.iv_off + 12 - b.salt_len]
        aad = f[:body] if auth_only else f[:b.aad_len]
    return nonce, aad, (b"" if auth_only else f[b.hdr_len:body])


def x_ref_encrypt(evp, key_len, keys, sa, xf, slots, his, frames):
    return evp_by_slot(evp, key_len, keys, slots, [x_split(xf, sa, s, h, f) for s, h, f in zip(slots, his, frames)], frames, xf.f.tag_len)


def tls_ref_encrypt(evp, key_len, keys, ivs, ver, slots, seqs, recs):
    h = T.HDR[ver]
    return evp_by_slot(evp, key_len, keys, slots, [(T.nonce_of(ver, ivs[s], q, r), T.aad_of(ver, q, r), r[h:-16]) for s, q, r in zip(slots, seqs, recs)], recs, 16)


# ---------------------------------------------------------------------------------------------- the grid of tests/kt_grid.py: device helpers and the reference
def up_arena(hip, data):
    b = data.tobytes() if isinstance(data, np.ndarray) else bytes(data)
    d = hip.DeviceBuffer(max(len(b), 16))
    assert d.ptr % 128 == 0, "device allocations are expected on a cache line: the grid's residues are offsets"
    d.upload(b)
    d.size = len(b)
    return d


class Guarded:
    """a small device array (tags, verdicts, packet numbers) between two guards"""

    def __init__(self, hip, n):
        self.n, self.buf = n, up_arena(hip, bytes([0xA7]) * (n + 2 * PG.GUARD))
        self.ptr = self.buf.ptr + PG.GUARD

    def read(self, label):
        b = bytes(self.buf.download())
        assert b[:PG.GUARD] == bytes([0xA7]) * PG.GUARD and b[PG.GUARD + self.n:] == bytes([0xA7]) * PG.GUARD, ("guard bytes around tags / verdicts overwritten", label)
        return b[PG.GUARD:PG.GUARD + self.n]


def grid_format(lib, mode):
    """the library's format of a grid mode (None for QUIC, which has none)"""
    W, X, F, DF, SF = lib.WireFormat, lib.WireFormatX, lib.TlsFormat, lib.DtlsFormat, lib.SrtpFormat
    return {"macsec": W.macsec, "esp16": lambda: W.esp(16), "esp12": lambda: W.esp(12), "esp8": lambda: W.esp(8), "macsec_auth": lambda: W.macsec(sci=False, auth_only=True),
            "xpn": X.macsec_xpn, "esn16": lambda: X.esp_esn(16), "tls13": F.tls13, "tls12": F.tls12, "quic": lambda: None, "dtls13": DF.dtls13, "dtls12": DF.dtls12,
            "srtp": lambda: SF.rtp(0), "srtp_mki": lambda: SF.rtp(4), "srtcp": lambda: SF.rtcp(0), "srtcp_clear": lambda: SF.rtcp(3)}[mode]()


class GridRef:
    """what a grid of tests/kt_grid.py must become under one key size, from the family's own fixture (libcrypto through evp_by_slot with nonce and AAD by the
    family's formulas; QUIC: tests/quic_fixture.py; DTLS: tests/dtls_fixture.py; SRTP and SRTCP: tests/srtp_fixture.py) -- never from a GPU path:
      keys, salts / sa / ivs   what the table's slots hold (DTLS and SRTP: ivs, the 12-byte IV or session salt that set_tls_iv takes)
      enc         the arena with the reference's frames in place of the plaintext ones
      dec_in      ... with the ICVs of g.forged forged (one bit inside the first tag_len bytes of the ICV, which SRTP and SRTCP have in front of their trailer)
      dec_out     what decrypting dec_in in place leaves: front and plaintext, the ICV's bytes as they came, the trailer (QUIC and DTLS 1.3: a forged packet's
                  bytes are what the fixture's unprotect makes of it -- a forged tag that lies in the sample changes the header's mask)
      auth, pn_out  the verdicts, and for QUIC and DTLS 1.3 the decoded numbers"""


_REFS = {}


def grid_reference(lib, evp, mode, key_len):
    if (mode, key_len) in _REFS:
        return _REFS[mode, key_len]
    g = KG.grid(mode)
    R = GridRef()
    R.g, R.key_len, R.fmt = g, key_len, grid_format(lib, mode)
    n_slots = KG.N_AEAD + (KG.N_HP if g.hps is not None else 0)
    seed = 0x6B7E0000 + 256 * KG.SEED_ORDER.index(mode) + key_len
    R.keys = splitmix_bytes(seed, key_len * n_slots)
    frames = g.frames()
    f = R.fmt.f if g.family == "wirex" else R.fmt
    if g.family in ("wire", "wirex"):
        assert (f.hdr_len, f.tag_len, bool(f.flags & 1)) == (g.fronts[0], g.tag_len, g.auth_only), mode
    if g.family == "wire":
        sb = splitmix_bytes(seed + 1, 8 * n_slots)
        R.salts = [sb[8 * s:8 * s + 8] for s in range(n_slots)]
        enc = wire_ref_encrypt(evp, key_len, R.keys, R.salts, R.fmt, g.slots, frames)
    elif g.family == "wirex":
        R.sa = Sa(n_slots, seed + 1)
        enc = x_ref_encrypt(evp, key_len, R.keys, R.sa, R.fmt, g.slots, g.nums, frames)
    elif g.family == "tls":
        ib = splitmix_bytes(seed + 1, 12 * n_slots)
        R.ivs = [ib[12 * s:12 * s + 12] for s in range(n_slots)]
        assert T.HDR[R.fmt.version] == g.fronts[0]
        enc = tls_ref_encrypt(evp, key_len, R.keys, R.ivs, R.fmt.version, g.slots, g.nums, frames)
    else:
        ib = splitmix_bytes(seed + 1, 12 * KG.N_AEAD)
        R.ivs = [ib[12 * s:12 * s + 12] for s in range(KG.N_AEAD)]
        R.key = lambda s: R.keys[key_len * s:key_len * (s + 1)]
        R.mki_len = 0
        if g.family == "quic":
            enc = [Q.protect(R.key(g.slots[i]), R.ivs[g.slots[i]], R.key(g.hps[i]), g.nums[i], g.pn_off[i], frames[i]) for i in range(g.n)]
        elif mode == "dtls13":
            enc = [D.protect13(R.key(g.slots[i]), R.ivs[g.slots[i]], R.key(g.hps[i]), g.nums[i], g.sn_off[i], frames[i]) for i in range(g.n)]
        elif mode == "dtls12":
            enc = [D.protect12(R.key(g.slots[i]), R.ivs[g.slots[i]], frames[i]) for i in range(g.n)]
        else:
            R.kind, R.mki_len = (S.RTCP, g.trail[0] - 4) if g.rtcp else (S.RTP, g.trail[0])
            assert (R.fmt.kind, R.fmt.mki_len) == (R.kind, R.mki_len), mode
            enc = [S.protect(R.kind, R.key(g.slots[i]), R.ivs[g.slots[i]], 0 if g.rtcp else g.nums[i], frames[i], R.mki_len) for i in range(g.n)]
    assert [len(e) for e in enc] == g.flen
    tl = g.tag_len
    bad = list(enc)
    for i in g.forged:
        b = bytearray(enc[i])
        b[g.tag_at(i) + i % tl] ^= 1 << (i % 8)
        bad[i] = bytes(b)
    dec = [p[:g.tag_at(i)] + e[g.tag_at(i):] for i, (p, e) in enumerate(zip(frames, bad))]
    R.auth = [0 if i in set(g.forged) else 1 for i in range(g.n)]
    if g.family == "quic":
        R.pn_out = list(g.nums)
        for i in g.forged:
            dec[i], R.pn_out[i], ok = Q.unprotect(R.key(g.slots[i]), R.ivs[g.slots[i]], R.key(g.hps[i]), g.expected_pns[i], g.pn_off[i], bad[i])
            assert not ok
    if mode == "dtls13":
        R.pn_out = list(g.nums)
        for i in g.forged:
            dec[i], R.pn_out[i], ok = D.unprotect13(R.key(g.slots[i]), R.ivs[g.slots[i]], R.key(g.hps[i]), g.expected_seqs[i], g.sn_off[i], bad[i])
            assert not ok
    lo, hi = PG.GUARD, int(g.off[-1])

    def arena(fr):
        a = np.array(g.arena)
        a[lo:hi] = np.frombuffer(b"".join(fr), dtype=np.uint8)
        a.setflags(write=False)
        return a
    R.enc, R.dec_in, R.dec_out = arena(enc), arena(bad), arena(dec)
    _REFS[mode, key_len] = R
    return R


def grid_table(lib, R):
    """a key table of the library in force holding what the reference's slots hold"""
    g = R.g
    kt = lib.KeyTable(R.key_len, len(R.keys) // R.key_len)
    kt.set(0, R.keys)
    if g.family == "wire":
        kt.set_salt(0, b"".join(R.salts))
    elif g.family == "wirex":
        kt.set_salt(0, b"".join(R.sa.salt))
        kt.set_xpn(0, b"".join(R.sa.xsalt), b"".join(R.sa.ssci))
    else:
        kt.set_tls_iv(0, b"".join(R.ivs))
    return kt
