"""ctypes binding of libaesgcm_hip.so -- one Python function per entry point of include/aesgcm.h.

Mirrors the C ABI one to one (same names without the aesgcm_ prefix, same argument meaning, error
codes turned into exceptions).  No torch, no numpy requirement (numpy arrays are accepted as
buffers).  Loading fails loudly when the library is missing; compute calls fail loudly
(AesGcmError: AESGCM_EHIP) when no HIP device is usable -- there is no CPU path to fall back to.
"""
import ctypes
import os
import struct

from .build import SO, SO_DEBUG, build

OK, EARG, EKEYLEN, EIVLEN, ETOOLONG, EAUTH, EHIP, ENOMEM, ESTATE, EALIGN, ERCCL = 0, -1, -2, -3, -4, -5, -6, -7, -8, -9, -10

LAUNCH_NONE, LAUNCH_MAIN, LAUNCH_CYCLIC, LAUNCH_CYCLIC_HALF, LAUNCH_DEALT = range(5)      # aesgcm_ctx_last_launch
SHAPE_ROWS = 1 << 20    # AESGCM_SHAPE_ROWS: what packets_shape says for calls that go by rows
SHAPE_MIXED = 1 << 21   # AESGCM_SHAPE_MIXED: ... for calls with offset arrays: every message is routed by its own size on the device
STATUS_OK, STATUS_PLAN, STATUS_LENGTH, STATUS_UNITS = range(4)      # aesgcm_ctx_status
ABI_VERSION = 5         # AESGCM_ABI_VERSION of include/aesgcm.h this binding was written against

# every symbol include/aesgcm.h declares (tests check the .so exports exactly these)
SYMBOLS = [
    "aesgcm_abi_version", "aesgcm_strerror", "aesgcm_last_error", "aesgcm_device_count", "aesgcm_device_name",
    "aesgcm_key_expand", "aesgcm_ecb_encrypt", "aesgcm_gfmul", "aesgcm_ghash", "aesgcm_get_h",
    "aesgcm_ctx_create", "aesgcm_ctx_create_preexpanded", "aesgcm_ctx_rekey", "aesgcm_ctx_destroy", "aesgcm_ctx_device", "aesgcm_ctx_set_option", "aesgcm_ctx_stream", "aesgcm_ctx_wait", "aesgcm_ctx_wait_fused",
    "aesgcm_encrypt_pipelined", "aesgcm_decrypt_pipelined", "aesgcm_host_alloc", "aesgcm_host_free",
    "aesgcm_encrypt", "aesgcm_decrypt", "aesgcm_encrypt_dev", "aesgcm_decrypt_dev", "aesgcm_last_tag",
    "aesgcm_keystream", "aesgcm_keystream_dev",
    "aesgcm_shard_crypt_dev", "aesgcm_shard_finalize_dev", "aesgcm_shard_finalize_strided_dev", "aesgcm_shard_finalize_batch_dev", "aesgcm_batch_crypt_dev", "aesgcm_batch_crypt_var_dev", "aesgcm_packets_crypt_dev", "aesgcm_messages_crypt_dev", "aesgcm_batch_shape", "aesgcm_packets_shape",
    "aesgcm_stream_begin", "aesgcm_stream_aad", "aesgcm_stream_update", "aesgcm_stream_final",
    "aesgcm_dev_alloc", "aesgcm_dev_free", "aesgcm_dev_upload", "aesgcm_dev_download", "aesgcm_dev_sync", "aesgcm_dev_copy",
    "aesgcm_fill_splitmix64_dev",
    "aesgcm_ctx_timing_enable", "aesgcm_ctx_timing_read", "aesgcm_ctx_geometry", "aesgcm_ctx_body_geometry", "aesgcm_ctx_split", "aesgcm_ctx_wg_trace",
    "aesgcm_ctx_ceiling_probe",
    "aesgcm_timer_create", "aesgcm_timer_start", "aesgcm_timer_stop", "aesgcm_timer_ms", "aesgcm_timer_destroy",
    "aesgcm_comm_last_error", "aesgcm_comm_unique_id", "aesgcm_comm_create", "aesgcm_comm_ranks", "aesgcm_comm_allgather_dev",
    "aesgcm_comm_allreduce_f64", "aesgcm_comm_barrier", "aesgcm_comm_destroy",
    "aesgcm_mgpu_create", "aesgcm_mgpu_ranks", "aesgcm_mgpu_ctx", "aesgcm_mgpu_crypt_dev", "aesgcm_mgpu_destroy",
    "aesgcm_ctx_last_launch", "aesgcm_wipe_failed_dev", "aesgcm_mgpu_last_tags", "aesgcm_mgpu_sync", "aesgcm_batch_ceiling_probe_dev",
    "aesgcm_ctx_status", "aesgcm_stream_update_dev", "aesgcm_stream_export", "aesgcm_stream_import", "aesgcm_frames_ceiling_probe_dev", "aesgcm_ctx_last_route",
    "aesgcm_keytab_create", "aesgcm_keytab_set", "aesgcm_keytab_set_dev", "aesgcm_keytab_clear", "aesgcm_keytab_crypt_dev", "aesgcm_keytab_status", "aesgcm_keytab_destroy",
    "aesgcm_wire_fmt_check", "aesgcm_keytab_set_salt", "aesgcm_keytab_frames_crypt_dev",
    "aesgcm_wire_xfmt_check", "aesgcm_keytab_set_xpn", "aesgcm_keytab_frames_crypt_x_dev",
    "aesgcm_tls_fmt_check", "aesgcm_keytab_set_tls_iv", "aesgcm_keytab_records_crypt_dev",
    "aesgcm_keytab_quic_crypt_dev",
    "aesgcm_dtls_fmt_check", "aesgcm_keytab_dtls_crypt_dev",
    "aesgcm_srtp_fmt_check", "aesgcm_keytab_srtp_crypt_dev",
    "aesgcm_rxwin_create", "aesgcm_rxwin_set", "aesgcm_rxwin_get", "aesgcm_rxwin_fmt_check", "aesgcm_rxwin_recover_dev", "aesgcm_rxwin_commit_dev", "aesgcm_rxwin_status",
    "aesgcm_rxwin_destroy",
    "aesgcm_txnum_create", "aesgcm_txnum_set", "aesgcm_txnum_get", "aesgcm_txnum_fmt_check", "aesgcm_txnum_assign_dev", "aesgcm_txnum_status", "aesgcm_txnum_destroy",
    "aesgcm_kdf_create", "aesgcm_kdf_set", "aesgcm_kdf_set_dev", "aesgcm_kdf_clear", "aesgcm_kdf_fmt_check", "aesgcm_kdf_install_dev", "aesgcm_kdf_update_dev", "aesgcm_kdf_status",
    "aesgcm_kdf_destroy",
    "aesgcm_srtp_kdf_create", "aesgcm_srtp_kdf_set", "aesgcm_srtp_kdf_set_dev", "aesgcm_srtp_kdf_clear", "aesgcm_srtp_kdf_install_dev", "aesgcm_srtp_kdf_status",
    "aesgcm_srtp_kdf_destroy",
    "aesgcm_prf12_create", "aesgcm_prf12_set", "aesgcm_prf12_set_dev", "aesgcm_prf12_clear", "aesgcm_prf12_install_dev", "aesgcm_prf12_export_srtp_dev", "aesgcm_prf12_status",
    "aesgcm_prf12_destroy",
    "aesgcm_prfplus_create", "aesgcm_prfplus_set", "aesgcm_prfplus_set_dev", "aesgcm_prfplus_clear", "aesgcm_prfplus_install_dev", "aesgcm_prfplus_status", "aesgcm_prfplus_destroy",
    "aesgcm_mka_create", "aesgcm_mka_set", "aesgcm_mka_set_dev", "aesgcm_mka_clear", "aesgcm_mka_install_dev", "aesgcm_mka_unwrap_dev", "aesgcm_mka_status", "aesgcm_mka_destroy",
    "aesgcm_keytab_ssh_crypt_dev",
    "aesgcm_sshkdf_create", "aesgcm_sshkdf_set", "aesgcm_sshkdf_set_dev", "aesgcm_sshkdf_clear", "aesgcm_sshkdf_install_dev", "aesgcm_sshkdf_status", "aesgcm_sshkdf_destroy",
]


class AesGcmError(RuntimeError):
    def __init__(self, code, detail=""):
        self.code = code
        msg = _strerror(code)
        if detail:
            msg += ": " + detail
        super().__init__("aesgcm error %d: %s" % (code, msg))


class AuthenticationError(AesGcmError, ValueError):
    """Tag mismatch on decrypt (the ValueError pycryptodome's verify() raises, tb/gcm_model.py:47)."""


_L = None
vp, sz, u64, cint = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint64, ctypes.c_int
cp = ctypes.c_char_p


def load():
    """Load (building first if sources are newer) and type the library."""
    global _L
    if _L is not None:
        return _L
    build()                       # no-op when the .so is newer than csrc/ and include/aesgcm.h; tolerates a missing hipcc if a prebuilt .so exists
    _L = _typed(ctypes.CDLL(SO))
    return _L


_DBG = None


class debug_library:
    """`with lib.debug_library() as dbg:` -- inside the block every function of this module goes to libaesgcm_hip_dbg.so, the
    -DAESGCM_DEBUG_KNOBS build of the same sources, whose one extra export forces kernel shapes (include/aesgcm_debug.h):
    `dbg.force(pkt_lanes=8)`, `dbg.force(batch_lanes=16)`, ...; leaving the block clears every force and switches back to the
    product library.  Device memory is the process's (either library's allocations serve both); contexts belong to the library
    that made them, so create them inside the block.  Tests and profiling scripts only."""

    def __enter__(self):
        global _L, _DBG
        load()
        if _DBG is None:
            _DBG = _typed(ctypes.CDLL(SO_DEBUG))
            _DBG.aesgcm_debug_force_shape.argtypes = [cp, cint]
        self._prev, _L = _L, _DBG
        return self

    def force(self, **kw):
        for k, v in kw.items():
            _chk(_DBG.aesgcm_debug_force_shape(k.encode(), int(v)))

    def __exit__(self, *a):
        global _L
        for k in ("pkt_lanes", "pkt_deal", "batch_lanes", "batch_deal", "batch_order", "pkt_ilp", "pkt_rows"):
            _DBG.aesgcm_debug_force_shape(k.encode(), 0)
        _L = self._prev


def _typed(L):
    L.aesgcm_strerror.restype = cp
    L.aesgcm_strerror.argtypes = [cint]
    L.aesgcm_last_error.restype = cp
    L.aesgcm_device_count.argtypes = [ctypes.POINTER(cint)]
    L.aesgcm_device_name.argtypes = [cint, cp, sz]
    L.aesgcm_key_expand.argtypes = [cint, vp, sz, vp, ctypes.POINTER(cint)]
    L.aesgcm_ecb_encrypt.argtypes = [vp, vp, sz, vp]
    L.aesgcm_gfmul.argtypes = [cint, vp, vp, vp, sz]
    L.aesgcm_ghash.argtypes = [vp, vp, sz, vp]
    L.aesgcm_get_h.argtypes = [vp, vp]
    L.aesgcm_ctx_create.argtypes = [ctypes.POINTER(vp), cint, vp, sz]
    L.aesgcm_ctx_create_preexpanded.argtypes = [ctypes.POINTER(vp), cint, vp, cint]
    L.aesgcm_ctx_rekey.argtypes = [vp, vp, sz]
    L.aesgcm_ctx_destroy.argtypes = [vp]
    L.aesgcm_ctx_device.argtypes = [vp]
    L.aesgcm_ctx_set_option.argtypes = [vp, cp, ctypes.c_int64]
    L.aesgcm_ctx_stream.argtypes = [vp, ctypes.POINTER(vp)]
    L.aesgcm_ctx_wait.argtypes = [vp, vp]
    L.aesgcm_ctx_wait_fused.argtypes = [vp, vp]
    L.aesgcm_encrypt.argtypes = [vp, vp, vp, sz, vp, sz, vp, vp]
    L.aesgcm_decrypt.argtypes = [vp, vp, vp, sz, vp, sz, vp, vp, vp]
    L.aesgcm_encrypt_pipelined.argtypes = [vp, vp, vp, sz, vp, sz, vp, vp, sz]
    L.aesgcm_decrypt_pipelined.argtypes = [vp, vp, vp, sz, vp, sz, vp, vp, vp, sz]
    L.aesgcm_host_alloc.argtypes = [ctypes.POINTER(vp), sz]
    L.aesgcm_host_free.argtypes = [vp]
    L.aesgcm_encrypt_dev.argtypes = [vp, vp, vp, sz, vp, sz, vp, vp, vp]
    L.aesgcm_decrypt_dev.argtypes = [vp, vp, vp, sz, vp, sz, vp, vp, vp, vp]
    L.aesgcm_last_tag.argtypes = [vp, vp, vp]
    L.aesgcm_keystream.argtypes = [vp, vp, u64, u64, vp]
    L.aesgcm_keystream_dev.argtypes = [vp, vp, u64, u64, vp, vp]
    L.aesgcm_shard_crypt_dev.argtypes = [vp, cint, vp, vp, sz, vp, sz, vp, u64, u64, vp, vp]
    L.aesgcm_shard_finalize_dev.argtypes = [vp, vp, vp, sz, sz, u64, vp, vp]
    L.aesgcm_shard_finalize_strided_dev.argtypes = [vp, vp, vp, sz, sz, sz, u64, vp, vp]
    L.aesgcm_shard_finalize_batch_dev.argtypes = [vp, sz, vp, vp, sz, sz, sz, ctypes.POINTER(sz), ctypes.POINTER(u64), vp, vp]
    L.aesgcm_batch_crypt_dev.argtypes = [cint, cint, sz, sz, vp, vp, vp, sz, vp, sz, vp, vp, vp, vp, vp]
    L.aesgcm_batch_crypt_var_dev.argtypes = [cint, cint, sz, sz, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.aesgcm_packets_crypt_dev.argtypes = [vp, cint, sz, vp, vp, sz, vp, vp, sz, vp, vp, vp, vp, vp, vp]
    L.aesgcm_messages_crypt_dev.argtypes = [vp, cint, sz, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.aesgcm_batch_shape.argtypes = [cint, sz, sz, cint, ctypes.POINTER(cint)]
    L.aesgcm_packets_shape.argtypes = [vp, sz, sz, cint, ctypes.POINTER(cint)]
    L.aesgcm_stream_begin.argtypes = [vp, vp, cint]
    L.aesgcm_stream_aad.argtypes = [vp, vp, sz]
    L.aesgcm_stream_update.argtypes = [vp, vp, sz, vp]
    L.aesgcm_stream_final.argtypes = [vp, vp]
    L.aesgcm_dev_alloc.argtypes = [cint, ctypes.POINTER(vp), sz]
    L.aesgcm_dev_free.argtypes = [cint, vp]
    L.aesgcm_dev_upload.argtypes = [cint, vp, vp, sz]
    L.aesgcm_dev_download.argtypes = [cint, vp, vp, sz]
    L.aesgcm_dev_sync.argtypes = [cint]
    L.aesgcm_dev_copy.argtypes = [cint, vp, vp, sz, vp]
    L.aesgcm_fill_splitmix64_dev.argtypes = [cint, vp, sz, u64, u64, vp]
    L.aesgcm_ctx_timing_enable.argtypes = [vp, cint]
    L.aesgcm_ctx_timing_read.argtypes = [vp, ctypes.POINTER(u64), ctypes.POINTER(ctypes.c_double), cint]
    L.aesgcm_ctx_wg_trace.argtypes = [vp, vp, sz, ctypes.POINTER(sz)]
    L.aesgcm_ctx_geometry.argtypes = [vp, ctypes.POINTER(cint), ctypes.POINTER(cint), ctypes.POINTER(cint)]
    L.aesgcm_ctx_body_geometry.argtypes = [vp, ctypes.POINTER(cint), ctypes.POINTER(cint), ctypes.POINTER(cint)]
    L.aesgcm_ctx_split.argtypes = [vp, sz, u64, ctypes.POINTER(u64), ctypes.POINTER(u64)]
    L.aesgcm_ctx_ceiling_probe.argtypes = [vp, sz, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(u64)]
    L.aesgcm_timer_create.argtypes = [ctypes.POINTER(vp), cint]
    L.aesgcm_timer_start.argtypes = [vp, vp]
    L.aesgcm_timer_stop.argtypes = [vp, vp]
    L.aesgcm_timer_ms.argtypes = [vp, ctypes.POINTER(ctypes.c_double)]
    L.aesgcm_timer_destroy.argtypes = [vp]
    L.aesgcm_comm_last_error.restype = cp
    L.aesgcm_comm_unique_id.argtypes = [vp]
    L.aesgcm_comm_create.argtypes = [ctypes.POINTER(vp), cint, vp, cint, cint]
    L.aesgcm_comm_ranks.argtypes = [vp, ctypes.POINTER(cint), ctypes.POINTER(cint)]
    L.aesgcm_comm_allgather_dev.argtypes = [vp, vp, vp, sz, vp]
    L.aesgcm_comm_allreduce_f64.argtypes = [vp, ctypes.POINTER(ctypes.c_double), cint]
    L.aesgcm_comm_barrier.argtypes = [vp]
    L.aesgcm_comm_destroy.argtypes = [vp]
    L.aesgcm_mgpu_create.argtypes = [ctypes.POINTER(vp), cint, ctypes.POINTER(cint), vp, sz]
    L.aesgcm_mgpu_ranks.argtypes = [vp, ctypes.POINTER(cint)]
    L.aesgcm_mgpu_ctx.argtypes = [vp, cint, ctypes.POINTER(vp)]
    L.aesgcm_mgpu_crypt_dev.argtypes = [vp, cint, vp, vp, sz, ctypes.POINTER(vp), ctypes.POINTER(sz), ctypes.POINTER(vp), vp]
    L.aesgcm_mgpu_destroy.argtypes = [vp]
    L.aesgcm_mgpu_last_tags.argtypes = [vp, sz, vp]
    L.aesgcm_mgpu_sync.argtypes = [vp]
    L.aesgcm_ctx_last_launch.argtypes = [vp, ctypes.POINTER(cint)]
    L.aesgcm_wipe_failed_dev.argtypes = [cint, sz, vp, sz, vp, vp, vp]
    L.aesgcm_batch_ceiling_probe_dev.argtypes = [cint, sz, sz, vp, vp, sz, vp, vp]
    L.aesgcm_ctx_status.argtypes = [vp, ctypes.POINTER(cint), ctypes.POINTER(u64)]
    L.aesgcm_stream_update_dev.argtypes = [vp, vp, sz, vp, vp]
    L.aesgcm_stream_export.argtypes = [vp, vp]
    L.aesgcm_stream_import.argtypes = [vp, vp]
    L.aesgcm_frames_ceiling_probe_dev.argtypes = [vp, sz, vp, vp, vp, vp, vp, vp]
    L.aesgcm_ctx_last_route.argtypes = [vp, ctypes.POINTER(u64)]
    if L.aesgcm_abi_version() != ABI_VERSION:
        raise ImportError("libaesgcm_hip.so ABI %d, expected %d (stale build? rebuild with `make -C csrc`)" % (L.aesgcm_abi_version(), ABI_VERSION))
    return L


def _strerror(code):
    try:
        return load().aesgcm_strerror(code).decode()
    except Exception:
        return "code %d" % code


def _chk(rc):
    if rc == OK:
        return
    detail = load().aesgcm_last_error().decode() if rc == EHIP else ""
    if rc == ERCCL or (rc == EHIP and not detail):
        detail = load().aesgcm_comm_last_error().decode()
    if rc == EAUTH:
        raise AuthenticationError(rc, "MAC check failed")
    raise AesGcmError(rc, detail)


class _Buf:
    """(address, length, keepalive) view of bytes / bytearray / memoryview / numpy array / None."""

    def __init__(self, obj, writable=False):
        self.keep = obj
        if obj is None:
            self.addr, self.n = None, 0
        elif isinstance(obj, bytes):
            if writable:
                raise TypeError("output buffer must be writable")
            self.n = len(obj)
            self.addr = ctypes.cast(ctypes.c_char_p(obj), vp).value if self.n else None
        elif hasattr(obj, "ctypes") and hasattr(obj, "nbytes"):          # numpy
            if writable and not obj.flags.writeable:
                raise TypeError("output buffer must be writable")
            if not obj.flags.c_contiguous:
                raise TypeError("buffer must be C-contiguous")
            self.n = obj.nbytes
            self.addr = obj.ctypes.data if self.n else None
        else:
            mv = memoryview(obj).cast("B")
            self.n = mv.nbytes
            if self.n == 0:
                self.addr = None
            elif mv.readonly:
                if writable:
                    raise TypeError("output buffer must be writable")
                self.keep = bytes(mv)
                self.addr = ctypes.cast(ctypes.c_char_p(self.keep), vp).value
            else:
                self.keep = (ctypes.c_char * self.n).from_buffer(mv)
                self.addr = ctypes.addressof(self.keep)


def _fixed(b, n, what):
    b = bytes(b)
    if len(b) != n:
        raise AesGcmError(EIVLEN if what == "iv" else EARG, "%s must be %d bytes, got %d" % (what, n, len(b)))
    return b


# ---------------------------------------------------------------- module-level (no context)
def device_count():
    n = cint(0)
    _chk(load().aesgcm_device_count(ctypes.byref(n)))
    return n.value


def device_name(device=0):
    b = ctypes.create_string_buffer(256)
    _chk(load().aesgcm_device_name(device, b, 256))
    return b.value.decode()


def key_expand(key, device=0):
    """-> (expanded key bytes (16*(nr+1)), nr).  GPU twin of tb/key_exp.py aes_expand_key."""
    key = bytes(key)
    rk = ctypes.create_string_buffer(240)
    nr = cint(0)
    _chk(load().aesgcm_key_expand(device, key, len(key), rk, ctypes.byref(nr)))
    return rk.raw[:16 * (nr.value + 1)], nr.value


def gfmul(h, x, device=0):
    """Element-wise GF(2^128) products of equal-length sequences of 16-byte blocks."""
    h, x = bytes(h), bytes(x)
    if len(h) != len(x) or len(h) % 16:
        raise AesGcmError(EARG, "h and x must be equal-length multiples of 16 bytes")
    z = ctypes.create_string_buffer(max(len(h), 1))
    _chk(load().aesgcm_gfmul(device, h, x, z, len(h) // 16))
    return z.raw[:len(h)]


class DeviceBuffer:
    """Device memory owned by the library (hipMalloc); upload/download/fill helpers."""

    def __init__(self, nbytes, device=0):
        self.device, self.nbytes = device, nbytes
        p = vp()
        _chk(load().aesgcm_dev_alloc(device, ctypes.byref(p), nbytes))
        self.ptr = p.value

    def upload(self, data, offset=0):
        b = _Buf(data)
        if offset < 0 or offset + b.n > self.nbytes:
            raise AesGcmError(EARG, "upload past end of buffer")
        _chk(load().aesgcm_dev_upload(self.device, self.ptr + offset, b.addr, b.n))

    def download(self, nbytes=None, offset=0, out=None):
        n = self.nbytes - offset if nbytes is None else nbytes
        if offset < 0 or n < 0 or offset + n > self.nbytes:
            raise AesGcmError(EARG, "download past end of buffer")
        if out is None:
            out = bytearray(n)
        b = _Buf(out, writable=True)
        if b.n < n:
            raise AesGcmError(EARG, "output buffer smaller than the %d bytes requested" % n)
        _chk(load().aesgcm_dev_download(self.device, b.addr, self.ptr + offset, n))
        return out

    def fill_splitmix64(self, seed, first_word=0, nbytes=None, offset=0, stream=None):
        n = self.nbytes - offset if nbytes is None else nbytes
        if offset < 0 or n < 0 or offset + n > self.nbytes:
            raise AesGcmError(EARG, "fill past end of buffer")
        _chk(load().aesgcm_fill_splitmix64_dev(self.device, self.ptr + offset, n, seed, first_word, stream))

    def free(self):
        if self.ptr:
            load().aesgcm_dev_free(self.device, self.ptr)
            self.ptr = None

    __del__ = free


def batch_crypt_dev(decrypt, n_pkts, key_len, d_keys, d_ivs, d_in, pkt_len, d_out, d_tags, d_aad=None, aad_len=0,
                    d_expect_tags=None, d_auth=None, device=0, stream=None):
    """n independent packets with per-packet key and IV, all arrays contiguous device memory (aesgcm.h)."""
    _chk(load().aesgcm_batch_crypt_dev(device, int(bool(decrypt)), n_pkts, key_len, d_keys, d_ivs, d_aad, aad_len,
                                       d_in, pkt_len, d_out, d_tags, d_expect_tags, d_auth, stream))


def batch_crypt_var_dev(decrypt, n_pkts, key_len, d_keys, d_ivs, d_in, d_data_off, d_out, d_tags, d_aad=None, d_aad_off=None,
                        d_expect_tags=None, d_auth=None, device=0, stream=None):
    """Variable-length packets: uint64 offset arrays (n_pkts + 1 entries, device memory) delimit data and AAD."""
    _chk(load().aesgcm_batch_crypt_var_dev(device, int(bool(decrypt)), n_pkts, key_len, d_keys, d_ivs, d_aad, d_aad_off,
                                           d_in, d_data_off, d_out, d_tags, d_expect_tags, d_auth, stream))


def wipe_failed_dev(n_pkts, d_out, d_auth, pkt_len=0, d_data_off=None, device=0, stream=None):
    """aesgcm_wipe_failed_dev: zero the output of every packet whose d_auth entry is 0 (what the context option wipe_on_auth_fail does for the packet calls of a context)"""
    _chk(load().aesgcm_wipe_failed_dev(device, n_pkts, d_out, pkt_len, d_data_off, d_auth, stream))


def batch_ceiling_probe_dev(n_pkts, key_len, d_keys, d_ivs, pkt_len, d_tags, device=0, stream=None):
    """aesgcm_batch_ceiling_probe_dev: one launch of the batch kernel without the data's loads and stores (8 lanes per packet only); time it with a Timer"""
    _chk(load().aesgcm_batch_ceiling_probe_dev(device, n_pkts, key_len, d_keys, d_ivs, pkt_len, d_tags, stream))


def batch_shape(n_pkts, pkt_len=0, var_len=False, device=0):
    """lanes per packet the batch entry points take for such a call: 8 / 16 (k_batch3) or 64 (k_batch)"""
    v = cint(0)
    _chk(load().aesgcm_batch_shape(device, n_pkts, pkt_len, int(bool(var_len)), ctypes.byref(v)))
    return v.value


class PinnedBuffer:
    """Page-locked host memory (hipHostMalloc) exposed as a writable memoryview / numpy-compatible buffer."""

    def __init__(self, nbytes):
        p = vp()
        _chk(load().aesgcm_host_alloc(ctypes.byref(p), nbytes))
        self.ptr, self.nbytes = p.value, nbytes
        self._arr = (ctypes.c_ubyte * max(nbytes, 1)).from_address(self.ptr)
        self.view = memoryview(self._arr).cast("B")[:nbytes]

    def free(self):
        if self.ptr:
            self.view = None
            self._arr = None
            load().aesgcm_host_free(self.ptr)
            self.ptr = None

    __del__ = free


def dev_sync(device=0):
    _chk(load().aesgcm_dev_sync(device))


def dev_copy(d_dst, d_src, nbytes, device=0, stream=None):
    """asynchronous device-to-device copy by the library's plain copy kernel"""
    _chk(load().aesgcm_dev_copy(device, d_dst, d_src, nbytes, stream))


class Timer:
    """aesgcm_timer: two HIP events recorded on the stream the timed launches run on."""

    def __init__(self, device=0):
        self._t = None
        t = vp()
        _chk(load().aesgcm_timer_create(ctypes.byref(t), device))
        self._t = t.value

    def start(self, stream=None):
        _chk(load().aesgcm_timer_start(self._t, stream))

    def stop(self, stream=None):
        _chk(load().aesgcm_timer_stop(self._t, stream))

    def ms(self):
        v = ctypes.c_double(0)
        _chk(load().aesgcm_timer_ms(self._t, ctypes.byref(v)))
        return v.value

    def close(self):
        if self._t:
            load().aesgcm_timer_destroy(self._t)
            self._t = None

    __del__ = close


# ---------------------------------------------------------------- context
class Context:
    """aesgcm_ctx: (device, expanded key, H, H-power tables).  One per key."""

    def __init__(self, key=None, device=0, expanded_key=None):
        self._c = None
        L = load()
        c = vp()
        if expanded_key is not None:
            ek = bytes(expanded_key)
            nr = len(ek) // 16 - 1
            if len(ek) % 16 or nr not in (10, 12, 14):
                raise AesGcmError(EKEYLEN, "expanded key must be 176/208/240 bytes")
            _chk(L.aesgcm_ctx_create_preexpanded(ctypes.byref(c), device, ek, nr))
        else:
            key = bytes(key)
            _chk(L.aesgcm_ctx_create(ctypes.byref(c), device, key, len(key)))
        self._c = c.value
        self.device = device
        self._lib = L               # the library that made it destroys it (debug_library switches the module's library for a block)

    _borrowed = False           # True for a view of a context another object owns (MultiGpu.context)
    _lib = None

    def close(self):
        if self._c:
            if not self._borrowed:
                self._lib.aesgcm_ctx_destroy(self._c)
            self._c = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def rekey(self, key):
        """aesgcm_ctx_rekey: a new key (16 / 24 / 32 bytes) for this context -- the reference core's key load between frames; everything else stays"""
        key = bytes(key)
        _chk(self._lib.aesgcm_ctx_rekey(self._c, key, len(key)))
        return self

    def set_option(self, key, value):
        """aesgcm_ctx_set_option: "tw", "body_min", "cyc_min", "cyc_max", "cyc_close", "fold_close", "cyc_prio", "pkt_order", "rows_min", "route_top_min", "route_mid_min", "route_blocks_min", "rows_block", "wipe_on_auth_fail", "poll_us" (include/aesgcm.h)"""
        _chk(self._lib.aesgcm_ctx_set_option(self._c, key.encode(), int(value)))
        return self

    def last_launch(self):
        """aesgcm_ctx_last_launch: which launch structure the last whole-message call took (LAUNCH_MAIN / CYCLIC / CYCLIC_HALF / DEALT)"""
        v = cint(0)
        _chk(self._lib.aesgcm_ctx_last_launch(self._c, ctypes.byref(v)))
        return v.value

    def status(self):
        """aesgcm_ctx_status -> (code, detail): what an asynchronous call on this context (packets with offset arrays, messages) was refused for on the device --
        STATUS_LENGTH / STATUS_PLAN / STATUS_UNITS, detail = the first offending message for LENGTH -- or (STATUS_OK, 0).  Reading clears it.  Synchronise first."""
        code, detail = cint(0), u64(0)
        _chk(self._lib.aesgcm_ctx_status(self._c, ctypes.byref(code), ctypes.byref(detail)))
        return code.value, detail.value

    def last_route(self):
        """aesgcm_ctx_last_route -> dict(route_min, n_small, lanes, row_units): what the device decided for the last call with offset arrays / scattered messages"""
        v = (u64 * 4)()
        _chk(self._lib.aesgcm_ctx_last_route(self._c, v))
        return {"route_min": v[0], "n_small": v[1], "lanes": v[2], "row_units": v[3]}

    def packets_shape(self, n_pkts, pkt_len=0, var_len=False):
        """lanes per packet packets_crypt_dev takes for such a call: 1 (k_pktl), 4 / 8 / 16 or 64 (k_pktg), or SHAPE_ROWS: by rows (k_rows); with offset arrays
        (var_len) SHAPE_MIXED: every message is routed by its own size on the device, pkt_len is ignored"""
        v = cint(0)
        _chk(self._lib.aesgcm_packets_shape(self._c, n_pkts, pkt_len, int(bool(var_len)), ctypes.byref(v)))
        return v.value

    def stream(self):
        """the context's own HIP stream as an integer handle (what stream=None means)"""
        s = vp()
        _chk(self._lib.aesgcm_ctx_stream(self._c, ctypes.byref(s)))
        return s.value

    def wait(self, other):
        """what is enqueued on this context's stream from now on starts after everything enqueued so far on `other`'s"""
        _chk(self._lib.aesgcm_ctx_wait(self._c, other._c))

    def wait_fused(self, other):
        """... starts after `other`'s most recently enqueued fused kernel (not its fold / combine tail)"""
        _chk(self._lib.aesgcm_ctx_wait_fused(self._c, other._c))

    # unit level
    def h(self):
        b = ctypes.create_string_buffer(16)
        _chk(self._lib.aesgcm_get_h(self._c, b))
        return b.raw

    def ecb_encrypt(self, blocks):
        b = _Buf(blocks)
        if b.n % 16:
            raise AesGcmError(EARG, "ECB input must be a multiple of 16 bytes")
        out = bytearray(b.n)
        o = _Buf(out, writable=True)
        _chk(self._lib.aesgcm_ecb_encrypt(self._c, b.addr, b.n // 16, o.addr))
        return bytes(out)

    def ghash(self, data):
        b = _Buf(data)
        y = ctypes.create_string_buffer(16)
        _chk(self._lib.aesgcm_ghash(self._c, b.addr, b.n, y))
        return y.raw

    def keystream(self, iv, first_block, nblocks):
        out = bytearray(16 * nblocks)
        o = _Buf(out, writable=True)
        _chk(self._lib.aesgcm_keystream(self._c, _fixed(iv, 12, "iv"), first_block, nblocks, o.addr))
        return bytes(out)

    # whole messages, host buffers
    def encrypt(self, iv, aad, pt, out=None):
        """-> (ct, tag)"""
        a, p = _Buf(aad), _Buf(pt)
        ret = out if out is not None else bytearray(p.n)
        o = _Buf(ret, writable=True)
        tag = ctypes.create_string_buffer(16)
        _chk(self._lib.aesgcm_encrypt(self._c, _fixed(iv, 12, "iv"), a.addr, a.n, p.addr, p.n, o.addr, tag))
        return (bytes(ret) if out is None else ret), tag.raw

    def decrypt(self, iv, aad, ct, tag=None, out=None):
        """-> (pt, computed_tag); raises AuthenticationError when `tag` is given and does not match
        (the plaintext has been produced regardless, as in the reference model)."""
        a, c = _Buf(aad), _Buf(ct)
        ret = out if out is not None else bytearray(c.n)
        o = _Buf(ret, writable=True)
        tout = ctypes.create_string_buffer(16)
        exp = _fixed(tag, 16, "tag") if tag is not None else None
        rc = self._lib.aesgcm_decrypt(self._c, _fixed(iv, 12, "iv"), a.addr, a.n, c.addr, c.n, o.addr, exp, tout)
        self.last_plaintext = bytes(ret) if out is None else ret
        _chk(rc)
        return self.last_plaintext, tout.raw

    def encrypt_pipelined(self, iv, aad, pt, out=None, chunk_bytes=0):
        """Host buffers, H2D / kernel / D2H overlapped in chunks -> (ct, tag)."""
        a, p = _Buf(aad), _Buf(pt)
        ret = out if out is not None else bytearray(p.n)
        o = _Buf(ret, writable=True)
        tag = ctypes.create_string_buffer(16)
        _chk(self._lib.aesgcm_encrypt_pipelined(self._c, _fixed(iv, 12, "iv"), a.addr, a.n, p.addr, p.n, o.addr, tag, chunk_bytes))
        return (bytes(ret) if out is None else ret), tag.raw

    def decrypt_pipelined(self, iv, aad, ct, tag=None, out=None, chunk_bytes=0):
        a, c = _Buf(aad), _Buf(ct)
        ret = out if out is not None else bytearray(c.n)
        o = _Buf(ret, writable=True)
        tout = ctypes.create_string_buffer(16)
        exp = _fixed(tag, 16, "tag") if tag is not None else None
        rc = self._lib.aesgcm_decrypt_pipelined(self._c, _fixed(iv, 12, "iv"), a.addr, a.n, c.addr, c.n, o.addr, exp, tout, chunk_bytes)
        self.last_plaintext = bytes(ret) if out is None else ret
        _chk(rc)
        return self.last_plaintext, tout.raw

    # whole messages, device buffers
    def encrypt_dev(self, iv, d_pt, nbytes, d_ct, d_aad=None, aad_len=0, stream=None, want_tag=True):
        tag = ctypes.create_string_buffer(16) if want_tag else None
        _chk(self._lib.aesgcm_encrypt_dev(self._c, _fixed(iv, 12, "iv"), d_aad, aad_len, d_pt, nbytes, d_ct, tag, stream))
        return tag.raw if want_tag else None

    def decrypt_dev(self, iv, d_ct, nbytes, d_pt, d_aad=None, aad_len=0, tag=None, stream=None, want_tag=True):
        tout = ctypes.create_string_buffer(16) if want_tag else None
        exp = _fixed(tag, 16, "tag") if tag is not None else None
        _chk(self._lib.aesgcm_decrypt_dev(self._c, _fixed(iv, 12, "iv"), d_aad, aad_len, d_ct, nbytes, d_pt, exp, tout, stream))
        return tout.raw if want_tag else None

    def last_tag(self, stream=None):
        t = ctypes.create_string_buffer(16)
        _chk(self._lib.aesgcm_last_tag(self._c, t, stream))
        return t.raw

    def keystream_dev(self, iv, first_block, nblocks, d_out, stream=None):
        _chk(self._lib.aesgcm_keystream_dev(self._c, _fixed(iv, 12, "iv"), first_block, nblocks, d_out, stream))

    # many packets under this context's key
    def packets_crypt_dev(self, decrypt, n_pkts, d_ivs, d_in, d_out, d_tags, pkt_len=0, d_data_off=None,
                          d_aad=None, aad_len=0, d_aad_off=None, d_expect_tags=None, d_auth=None, stream=None):
        _chk(self._lib.aesgcm_packets_crypt_dev(self._c, int(bool(decrypt)), n_pkts, d_ivs, d_aad, aad_len, d_aad_off,
                                             d_in, pkt_len, d_data_off, d_out, d_tags, d_expect_tags, d_auth, stream))

    def frames_ceiling_probe_dev(self, n_pkts, d_ivs, d_data_off, d_tags, d_aad=None, d_aad_off=None, stream=None):
        """aesgcm_frames_ceiling_probe_dev: the packet kernels' instruction stream over these frames without the data's loads and stores (measurement support)"""
        _chk(self._lib.aesgcm_frames_ceiling_probe_dev(self._c, n_pkts, d_ivs, d_aad, d_aad_off, d_data_off, d_tags, stream))

    def messages_crypt_dev(self, decrypt, n_msgs, d_ivs, d_in_ptr, d_len, d_out_ptr, d_tags, d_aad_ptr=None, d_aad_len=None, d_expect_tags=None, d_auth=None, stream=None):
        """aesgcm_messages_crypt_dev: n_msgs messages wherever they live -- device arrays of addresses (uint64) and lengths (uint32) -- under the context's key, by rows"""
        _chk(self._lib.aesgcm_messages_crypt_dev(self._c, int(bool(decrypt)), n_msgs, d_ivs, d_aad_ptr, d_aad_len, d_in_ptr, d_len, d_out_ptr, d_tags, d_expect_tags, d_auth, stream))

    # shards
    def shard_crypt_dev(self, decrypt, iv, d_in, nbytes, d_out, first_block, total_len, d_partial,
                        d_aad=None, aad_len=0, stream=None):
        _chk(self._lib.aesgcm_shard_crypt_dev(self._c, int(bool(decrypt)), _fixed(iv, 12, "iv"), d_aad, aad_len,
                                           d_in, nbytes, d_out, first_block, total_len, d_partial, stream))

    def shard_finalize_dev(self, iv, d_partials, n_partials, aad_len, total_len, stream=None, want_tag=True, stride_bytes=16):
        tag = ctypes.create_string_buffer(16) if want_tag else None
        _chk(self._lib.aesgcm_shard_finalize_strided_dev(self._c, _fixed(iv, 12, "iv"), d_partials, n_partials, stride_bytes, aad_len, total_len, tag, stream))
        return tag.raw if want_tag else None

    def shard_finalize_batch_dev(self, ivs, d_partials, n_partials, total_lens, aad_lens=None, stride_bytes=None, msg_stride_bytes=16, stream=None):
        """the tags of len(ivs) messages in one launch and one wait (aesgcm_shard_finalize_batch_dev); default layout [rank][message][16]"""
        n = len(ivs)
        ivb = b"".join(_fixed(iv, 12, "iv") for iv in ivs)
        tl = (u64 * n)(*total_lens)
        al = (sz * n)(*aad_lens) if aad_lens is not None else None
        tags = ctypes.create_string_buffer(16 * n)
        _chk(self._lib.aesgcm_shard_finalize_batch_dev(self._c, n, ivb, d_partials, n_partials, 16 * n if stride_bytes is None else stride_bytes,
                                                    msg_stride_bytes, al, tl, tags, stream))
        return [tags.raw[16 * m:16 * m + 16] for m in range(n)]

    # streaming
    def stream_begin(self, iv, decrypt=False):
        _chk(self._lib.aesgcm_stream_begin(self._c, _fixed(iv, 12, "iv"), int(bool(decrypt))))

    def stream_aad(self, aad):
        b = _Buf(aad)
        _chk(self._lib.aesgcm_stream_aad(self._c, b.addr, b.n))

    def stream_update(self, data):
        b = _Buf(data)
        out = bytearray(b.n)
        o = _Buf(out, writable=True)
        _chk(self._lib.aesgcm_stream_update(self._c, b.addr, b.n, o.addr))
        return bytes(out)

    def stream_final(self):
        t = ctypes.create_string_buffer(16)
        _chk(self._lib.aesgcm_stream_final(self._c, t))
        return t.raw

    def stream_update_dev(self, d_in, nbytes, d_out, stream=None):
        """aesgcm_stream_update_dev: the next chunk of the open session on device pointers, asynchronous on `stream` (None = the context's own)"""
        _chk(self._lib.aesgcm_stream_update_dev(self._c, d_in, nbytes, d_out, stream))

    def stream_export(self):
        """aesgcm_stream_export -> the 64-byte state of the open session; the session stays open.  No key in it, but it gives H with the public data: keep it like the key"""
        b = ctypes.create_string_buffer(64)
        _chk(self._lib.aesgcm_stream_export(self._c, b))
        return b.raw

    def stream_import(self, blob):
        """aesgcm_stream_import: open a session in this context at the point `blob` (another context's stream_export under the same key) was taken"""
        _chk(self._lib.aesgcm_stream_import(self._c, _fixed(blob, 64, "blob")))

    # measurement
    def timing_enable(self, on=True):
        _chk(self._lib.aesgcm_ctx_timing_enable(self._c, int(on)))

    def timing_read(self, reset=True):
        n, ms = u64(0), ctypes.c_double(0)
        _chk(self._lib.aesgcm_ctx_timing_read(self._c, ctypes.byref(n), ctypes.byref(ms), int(reset)))
        return n.value, ms.value

    def wg_trace(self, max_wgs=512):
        """[(start, end, hw_id, xcc_id)] per workgroup of the last timed launch (100 MHz wall clock)."""
        buf = (u64 * (4 * max_wgs))()
        n = sz(0)
        _chk(self._lib.aesgcm_ctx_wg_trace(self._c, buf, max_wgs, ctypes.byref(n)))
        return [tuple(buf[4 * i:4 * i + 4]) for i in range(n.value)]

    def geometry(self, body=False):
        """launch geometry of k_main, or (body=True) of k_body, the kernel of the aligned middle of ranges >= 256 MiB"""
        a, b, c = cint(0), cint(0), cint(0)
        fn = self._lib.aesgcm_ctx_body_geometry if body else self._lib.aesgcm_ctx_geometry
        _chk(fn(self._c, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)))
        return dict(workgroups=a.value, wg_lanes=b.value, lds_bytes=c.value)

    def ceiling_probe(self, nbytes):
        """(ms, blocks) of the fused kernel's instruction stream without its HBM traffic (aesgcm_ctx_ceiling_probe)"""
        ms, nb = ctypes.c_double(0), u64(0)
        _chk(self._lib.aesgcm_ctx_ceiling_probe(self._c, nbytes, ctypes.byref(ms), ctypes.byref(nb)))
        return ms.value, nb.value

    def split(self, nbytes, first_block=0):
        """(head_blocks, body_blocks) of the head / k_body / tail cut of a data range; body_blocks = 0: one k_main launch"""
        h, b = u64(0), u64(0)
        _chk(self._lib.aesgcm_ctx_split(self._c, nbytes, first_block, ctypes.byref(h), ctypes.byref(b)))
        return h.value, b.value


# ---------------------------------------------------------------- key tables (aesgcm_keytab_*)
def _keytab_typed(L):
    """type the aesgcm_keytab_* symbols on first use, not in _typed: the fake runtime of tests/fake_hip links no key-table unit and still loads"""
    if not getattr(L, "_keytab_typed", False):
        L.aesgcm_keytab_create.argtypes = [ctypes.POINTER(vp), cint, sz, sz]
        L.aesgcm_keytab_set.argtypes = [vp, sz, sz, vp, vp]
        L.aesgcm_keytab_set_dev.argtypes = [vp, sz, vp, vp, vp]
        L.aesgcm_keytab_clear.argtypes = [vp, sz, sz, vp]
        L.aesgcm_keytab_crypt_dev.argtypes = [vp, cint, sz, vp, vp, vp, sz, vp, vp, sz, vp, vp, vp, vp, vp, vp]
        L.aesgcm_keytab_status.argtypes = [vp, ctypes.POINTER(cint), ctypes.POINTER(u64)]
        L.aesgcm_keytab_destroy.argtypes = [vp]
        L.aesgcm_wire_fmt_check.argtypes = [ctypes.POINTER(WireFormat)]
        L.aesgcm_keytab_set_salt.argtypes = [vp, sz, sz, vp, vp]
        L.aesgcm_keytab_frames_crypt_dev.argtypes = [vp, cint, ctypes.POINTER(WireFormat), sz, vp, vp, vp, vp, vp, vp]
        L.aesgcm_wire_xfmt_check.argtypes = [ctypes.POINTER(WireFormatX)]
        L.aesgcm_keytab_set_xpn.argtypes = [vp, sz, sz, vp, vp, vp]
        L.aesgcm_keytab_frames_crypt_x_dev.argtypes = [vp, cint, ctypes.POINTER(WireFormatX), sz, vp, vp, vp, vp, vp, vp, vp]
        L.aesgcm_tls_fmt_check.argtypes = [ctypes.POINTER(TlsFormat)]
        L.aesgcm_keytab_set_tls_iv.argtypes = [vp, sz, sz, vp, vp]
        L.aesgcm_keytab_records_crypt_dev.argtypes = [vp, cint, ctypes.POINTER(TlsFormat), sz, vp, vp, vp, vp, vp, vp, vp]
        L.aesgcm_keytab_quic_crypt_dev.argtypes = [vp, cint, sz, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
        L.aesgcm_dtls_fmt_check.argtypes = [ctypes.POINTER(DtlsFormat)]
        L.aesgcm_keytab_dtls_crypt_dev.argtypes = [vp, cint, ctypes.POINTER(DtlsFormat), sz, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
        L.aesgcm_srtp_fmt_check.argtypes = [ctypes.POINTER(SrtpFormat)]
        L.aesgcm_keytab_srtp_crypt_dev.argtypes = [vp, cint, ctypes.POINTER(SrtpFormat), sz, vp, vp, vp, vp, vp, vp, vp]
        L.aesgcm_keytab_ssh_crypt_dev.argtypes = [vp, cint, sz, vp, vp, vp, vp, vp, vp, vp]
        L._keytab_typed = True
    return L


class _Format:
    """what the format structs share: check() through the C symbol the class names in _check (typed on first use by _typed), and the repr of the fields by name"""
    _typed = staticmethod(_keytab_typed)

    def check(self):
        """aesgcm_*_fmt_check -> OK or EARG (no device needed)"""
        return getattr(self._typed(load()), self._check)(ctypes.byref(self))

    def __repr__(self):
        vals = [(f, getattr(self, f)) for f, _ in self._fields_]
        return "%s(%s)" % (type(self).__name__, ", ".join("%s=%d" % fv if isinstance(fv[1], int) else repr(fv[1]) for fv in vals))      # a nested format: positionally


WIRE_AUTH_ONLY = 1      # AESGCM_WIRE_AUTH_ONLY


class WireFormat(_Format, ctypes.Structure):
    """aesgcm_wire_fmt: how a frame header | payload | ICV is laid out (include/aesgcm.h "frames in WIRE FORMAT")"""
    _fields_ = [("aad_len", ctypes.c_uint32), ("hdr_len", ctypes.c_uint32), ("iv_off", ctypes.c_uint32), ("salt_len", ctypes.c_uint32),
                ("tag_len", ctypes.c_uint32), ("flags", ctypes.c_uint32)]
    _check = "aesgcm_wire_fmt_check"

    @classmethod
    def macsec(cls, sci=True, auth_only=False):
        """IEEE 802.1AE: DA SA | SecTAG (with or without the explicit SCI) | user data | 16-byte ICV; the slot's salt = the SCI, the PN is read from the SecTAG"""
        h = 28 if sci else 20
        return cls(h, h, 16, 8, 16, WIRE_AUTH_ONLY if auth_only else 0)

    @classmethod
    def esp(cls, tag_len=16):
        """RFC 4106: SPI, sequence number | 8-byte IV field | payload | ICV of 16, 12 or 8 bytes; the slot's salt = the SA's 4-byte salt"""
        return cls(8, 16, 8, 4, tag_len, 0)


WIREX_XPN = 1           # AESGCM_WIREX_XPN
WIREX_ESN = 2           # AESGCM_WIREX_ESN


class WireFormatX(_Format, ctypes.Structure):
    """aesgcm_wire_xfmt: a WireFormat and what the 32-bit number per frame that is not on the wire does (include/aesgcm.h "wire frames with 64-BIT NUMBERS")"""
    _fields_ = [("f", WireFormat), ("ext", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]
    _check = "aesgcm_wire_xfmt_check"

    @classmethod
    def macsec_xpn(cls, sci=True, auth_only=False):
        """IEEE 802.1AEbw: a MACsec frame whose nonce is the slot's 12-byte XPN salt XOR (SSCI | 64-bit PN); hi = the PN's upper half, the SecTAG holds the lower"""
        return cls(WireFormat.macsec(sci=sci, auth_only=auth_only), WIREX_XPN, 0)

    @classmethod
    def esp_esn(cls, tag_len=16):
        """RFC 4303 / RFC 4106 section 5: an ESP frame whose AAD is SPI | seq-hi | seq-lo; hi = seq-hi, which is never transmitted"""
        return cls(WireFormat.esp(tag_len), WIREX_ESN, 0)


TLS_13 = 1              # AESGCM_TLS_13
TLS_12 = 2              # AESGCM_TLS_12


class TlsFormat(_Format, ctypes.Structure):
    """aesgcm_tls_fmt: which TLS record header | ciphertext | tag a records call takes (include/aesgcm.h "TLS RECORDS")"""
    _fields_ = [("version", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]
    _check = "aesgcm_tls_fmt_check"

    @classmethod
    def tls13(cls):
        """RFC 8446: hdr[5] | payload | tag[16]; nonce = the slot's IV XOR the 64-bit sequence number, AAD = the header"""
        return cls(TLS_13, 0)

    @classmethod
    def tls12(cls):
        """RFC 5288: hdr[5] | explicit nonce[8] | payload | tag[16]; nonce = the slot IV's four bytes | explicit nonce, AAD = seq | type, version | payload length"""
        return cls(TLS_12, 0)


DTLS_13 = 1             # AESGCM_DTLS_13
DTLS_12 = 2             # AESGCM_DTLS_12


class DtlsFormat(_Format, ctypes.Structure):
    """aesgcm_dtls_fmt: which DTLS record a dtls call takes (include/aesgcm.h "DTLS RECORDS")"""
    _fields_ = [("version", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]
    _check = "aesgcm_dtls_fmt_check"

    @classmethod
    def dtls13(cls):
        """RFC 9147: unified_hdr | payload | tag[16]; nonce = the slot's IV XOR the 64-bit record sequence number, AAD = the unprotected header, the sequence bytes
        masked under a second slot"""
        return cls(DTLS_13, 0)

    @classmethod
    def dtls12(cls):
        """RFC 6347 / RFC 5288: hdr[13] | explicit nonce[8] | payload | tag[16]; nonce = the slot IV's four bytes | explicit nonce, AAD = epoch, sequence number (from
        the record) | type, version | payload length"""
        return cls(DTLS_12, 0)


SRTP_RTP = 1            # AESGCM_SRTP_RTP
SRTP_RTCP = 2           # AESGCM_SRTP_RTCP


class SrtpFormat(_Format, ctypes.Structure):
    """aesgcm_srtp_fmt: which packet an srtp call takes and how many bytes of MKI end it (include/aesgcm.h "SRTP AND SRTCP PACKETS")"""
    _fields_ = [("kind", ctypes.c_uint32), ("mki_len", ctypes.c_uint32)]
    _check = "aesgcm_srtp_fmt_check"

    @classmethod
    def rtp(cls, mki_len=0):
        """RFC 7714 over RFC 3711 3.1: rtp_hdr | payload | tag[16] | mki; the header's length from the packet, nonce = the slot's salt XOR (SSRC, the rollover counter,
        the sequence number), AAD = the header"""
        return cls(SRTP_RTP, mki_len)

    @classmethod
    def rtcp(cls, mki_len=0):
        """RFC 7714 over RFC 3711 3.4: rtcp_hdr[8] | payload | tag[16] | W[4] | mki, W = E | index; nonce = the slot's salt XOR (SSRC, the index); AAD = the header | W, or
        with E clear everything in front of the tag | W"""
        return cls(SRTP_RTCP, mki_len)


def _per_slot(x, width, what, pad=False):
    """a setter's host data: one bytes-like of n * width bytes, or a list of n items (pad: shorter ones zero-padded to width) -> (bytes, n)"""
    items = [bytes(i) for i in x] if isinstance(x, (list, tuple)) else None
    b = bytes(x) if items is None else b"".join(i.ljust(width, b"\0") if pad else i for i in items)
    if len(b) % width or (pad and items is not None and any(len(i) > width for i in items)):
        raise AesGcmError(EARG, what)
    return b, len(b) // width


def _joined(items):
    """a byte string per packet -> (the packets side by side, their n + 1 offsets)"""
    off = [0]
    for x in items:
        off.append(off[-1] + len(x))
    return b"".join(bytes(x) for x in items), off


def _device_call(device, up, down, call):
    """What the tables' host conveniences share.  Every entry of `up` -- name: bytes, or (struct code, values) -- uploaded into a DeviceBuffer of its name; every entry
    of `down` -- name: (struct code, count) of the values that come back -- allocated (a name in both is one buffer); then call(bufs) over the DeviceBuffers by name, a
    device sync and the downloads.  -> {name: list of count values}"""
    up = {k: v if isinstance(v, bytes) else struct.pack("<%d%s" % (len(v[1]), v[0]), *v[1]) for k, v in up.items()}
    down = {k: (code, count, count * struct.calcsize("<" + code)) for k, (code, count) in down.items()}
    size = {k: len(v) for k, v in up.items()}
    for k, (_, _, nb) in down.items():
        size[k] = max(size.get(k, 0), nb)
    bufs = {k: DeviceBuffer(max(nb, 16), device) for k, nb in size.items()}
    try:
        for k, v in up.items():
            if v:
                bufs[k].upload(v)
        call(bufs)
        _chk(load().aesgcm_dev_sync(device))
        return {k: list(struct.unpack("<" + code * count, bytes(bufs[k].download(nb)) if nb else b"")) for k, (code, count, nb) in down.items()}
    finally:
        for b in bufs.values():
            b.free()


class _Table:
    """what KeyTable, RxWindows, TxCounters, SecretTable, MasterKeyTable, MasterSecretTable, IkeSaTable and CakTable share: the handle of a device table made by <_prefix>_create, which belongs to the library that made it (_lib); close, the
    context manager, status()"""
    _h = _lib = None

    def _create(self, typed, device, *args):
        L = typed(load())
        h = vp()
        _chk(getattr(L, self._prefix + "_create")(ctypes.byref(h), device, *args))
        self._h, self._lib, self.device = h.value, L, device

    def close(self):
        if self._h:
            getattr(self._lib, self._prefix + "_destroy")(self._h)
            self._h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def status(self):
        """aesgcm_keytab_status / aesgcm_rxwin_status -> (code, detail): (EARG, lowest refused packet) or (OK, 0).  Reading clears it.  Synchronise first."""
        code, detail = cint(0), u64(0)
        _chk(getattr(self._lib, self._prefix + "_status")(self._h, ctypes.byref(code), ctypes.byref(detail)))
        return code.value, detail.value


class KeyTable(_Table):
    """aesgcm_keytab: n_slots device-resident slots of one key size; the key schedule, H and its powers are computed on the GPU once per `set`, and a crypt call
    names a slot per packet (include/aesgcm.h "key tables").  Belongs to the library that made it (create it inside a debug_library block to force shapes)."""
    _prefix = "aesgcm_keytab"

    def __init__(self, key_len, n_slots, device=0):
        self._create(_keytab_typed, device, key_len, n_slots)
        self.key_len, self.n_slots = key_len, n_slots

    def set(self, first_slot, keys, stream=None):
        """aesgcm_keytab_set: host keys (one bytes-like of n * key_len bytes, or a list of keys) into slots first_slot, first_slot + 1, ..."""
        kb, n = _per_slot(keys, self.key_len, "keys must be a multiple of %d bytes" % self.key_len)
        _chk(self._lib.aesgcm_keytab_set(self._h, first_slot, n, kb, stream))
        return self

    def set_dev(self, n, d_slots, d_keys, stream=None):
        """aesgcm_keytab_set_dev: n keys from device memory (n x key_len bytes) into the slots d_slots (n uint32, device memory)"""
        _chk(self._lib.aesgcm_keytab_set_dev(self._h, n, d_slots, d_keys, stream))
        return self

    def clear(self, first_slot, n=1, stream=None):
        """aesgcm_keytab_clear: retire slots first_slot .. first_slot + n - 1 (zeroed, unset: their packets are refused)"""
        _chk(self._lib.aesgcm_keytab_clear(self._h, first_slot, n, stream))
        return self

    def crypt_dev(self, decrypt, n_pkts, d_slots, d_ivs, d_in, d_data_off, d_out, d_tags, d_aad=None, d_aad_off=None,
                  d_expect_tags=None, d_auth=None, pkt_len=0, aad_len=0, stream=None):
        """aesgcm_keytab_crypt_dev: packet p under slot d_slots[p] (uint32, device memory); the rest as batch_crypt_var_dev.  d_data_off = None: fixed-size
        records of pkt_len bytes (and aad_len bytes of AAD each unless d_aad_off is given)."""
        _chk(self._lib.aesgcm_keytab_crypt_dev(self._h, int(bool(decrypt)), n_pkts, d_slots, d_ivs, d_aad, aad_len, d_aad_off,
                                               d_in, pkt_len, d_data_off, d_out, d_tags, d_expect_tags, d_auth, stream))

    def set_salt(self, first_slot, salts, stream=None):
        """aesgcm_keytab_set_salt: 8 bytes per slot (one bytes-like of n * 8 bytes, or a list; shorter entries are zero-padded) into slots first_slot, ..."""
        sb, n = _per_slot(salts, 8, "a salt is 8 bytes", pad=True)
        _chk(self._lib.aesgcm_keytab_set_salt(self._h, first_slot, n, sb, stream))
        return self

    def frames_crypt_dev(self, decrypt, fmt, n_frames, d_slots, d_in, d_frame_off, d_out, d_auth=None, stream=None):
        """aesgcm_keytab_frames_crypt_dev: frame p = bytes [d_frame_off[p], d_frame_off[p + 1]) of d_in / d_out in the wire format fmt, under slot d_slots[p]"""
        _chk(self._lib.aesgcm_keytab_frames_crypt_dev(self._h, int(bool(decrypt)), ctypes.byref(fmt), n_frames, d_slots, d_in, d_frame_off, d_out, d_auth, stream))

    def set_xpn(self, first_slot, salts, sscis, stream=None):
        """aesgcm_keytab_set_xpn: MACsec XPN's 12-byte salt and 4-byte SSCI per slot (each one bytes-like of n * 12 / n * 4 bytes, or a list) into slots first_slot, ..."""
        what = "an XPN salt is 12 bytes, an SSCI 4, one of each per slot"
        (sb, n), (cb, nc) = _per_slot(salts, 12, what), _per_slot(sscis, 4, what)
        if n != nc:
            raise AesGcmError(EARG, what)
        _chk(self._lib.aesgcm_keytab_set_xpn(self._h, first_slot, n, sb, cb, stream))
        return self

    def frames_crypt_x_dev(self, decrypt, xfmt, n_frames, d_slots, d_hi, d_in, d_frame_off, d_out, d_auth=None, stream=None):
        """aesgcm_keytab_frames_crypt_x_dev: frames_crypt_dev in the format xfmt (WireFormatX) with d_hi[p] (uint32, device memory) = the upper half of frame p's
        64-bit packet / sequence number"""
        _chk(self._lib.aesgcm_keytab_frames_crypt_x_dev(self._h, int(bool(decrypt)), ctypes.byref(xfmt), n_frames, d_slots, d_hi, d_in, d_frame_off, d_out, d_auth, stream))

    def crypt_frames(self, fmt, slots, frames, decrypt=False, hi=None):
        """Host convenience (tests, examples): whole frames (header | payload | ICV; on encrypt the ICV bytes are placeholders) through one call, in place.
        fmt a WireFormatX: through frames_crypt_x_dev with hi (one number per frame).  -> (frames_out, auth); auth is None on encrypt."""
        n = len(slots)
        if len(frames) != n or not n:
            raise AesGcmError(EARG, "slots and frames must be equally long and not empty")
        ext = isinstance(fmt, WireFormatX)
        if (hi is not None and not ext) or (hi is not None and len(hi) != n):
            raise AesGcmError(EARG, "hi goes with a WireFormatX, one number per frame")

        def call(b):
            auth = b["auth"].ptr if decrypt else None
            if ext:
                self.frames_crypt_x_dev(decrypt, fmt, n, b["slots"].ptr, b["hi"].ptr if hi is not None else None, b["data"].ptr, b["off"].ptr, b["data"].ptr, d_auth=auth)
            else:
                self.frames_crypt_dev(decrypt, fmt, n, b["slots"].ptr, b["data"].ptr, b["off"].ptr, b["data"].ptr, d_auth=auth)
        outs, got = self._packed_call(frames, {"slots": ("I", slots), "hi": ("I", hi if hi is not None else ())}, {"auth": "i"} if decrypt else {}, call)
        return outs, got.get("auth")

    def set_tls_iv(self, first_slot, ivs, stream=None):
        """aesgcm_keytab_set_tls_iv: a TLS connection direction's 12-byte write IV per slot (one bytes-like of n * 12 bytes, or a list) into slots first_slot, ...;
        it takes the place of the slot's XPN state"""
        ib, n = _per_slot(ivs, 12, "a TLS write IV is 12 bytes")
        _chk(self._lib.aesgcm_keytab_set_tls_iv(self._h, first_slot, n, ib, stream))
        return self

    def records_crypt_dev(self, decrypt, fmt, n_recs, d_slots, d_seq, d_in, d_rec_off, d_out, d_auth=None, stream=None):
        """aesgcm_keytab_records_crypt_dev: TLS record p = bytes [d_rec_off[p], d_rec_off[p + 1]) of d_in / d_out, of the version fmt (TlsFormat) says, under slot
        d_slots[p] with the 64-bit sequence number d_seq[p] (uint64, device memory)"""
        _chk(self._lib.aesgcm_keytab_records_crypt_dev(self._h, int(bool(decrypt)), ctypes.byref(fmt), n_recs, d_slots, d_seq, d_in, d_rec_off, d_out, d_auth, stream))

    def crypt_records(self, fmt, slots, seqs, records, decrypt=False):
        """Host convenience (tests, examples), crypt_frames' counterpart: whole TLS records (header | (1.2: explicit nonce |) payload | tag; on encrypt the tag's bytes are
        placeholders) with a sequence number each through one call, in place.  -> (records_out, auth); auth is None on encrypt."""
        n = len(slots)
        if len(records) != n or len(seqs) != n or not n:
            raise AesGcmError(EARG, "slots, seqs and records must be equally long and not empty")

        def call(b):
            self.records_crypt_dev(decrypt, fmt, n, b["slots"].ptr, b["seq"].ptr, b["data"].ptr, b["off"].ptr, b["data"].ptr, d_auth=b["auth"].ptr if decrypt else None)
        outs, got = self._packed_call(records, {"slots": ("I", slots), "seq": ("Q", seqs)}, {"auth": "i"} if decrypt else {}, call)
        return outs, got.get("auth")

    def ssh_crypt_dev(self, decrypt, n_pkts, d_slots, d_seq, d_in, d_pkt_off, d_out, d_auth=None, stream=None):
        """aesgcm_keytab_ssh_crypt_dev: SSH binary packet p (packet_length[4] | body | tag[16], RFC 5647) = bytes [d_pkt_off[p], d_pkt_off[p + 1]) of d_in / d_out under
        slot d_slots[p] (key by set, initial IV by set_tls_iv); d_seq[p] (uint64, device memory) = the packets sent under that key before this one, added to the IV's
        invocation counter"""
        _chk(self._lib.aesgcm_keytab_ssh_crypt_dev(self._h, int(bool(decrypt)), n_pkts, d_slots, d_seq, d_in, d_pkt_off, d_out, d_auth, stream))

    def crypt_ssh(self, slots, seqs, packets, decrypt=False):
        """Host convenience (tests, examples), crypt_records' counterpart: whole SSH packets (packet_length | body | tag; on encrypt the length field is written and the
        tag's bytes are placeholders) with a packet count each through one call, in place.  -> (packets_out, auth); auth is None on encrypt."""
        n = len(slots)
        if len(packets) != n or len(seqs) != n or not n:
            raise AesGcmError(EARG, "slots, seqs and packets must be equally long and not empty")

        def call(b):
            self.ssh_crypt_dev(decrypt, n, b["slots"].ptr, b["seq"].ptr, b["data"].ptr, b["off"].ptr, b["data"].ptr, d_auth=b["auth"].ptr if decrypt else None)
        outs, got = self._packed_call(packets, {"slots": ("I", slots), "seq": ("Q", seqs)}, {"auth": "i"} if decrypt else {}, call)
        return outs, got.get("auth")

    def quic_crypt_dev(self, decrypt, n_pkts, d_slots, d_hp_slots, d_pn, d_pn_off, d_in, d_pkt_off, d_out, d_pn_out=None, d_auth=None, stream=None):
        """aesgcm_keytab_quic_crypt_dev: QUIC packet p = bytes [d_pkt_off[p], d_pkt_off[p + 1]) of d_in / d_out, its packet-number field at byte d_pn_off[p] (uint32), under
        the AEAD slot d_slots[p] (key by set, IV by set_tls_iv) and the header-protection slot d_hp_slots[p] (key by set).  d_pn[p] (uint64): the full packet number on
        encrypt, the expected one on decrypt, where the decoded number goes to d_pn_out[p] (may be d_pn) and the verdict to d_auth[p]"""
        _chk(self._lib.aesgcm_keytab_quic_crypt_dev(self._h, int(bool(decrypt)), n_pkts, d_slots, d_hp_slots, d_pn, d_pn_out, d_pn_off, d_in, d_pkt_off, d_out, d_auth, stream))

    def crypt_quic(self, slots, hp_slots, pns, pn_offs, packets, decrypt=False):
        """Host convenience (tests, examples), crypt_records' counterpart: whole QUIC packets (header | payload | tag; on encrypt the header is unprotected with the truncated
        packet number written and the tag's bytes are placeholders) through one call, in place.  pns: the full packet numbers (encrypt) or the expected ones (decrypt).
        -> (packets_out, auth, pns_out); auth and pns_out are None on encrypt."""
        n = len(slots)
        if len(packets) != n or len(hp_slots) != n or len(pns) != n or len(pn_offs) != n or not n:
            raise AesGcmError(EARG, "slots, hp_slots, pns, pn_offs and packets must be equally long and not empty")
        up = {"slots": ("I", slots), "hp": ("I", hp_slots), "pn": ("Q", pns), "pn_off": ("I", pn_offs)}
        if decrypt:
            up.update(auth=bytes(4 * n), pn_out=bytes(8 * n))                      # zero where a refused packet leaves them alone

        def call(b):
            self.quic_crypt_dev(decrypt, n, b["slots"].ptr, b["hp"].ptr, b["pn"].ptr, b["pn_off"].ptr, b["data"].ptr, b["off"].ptr, b["data"].ptr,
                                d_pn_out=b["pn_out"].ptr if decrypt else None, d_auth=b["auth"].ptr if decrypt else None)
        outs, got = self._packed_call(packets, up, {"auth": "i", "pn_out": "Q"} if decrypt else {}, call)
        return outs, got.get("auth"), got.get("pn_out")

    def dtls_crypt_dev(self, decrypt, fmt, n_recs, d_slots, d_in, d_rec_off, d_out, d_sn_slots=None, d_seq=None, d_sn_off=None, d_seq_out=None, d_auth=None, stream=None):
        """aesgcm_keytab_dtls_crypt_dev: DTLS record p = bytes [d_rec_off[p], d_rec_off[p + 1]) of d_in / d_out, of the version fmt (DtlsFormat) says, under slot
        d_slots[p] (key by set, IV by set_tls_iv).  DTLS 1.3 also takes the record-number slot d_sn_slots[p] (key by set), d_sn_off[p] (uint32: where the sequence-number
        field starts) and d_seq[p] (uint64): the full record sequence number on encrypt, the expected one on decrypt, where the decoded number goes to d_seq_out[p] (may
        be d_seq).  The verdict goes to d_auth[p]"""
        _chk(self._lib.aesgcm_keytab_dtls_crypt_dev(self._h, int(bool(decrypt)), ctypes.byref(fmt), n_recs, d_slots, d_sn_slots, d_seq, d_seq_out, d_sn_off, d_in, d_rec_off,
                                                    d_out, d_auth, stream))

    def crypt_dtls(self, fmt, slots, records, decrypt=False, sn_slots=None, seqs=None, sn_offs=None):
        """Host convenience (tests, examples), crypt_quic's counterpart: whole DTLS records (on encrypt the header is written, a 1.3 record's sequence bytes unprotected, and
        the tag's bytes are placeholders) through one call, in place.  DTLS 1.3: sn_slots, sn_offs and seqs (the full numbers on encrypt, the expected ones on decrypt) per
        record.  -> (records_out, auth, seqs_out); auth is None on encrypt, seqs_out unless DTLS 1.3 decrypts."""
        n = len(slots)
        v13 = fmt.version == DTLS_13
        per = (sn_slots, seqs, sn_offs)
        if len(records) != n or not n or (v13 and any(x is None or len(x) != n for x in per)) or (not v13 and any(x is not None for x in per)):
            raise AesGcmError(EARG, "slots and records (DTLS 1.3: and sn_slots, seqs, sn_offs; DTLS 1.2: without them) must be equally long and not empty")
        up = {"slots": ("I", slots)}
        if v13:
            up.update(sn=("I", sn_slots), seq=("Q", seqs), sn_off=("I", sn_offs))
        if decrypt:
            up.update(auth=bytes(4 * n))                                           # zero where a refused record leaves them alone
            if v13:
                up.update(seq_out=bytes(8 * n))

        def call(b):
            self.dtls_crypt_dev(decrypt, fmt, n, b["slots"].ptr, b["data"].ptr, b["off"].ptr, b["data"].ptr, d_sn_slots=b["sn"].ptr if v13 else None,
                                d_seq=b["seq"].ptr if v13 else None, d_sn_off=b["sn_off"].ptr if v13 else None, d_seq_out=b["seq_out"].ptr if v13 and decrypt else None,
                                d_auth=b["auth"].ptr if decrypt else None)
        down = {"auth": "i"} if decrypt else {}
        if v13 and decrypt:
            down["seq_out"] = "Q"
        outs, got = self._packed_call(records, up, down, call)
        return outs, got.get("auth"), got.get("seq_out")

    def srtp_crypt_dev(self, decrypt, fmt, n_pkts, d_slots, d_in, d_pkt_off, d_out, d_roc=None, d_auth=None, stream=None):
        """aesgcm_keytab_srtp_crypt_dev: SRTP or SRTCP packet p (fmt, an SrtpFormat, says which) = bytes [d_pkt_off[p], d_pkt_off[p + 1]) of d_in / d_out under slot
        d_slots[p] (key by set, salt by set_tls_iv).  SRTP also takes d_roc[p] (uint32), the packet's rollover counter.  The verdict goes to d_auth[p]"""
        _chk(self._lib.aesgcm_keytab_srtp_crypt_dev(self._h, int(bool(decrypt)), ctypes.byref(fmt), n_pkts, d_slots, d_roc, d_in, d_pkt_off, d_out, d_auth, stream))

    def crypt_srtp(self, fmt, slots, packets, decrypt=False, rocs=None):
        """Host convenience (tests, examples), crypt_dtls's counterpart: whole SRTP or SRTCP packets (on encrypt the headers, SRTCP's word W and the MKI are written and
        the tag's bytes are placeholders) through one call, in place.  SRTP: rocs, a rollover counter per packet.  -> (packets_out, auth); auth is None on encrypt."""
        n = len(slots)
        rtp = fmt.kind == SRTP_RTP
        if len(packets) != n or not n or (rtp and (rocs is None or len(rocs) != n)) or (not rtp and rocs is not None):
            raise AesGcmError(EARG, "slots and packets (SRTP: and rocs; SRTCP: without them) must be equally long and not empty")
        up = {"slots": ("I", slots)}
        if rtp:
            up.update(roc=("I", rocs))
        if decrypt:
            up.update(auth=bytes(4 * n))                                           # zero where a refused packet leaves them alone

        def call(b):
            self.srtp_crypt_dev(decrypt, fmt, n, b["slots"].ptr, b["data"].ptr, b["off"].ptr, b["data"].ptr, d_roc=b["roc"].ptr if rtp else None,
                                d_auth=b["auth"].ptr if decrypt else None)
        outs, got = self._packed_call(packets, up, {"auth": "i"} if decrypt else {}, call)
        return outs, got.get("auth")

    def crypt(self, slots, ivs, aads, datas, decrypt=False, tags=None):
        """Host convenience (tests, examples): packet p = (slots[p], ivs[p], aads[p], datas[p]) through one offset-array call.
        -> (outputs, tags) on encrypt; (outputs, tags, auth) on decrypt, auth[p] = 1 when tags[p] (the expected tags given) matches."""
        n = len(slots)
        if not (len(ivs) == len(aads) == len(datas) == n) or not n:
            raise AesGcmError(EARG, "slots, ivs, aads and datas must be equally long and not empty")
        aoff = [0]
        for a in aads:
            aoff.append(aoff[-1] + len(a))
        expect = decrypt and tags is not None
        up = {"slots": ("I", slots), "ivs": b"".join(_fixed(iv, 12, "iv") for iv in ivs), "aad": b"".join(bytes(a) for a in aads), "aoff": ("Q", aoff)}
        if expect:
            up["exp"] = b"".join(_fixed(t, 16, "tag") for t in tags)

        def call(b):
            self.crypt_dev(decrypt, n, b["slots"].ptr, b["ivs"].ptr, b["data"].ptr, b["off"].ptr, b["data"].ptr, b["tags"].ptr, d_aad=b["aad"].ptr, d_aad_off=b["aoff"].ptr,
                           d_expect_tags=b["exp"].ptr if expect else None, d_auth=b["auth"].ptr if decrypt else None)
        outs, got = self._packed_call(datas, up, {"tags": "16s", "auth": "i"} if decrypt else {"tags": "16s"}, call)
        return (outs, got["tags"], got["auth"]) if decrypt else (outs, got["tags"])

    def _packed_call(self, items, up, down, call):
        """What the host conveniences share.  `items`, a byte string per packet, joined in the buffer "data" with their n + 1 offsets in "off"; `up` as _device_call's;
        every entry of `down` -- name: struct code of the n values that come back; call(bufs) works in place on "data".  -> (items_out, {name: list of n values})"""
        n = len(items)
        data, off = _joined(items)
        got = _device_call(self.device, dict(up, data=data, off=("Q", off)), dict({k: (code, n) for k, code in down.items()}, data=("%ds" % off[n], 1)), call)
        out = got.pop("data")[0]
        return [out[off[p]:off[p + 1]] for p in range(n)], got


# ---------------------------------------------------------------- receive windows (aesgcm_rxwin_*)
def _rxwin_typed(L):
    """type the aesgcm_rxwin_* symbols on first use, as _keytab_typed does: the fake runtime of tests/fake_hip links no such unit and still loads"""
    if not getattr(L, "_rxwin_typed", False):
        pu64 = ctypes.POINTER(u64)
        L.aesgcm_rxwin_create.argtypes = [ctypes.POINTER(vp), cint, sz, sz]
        L.aesgcm_rxwin_set.argtypes = [vp, sz, sz, pu64, pu64, vp]
        L.aesgcm_rxwin_get.argtypes = [vp, sz, sz, pu64, pu64, vp]
        L.aesgcm_rxwin_fmt_check.argtypes = [ctypes.POINTER(RxFormat)]
        L.aesgcm_rxwin_recover_dev.argtypes = [vp, ctypes.POINTER(RxFormat), sz, vp, vp, vp, vp, vp, vp]
        L.aesgcm_rxwin_commit_dev.argtypes = [vp, sz, vp, vp, vp, vp, vp, vp]
        L.aesgcm_rxwin_status.argtypes = [vp, ctypes.POINTER(cint), pu64]
        L.aesgcm_rxwin_destroy.argtypes = [vp]
        L._rxwin_typed = True
    return L


RXWIN_NONE = (1 << 64) - 1                                          # AESGCM_RXWIN_NONE
RXWIN_WIRE, RXWIN_LOWEST, RXWIN_SRTP, RXWIN_EXPECT = 1, 2, 3, 4     # AESGCM_RXWIN_WIRE ...
RXWIN_FROM_END, RXWIN_CLEAR_TOP = 1, 2                              # AESGCM_RXWIN_FROM_END, AESGCM_RXWIN_CLEAR_TOP
RXWIN_WHY = ("not authenticated", "accepted", "old", "replay", "refused")      # d_why's values 0 .. 4


class RxFormat(_Format, ctypes.Structure):
    """aesgcm_rxwin_fmt: where a packet's truncated number lies and how the full one is formed from it and the window (include/aesgcm.h "RECEIVE WINDOWS")"""
    _fields_ = [("rule", ctypes.c_uint32), ("num_off", ctypes.c_uint32), ("num_len", ctypes.c_uint32), ("flags", ctypes.c_uint32)]
    _check, _typed = "aesgcm_rxwin_fmt_check", staticmethod(_rxwin_typed)

    @classmethod
    def macsec(cls):
        """IEEE 802.1AE: the SecTAG's 32-bit PN is the number"""
        return cls(RXWIN_WIRE, 16, 4, 0)

    @classmethod
    def macsec_xpn(cls):
        """IEEE 802.1AEbw 10.6.2: the 64-bit PN at or above the lowest acceptable one; hi = the d_hi of frames_crypt_x_dev"""
        return cls(RXWIN_LOWEST, 16, 4, 0)

    @classmethod
    def esp(cls):
        """RFC 4303: the 32-bit sequence number"""
        return cls(RXWIN_WIRE, 4, 4, 0)

    @classmethod
    def esp_esn(cls):
        """RFC 4303 Appendix A2.1: the 64-bit sequence number; hi = seq-hi, the d_hi of frames_crypt_x_dev"""
        return cls(RXWIN_LOWEST, 4, 4, 0)

    @classmethod
    def dtls12(cls):
        """RFC 6347: the record's 48-bit sequence number (a window is an epoch)"""
        return cls(RXWIN_WIRE, 5, 6, 0)

    @classmethod
    def srtp(cls):
        """RFC 3711 3.3.1: ROC << 16 | SEQ; hi = the d_roc of srtp_crypt_dev"""
        return cls(RXWIN_SRTP, 2, 2, 0)

    @classmethod
    def srtcp(cls, mki_len=0):
        """RFC 3711 3.4: the 31-bit SRTCP index behind the tag, in front of the MKI"""
        return cls(RXWIN_WIRE, 4 + mki_len, 4, RXWIN_FROM_END | RXWIN_CLEAR_TOP)

    @classmethod
    def expect(cls):
        """QUIC and DTLS 1.3: the expected number, the window's next; no packet byte is read"""
        return cls(RXWIN_EXPECT, 0, 0, 0)


class RxWindows(_Table):
    """aesgcm_rxwin: n_wins device-resident receive windows of `window` bits; recover_dev gives a decrypt call its per-packet numbers, commit_dev drops replays and
    advances the windows behind it (include/aesgcm.h "RECEIVE WINDOWS")."""
    _prefix = "aesgcm_rxwin"

    def __init__(self, n_wins, window=64, device=0):
        self._create(_rxwin_typed, device, n_wins, window)
        self.n_wins, self.window = n_wins, window

    def set(self, first, nexts, seens=None, stream=None):
        """aesgcm_rxwin_set: windows first, first + 1, ... get next = nexts[k] and seen = seens[k], an int whose bit i says "number next - 1 - i was seen" (None: nothing)"""
        n, sw = len(nexts), self.window // 64
        nx = (u64 * max(n, 1))(*nexts)
        sn = None
        if seens is not None:
            if len(seens) != n or any(s < 0 or s >> self.window for s in seens):
                raise AesGcmError(EARG, "one seen value of at most `window` bits per window")
            sn = (u64 * max(n * sw, 1))(*[(s >> (64 * j)) & RXWIN_NONE for s in seens for j in range(sw)])
        _chk(self._lib.aesgcm_rxwin_set(self._h, first, n, nx, sn, stream))
        return self

    def get(self, first=0, n=None, stream=None):
        """aesgcm_rxwin_get -> (nexts, seens) of windows first .. first + n - 1 in set's form; waits on the stream"""
        n = self.n_wins - first if n is None else n
        sw = self.window // 64
        nx, sn = (u64 * max(n, 1))(), (u64 * max(n * sw, 1))()
        _chk(self._lib.aesgcm_rxwin_get(self._h, first, n, nx, sn, stream))
        return list(nx[:n]), [sum(sn[k * sw + j] << (64 * j) for j in range(sw)) for k in range(n)]

    def recover_dev(self, fmt, n_pkts, d_win, d_in, d_pkt_off, d_num_out, d_hi_out=None, stream=None):
        """aesgcm_rxwin_recover_dev: d_num_out[p] (uint64) = packet p's full number by fmt (an RxFormat) and window d_win[p] (uint32); d_hi_out[p] (uint32, optional) = what
        the decrypt call takes as d_hi / d_roc.  RxFormat.expect(): d_in and d_pkt_off may be None"""
        _chk(self._lib.aesgcm_rxwin_recover_dev(self._h, ctypes.byref(fmt), n_pkts, d_win, d_in, d_pkt_off, d_num_out, d_hi_out, stream))

    def commit_dev(self, n_pkts, d_win, d_num, d_auth, d_accept, d_why=None, stream=None):
        """aesgcm_rxwin_commit_dev: behind the decrypt call; d_accept[p] (int, may be d_auth) = 1 for the packets to deliver, d_why[p] (int, optional) an index of RXWIN_WHY"""
        _chk(self._lib.aesgcm_rxwin_commit_dev(self._h, n_pkts, d_win, d_num, d_auth, d_accept, d_why, stream))

    def recover(self, fmt, wins, packets=None):
        """Host convenience (tests, examples): -> (nums, his) of whole packets (RxFormat.expect(): packets may be None)"""
        n = len(wins)
        if not n or (packets is not None and len(packets) != n):
            raise AesGcmError(EARG, "wins and packets must be equally long and not empty")
        up = {"win": ("I", wins)}
        if packets is not None:
            data, off = _joined(packets)
            up.update(data=data, off=("Q", off))
        got = _device_call(self.device, up, {"num": ("Q", n), "hi": ("I", n)},
                           lambda b: self.recover_dev(fmt, n, b["win"].ptr, b["data"].ptr if packets is not None else None, b["off"].ptr if packets is not None else None,
                                                      b["num"].ptr, b["hi"].ptr))
        return got["num"], got["hi"]

    def commit(self, wins, nums, auths):
        """Host convenience (tests, examples): -> (accepts, whys)"""
        n = len(wins)
        if not n or len(nums) != n or len(auths) != n:
            raise AesGcmError(EARG, "wins, nums and auths must be equally long and not empty")
        got = _device_call(self.device, {"win": ("I", wins), "num": ("Q", nums), "auth": ("i", auths)}, {"accept": ("i", n), "why": ("i", n)},
                           lambda b: self.commit_dev(n, b["win"].ptr, b["num"].ptr, b["auth"].ptr, b["accept"].ptr, b["why"].ptr))
        return got["accept"], got["why"]


# ---------------------------------------------------------------- send counters (aesgcm_txnum_*)
def _txnum_typed(L):
    """type the aesgcm_txnum_* symbols on first use, as _rxwin_typed does: the fake runtime of tests/fake_hip links no such unit and still loads"""
    if not getattr(L, "_txnum_typed", False):
        pu64 = ctypes.POINTER(u64)
        L.aesgcm_txnum_create.argtypes = [ctypes.POINTER(vp), cint, sz, sz]
        L.aesgcm_txnum_set.argtypes = [vp, sz, sz, pu64, pu64, vp]
        L.aesgcm_txnum_get.argtypes = [vp, sz, sz, pu64, pu64, vp]
        L.aesgcm_txnum_fmt_check.argtypes = [ctypes.POINTER(TxFormat)]
        L.aesgcm_txnum_assign_dev.argtypes = [vp, ctypes.POINTER(TxFormat), sz, vp, vp, vp, vp, vp, vp, vp]
        L.aesgcm_txnum_status.argtypes = [vp, ctypes.POINTER(cint), pu64]
        L.aesgcm_txnum_destroy.argtypes = [vp]
        L._txnum_typed = True
    return L


TXNUM_FROM_END, TXNUM_KEEP_TOP, TXNUM_WHOLE = 1, 2, 4                # AESGCM_TXNUM_FROM_END, AESGCM_TXNUM_KEEP_TOP, AESGCM_TXNUM_WHOLE


class TxFormat(_Format, ctypes.Structure):
    """aesgcm_txnum_fmt: where a packet's number is written, how many of its low bytes, and what the field means (include/aesgcm.h "SEND COUNTERS")"""
    _fields_ = [("num_off", ctypes.c_uint32), ("num_len", ctypes.c_uint32), ("dup_off", ctypes.c_uint32), ("flags", ctypes.c_uint32)]
    _check, _typed = "aesgcm_txnum_fmt_check", staticmethod(_txnum_typed)

    @classmethod
    def macsec(cls):
        """IEEE 802.1AE: the SecTAG's 32-bit PN is the whole number; a counter that reaches 2^32 refuses"""
        return cls(16, 4, 0, TXNUM_WHOLE)

    @classmethod
    def macsec_xpn(cls):
        """IEEE 802.1AEbw: the SecTAG holds the 64-bit PN's lower half; hi = the d_hi of frames_crypt_x_dev"""
        return cls(16, 4, 0, 0)

    @classmethod
    def esp(cls):
        """RFC 4303: the 32-bit sequence number is the whole number"""
        return cls(4, 4, 0, TXNUM_WHOLE)

    @classmethod
    def esp_esn(cls):
        """RFC 4303 / RFC 4106 section 5: the header holds seq-lo; hi = seq-hi, the d_hi of frames_crypt_x_dev"""
        return cls(4, 4, 0, 0)

    @classmethod
    def tls12(cls):
        """RFC 5288: the record's 8-byte explicit nonce = the sequence number (nums = the d_seq of records_crypt_dev)"""
        return cls(5, 8, 0, TXNUM_WHOLE)

    @classmethod
    def dtls12(cls):
        """RFC 6347 / RFC 5288: the record's 48-bit sequence number, and again as the sequence half of the explicit nonce; the epoch bytes are the caller's"""
        return cls(5, 6, 15, TXNUM_WHOLE)

    @classmethod
    def srtcp(cls, mki_len=0):
        """RFC 3711 3.4: the 31-bit SRTCP index behind the tag, in front of the MKI; the E bit stays as the caller set it"""
        return cls(4 + mki_len, 4, 0, TXNUM_FROM_END | TXNUM_KEEP_TOP | TXNUM_WHOLE)

    @classmethod
    def number_only(cls):
        """TLS 1.3, QUIC, DTLS 1.3: nums = the d_seq / d_pn of their calls, which place their own bytes; no packet byte is written"""
        return cls(0, 0, 0, 0)


class TxCounters(_Table):
    """aesgcm_txnum: n_ctrs device-resident send counters (next, limit); assign_dev hands the packets of a call their numbers in array order and writes them into the
    packets, before the encrypt call (include/aesgcm.h "SEND COUNTERS").  max_pkts = the largest call."""
    _prefix = "aesgcm_txnum"

    def __init__(self, n_ctrs, max_pkts, device=0):
        self._create(_txnum_typed, device, n_ctrs, max_pkts)
        self.n_ctrs, self.max_pkts = n_ctrs, max_pkts

    def set(self, first, nexts, limits, stream=None):
        """aesgcm_txnum_set: counters first, first + 1, ... get next = nexts[k] and limit = limits[k] (exclusive)"""
        n = len(nexts)
        if len(limits) != n:
            raise AesGcmError(EARG, "one limit per next")
        _chk(self._lib.aesgcm_txnum_set(self._h, first, n, (u64 * max(n, 1))(*nexts), (u64 * max(n, 1))(*limits), stream))
        return self

    def get(self, first=0, n=None, stream=None):
        """aesgcm_txnum_get -> (nexts, limits) of counters first .. first + n - 1; waits on the stream"""
        n = self.n_ctrs - first if n is None else n
        nx, lm = (u64 * max(n, 1))(), (u64 * max(n, 1))()
        _chk(self._lib.aesgcm_txnum_get(self._h, first, n, nx, lm, stream))
        return list(nx[:n]), list(lm[:n])

    def assign_dev(self, fmt, n_pkts, d_ctr, d_pkts, d_pkt_off, d_num_out, d_hi_out=None, d_slots=None, stream=None):
        """aesgcm_txnum_assign_dev: d_num_out[p] (uint64) = packet p's number from counter d_ctr[p] (uint32), in array order per counter; d_hi_out[p] (uint32, optional)
        = its upper half; fmt (a TxFormat) says which bytes of the packet get it (TxFormat.number_only(): d_pkts and d_pkt_off may be None); d_slots[p] (uint32,
        optional, in/out, never the array d_ctr) = 0xFFFFFFFF for a refused packet"""
        _chk(self._lib.aesgcm_txnum_assign_dev(self._h, ctypes.byref(fmt), n_pkts, d_ctr, d_pkts, d_pkt_off, d_num_out, d_hi_out, d_slots, stream))

    def assign(self, fmt, ctrs, packets=None):
        """Host convenience (tests, examples): -> (packets, nums, his, refused) of whole packets (TxFormat.number_only(): packets may be None and come back as None);
        refused[p] = the packet was refused"""
        n = len(ctrs)
        if not n or (packets is not None and len(packets) != n):
            raise AesGcmError(EARG, "ctrs and packets must be equally long and not empty")
        up, down = {"ctr": ("I", ctrs), "slots": ("I", [0] * n)}, {"num": ("Q", n), "hi": ("I", n), "slots": ("I", n)}
        off = None
        if packets is not None:
            data, off = _joined(packets)
            up.update(data=data, off=("Q", off))
            down.update(data=("%ds" % off[n], 1))
        got = _device_call(self.device, up, down,
                           lambda b: self.assign_dev(fmt, n, b["ctr"].ptr, b["data"].ptr if packets is not None else None, b["off"].ptr if packets is not None else None,
                                                     b["num"].ptr, b["hi"].ptr, b["slots"].ptr))
        out = None if packets is None else [got["data"][0][off[p]:off[p + 1]] for p in range(n)]
        return out, got["num"], got["hi"], [s == 0xFFFFFFFF for s in got["slots"]]


# ---------------------------------------------------------------- on-device key derivation (aesgcm_kdf_*)
def _kdf_typed(L):
    """type the aesgcm_kdf_* symbols on first use, as _txnum_typed does: the fake runtime of tests/fake_hip links no such unit and still loads"""
    if not getattr(L, "_kdf_typed", False):
        L.aesgcm_kdf_create.argtypes = [ctypes.POINTER(vp), cint, sz, sz]
        L.aesgcm_kdf_set.argtypes = [vp, sz, sz, vp, vp]
        L.aesgcm_kdf_set_dev.argtypes = [vp, sz, vp, vp, vp]
        L.aesgcm_kdf_clear.argtypes = [vp, sz, sz, vp]
        L.aesgcm_kdf_fmt_check.argtypes = [ctypes.POINTER(KdfFormat)]
        L.aesgcm_kdf_install_dev.argtypes = [vp, ctypes.POINTER(KdfFormat), vp, sz, vp, vp, vp, vp]
        L.aesgcm_kdf_update_dev.argtypes = [vp, ctypes.POINTER(KdfFormat), sz, vp, vp, vp]
        L.aesgcm_kdf_status.argtypes = [vp, ctypes.POINTER(cint), ctypes.POINTER(u64)]
        L.aesgcm_kdf_destroy.argtypes = [vp]
        L._kdf_typed = True
    return L


KDF_LABEL_MAX = 20                                                  # bytes of a full label: the bound under which an HMAC is four compressions
KDF_NO_SLOT = 0xFFFFFFFF                                            # an entry of d_aux_slots that installs no auxiliary key


class KdfFormat(_Format, ctypes.Structure):
    """aesgcm_kdf_fmt: the four HKDF-Expand-Label labels of a protocol in full, prefix included -- 0 key, 1 iv, 2 aux (QUIC hp / DTLS 1.3 sn), 3 update; len 0 = absent
    (include/aesgcm.h "ON-DEVICE KEY DERIVATION")"""
    _fields_ = [("len", ctypes.c_uint8 * 4), ("label", (ctypes.c_uint8 * 20) * 4)]
    _check, _typed = "aesgcm_kdf_fmt_check", staticmethod(_kdf_typed)

    @classmethod
    def custom(cls, key, iv=b"", aux=b"", update=b""):
        """full labels as bytes (b"" or None = absent).  A label longer than 20 bytes keeps its length and its first 20 bytes: check() refuses it"""
        f = cls()
        for j, lab in enumerate((key, iv, aux, update)):
            lab = bytes(lab or b"")
            if len(lab) > 255:
                raise AesGcmError(EARG, "a label's length is one byte")
            f.len[j] = len(lab)
            for i, c in enumerate(lab[:KDF_LABEL_MAX]):
                f.label[j][i] = c
        return f

    def labels(self):
        """-> the four labels as bytes (b"" = absent)"""
        return tuple(bytes(self.label[j][:min(self.len[j], KDF_LABEL_MAX)]) for j in range(4))

    def __repr__(self):
        return "KdfFormat(%s)" % ", ".join(repr(x) for x in self.labels())

    @classmethod
    def tls13(cls):
        """RFC 8446 7.3 (key, iv) and 7.2 (traffic upd); TLS has no auxiliary key"""
        return cls.custom(b"tls13 key", b"tls13 iv", None, b"tls13 traffic upd")

    @classmethod
    def quic_v1(cls):
        """RFC 9001 5.1 (quic key, quic iv, quic hp) and 6.1 (quic ku)"""
        return cls.custom(b"tls13 quic key", b"tls13 quic iv", b"tls13 quic hp", b"tls13 quic ku")

    @classmethod
    def quic_v2(cls):
        """RFC 9369 3.3.2: quicv2 key, quicv2 iv, quicv2 hp, quicv2 ku"""
        return cls.custom(b"tls13 quicv2 key", b"tls13 quicv2 iv", b"tls13 quicv2 hp", b"tls13 quicv2 ku")

    @classmethod
    def dtls13(cls):
        """RFC 9147 5.9: the prefix is "dtls13" with no blank; key, iv, sn (4.2.3) and traffic upd (RFC 8446 7.2 under that prefix)"""
        return cls.custom(b"dtls13key", b"dtls13iv", b"dtls13sn", b"dtls13traffic upd")


class SecretTable(_Table):
    """aesgcm_kdf: n_secrets device-resident traffic secrets of one hash (hash_len 32 = SHA-256, 48 = SHA-384).  install_dev derives key, IV and auxiliary key of a
    secret into key-table slots, update_dev steps a secret to its next generation; no secret is ever read back (include/aesgcm.h "ON-DEVICE KEY DERIVATION").  Protect
    the table like keys."""
    _prefix = "aesgcm_kdf"

    def __init__(self, hash_len, n_secrets, device=0):
        self._create(_kdf_typed, device, hash_len, n_secrets)
        self.hash_len, self.n_secrets = hash_len, n_secrets

    def set(self, first, secrets, stream=None):
        """aesgcm_kdf_set: host secrets (one bytes-like of n * hash_len bytes, or a list of secrets) into records first, first + 1, ..."""
        sb, n = _per_slot(secrets, self.hash_len, "secrets must be a multiple of %d bytes" % self.hash_len)
        _chk(self._lib.aesgcm_kdf_set(self._h, first, n, sb, stream))
        return self

    def set_dev(self, n, d_idx, d_secrets, stream=None):
        """aesgcm_kdf_set_dev: n secrets from device memory (n x hash_len bytes) into the records d_idx (n uint32, device memory)"""
        _chk(self._lib.aesgcm_kdf_set_dev(self._h, n, d_idx, d_secrets, stream))
        return self

    def clear(self, first, n=1, stream=None):
        """aesgcm_kdf_clear: records first .. first + n - 1 zeroed and unset (their entries are refused)"""
        _chk(self._lib.aesgcm_kdf_clear(self._h, first, n, stream))
        return self

    def install_dev(self, fmt, keytab, n, d_idx, d_slots, d_aux_slots=None, stream=None):
        """aesgcm_kdf_install_dev: entry i derives key and IV of record d_idx[i] into slot d_slots[i] of keytab (a KeyTable), and the auxiliary key into slot
        d_aux_slots[i] where that array is given and the entry is not KDF_NO_SLOT (all uint32, device memory)"""
        _chk(self._lib.aesgcm_kdf_install_dev(self._h, ctypes.byref(fmt), keytab._h, n, d_idx, d_slots, d_aux_slots, stream))

    def update_dev(self, fmt, n, d_from, d_to, stream=None):
        """aesgcm_kdf_update_dev: record d_to[i] = the next generation of record d_from[i] (uint32, device memory; d_to[i] == d_from[i]: in place)"""
        _chk(self._lib.aesgcm_kdf_update_dev(self._h, ctypes.byref(fmt), n, d_from, d_to, stream))

    def install(self, fmt, keytab, idx, slots, aux_slots=None):
        """Host convenience (tests, examples): install_dev over host lists, waited for"""
        n = len(idx)
        if not n or len(slots) != n or (aux_slots is not None and len(aux_slots) != n):
            raise AesGcmError(EARG, "idx, slots and aux_slots must be equally long and not empty")
        up = {"idx": ("I", idx), "slots": ("I", slots)}
        if aux_slots is not None:
            up["aux"] = ("I", aux_slots)
        _device_call(self.device, up, {}, lambda b: self.install_dev(fmt, keytab, n, b["idx"].ptr, b["slots"].ptr, b["aux"].ptr if aux_slots is not None else None))
        return self

    def update(self, fmt, frm, to):
        """Host convenience (tests, examples): update_dev over host lists, waited for"""
        n = len(frm)
        if not n or len(to) != n:
            raise AesGcmError(EARG, "frm and to must be equally long and not empty")
        _device_call(self.device, {"frm": ("I", frm), "to": ("I", to)}, {}, lambda b: self.update_dev(fmt, n, b["frm"].ptr, b["to"].ptr))
        return self


# ---------------------------------------------------------------- SRTP's on-device key derivation (aesgcm_srtp_kdf_*)
def _srtp_kdf_typed(L):
    """type the aesgcm_srtp_kdf_* symbols on first use, as _kdf_typed does: the fake runtime of tests/fake_hip links no such unit and still loads"""
    if not getattr(L, "_srtp_kdf_typed", False):
        L.aesgcm_srtp_kdf_create.argtypes = [ctypes.POINTER(vp), cint, sz, sz]
        L.aesgcm_srtp_kdf_set.argtypes = [vp, sz, sz, vp, vp, vp]
        L.aesgcm_srtp_kdf_set_dev.argtypes = [vp, sz, vp, vp, vp, vp]
        L.aesgcm_srtp_kdf_clear.argtypes = [vp, sz, sz, vp]
        L.aesgcm_srtp_kdf_install_dev.argtypes = [vp, ctypes.c_uint32, vp, sz, vp, vp, vp, vp]
        L.aesgcm_srtp_kdf_status.argtypes = [vp, ctypes.POINTER(cint), ctypes.POINTER(u64)]
        L.aesgcm_srtp_kdf_destroy.argtypes = [vp]
        L._srtp_kdf_typed = True
    return L


SRTP_MASTER_SALT_LEN = 14                                           # bytes of a master salt in the C ABI; an AEAD profile's 12 are padded on the right


class MasterKeyTable(_Table):
    """aesgcm_srtp_kdf: n_masters device-resident SRTP master keys (key_len 16 / 24 / 32) and master salts.  install_dev derives a master's SRTP or SRTCP session key
    and session salt (RFC 3711 4.3.1, RFC 6188; labels 0x00 / 0x02 and 0x03 / 0x05) into key-table slots; no master is ever read back (include/aesgcm.h "SRTP KEY
    DERIVATION").  Protect the table like keys."""
    _prefix = "aesgcm_srtp_kdf"

    def __init__(self, key_len, n_masters, device=0):
        self._create(_srtp_kdf_typed, device, key_len, n_masters)
        self.key_len, self.n_masters = key_len, n_masters

    def set(self, first, keys, salts, stream=None):
        """aesgcm_srtp_kdf_set: host master keys (one bytes-like of n * key_len bytes, or a list) and master salts (a list of 12- or 14-byte salts, a 12-byte one
        padded with two zero bytes on the right as RFC 7714 11 enters it into the PRF; or one bytes-like of n * 14 bytes) into records first, first + 1, ..."""
        kb, n = _per_slot(keys, self.key_len, "master keys must be a multiple of %d bytes" % self.key_len)
        what = "a master salt is 12 or 14 bytes, one per master key"
        if isinstance(salts, (list, tuple)) and any(len(x) not in (12, SRTP_MASTER_SALT_LEN) for x in salts):
            raise AesGcmError(EARG, what)
        sb, ns = _per_slot(salts, SRTP_MASTER_SALT_LEN, what, pad=True)
        if ns != n:
            raise AesGcmError(EARG, what)
        _chk(self._lib.aesgcm_srtp_kdf_set(self._h, first, n, kb, sb, stream))
        return self

    def set_dev(self, n, d_idx, d_keys, d_salts, stream=None):
        """aesgcm_srtp_kdf_set_dev: n master keys (n x key_len bytes) and salts (n x 14 bytes) from device memory into the records d_idx (n uint32, device memory)"""
        _chk(self._lib.aesgcm_srtp_kdf_set_dev(self._h, n, d_idx, d_keys, d_salts, stream))
        return self

    def clear(self, first, n=1, stream=None):
        """aesgcm_srtp_kdf_clear: records first .. first + n - 1 zeroed and unset (their entries are refused)"""
        _chk(self._lib.aesgcm_srtp_kdf_clear(self._h, first, n, stream))
        return self

    def install_dev(self, kind, keytab, n, d_idx, d_slots, d_r=None, stream=None):
        """aesgcm_srtp_kdf_install_dev: entry i derives the session key and salt of record d_idx[i] for kind (SRTP_RTP or SRTP_RTCP) under r = d_r[i] (uint64, device
        memory; None: all 0) into slot d_slots[i] of keytab (a KeyTable of the same key size; d_idx and d_slots uint32, device memory)"""
        _chk(self._lib.aesgcm_srtp_kdf_install_dev(self._h, kind, keytab._h, n, d_idx, d_slots, d_r, stream))

    def install(self, kind, keytab, idx, slots, r=None):
        """Host convenience (tests, examples): install_dev over host lists, waited for.  As SecretTable.install: refused entries are what status() reports"""
        n = len(idx)
        if not n or len(slots) != n or (r is not None and len(r) != n):
            raise AesGcmError(EARG, "idx, slots and r must be equally long and not empty")
        up = {"idx": ("I", idx), "slots": ("I", slots)}
        if r is not None:
            up["r"] = ("Q", r)
        _device_call(self.device, up, {}, lambda b: self.install_dev(kind, keytab, n, b["idx"].ptr, b["slots"].ptr, b["r"].ptr if r is not None else None))
        return self


# ---------------------------------------------------------------- the TLS 1.2 PRF on the device (aesgcm_prf12_*)
def _prf12_typed(L):
    """type the aesgcm_prf12_* symbols on first use, as _kdf_typed does: a library that lacks them still loads"""
    if not getattr(L, "_prf12_typed", False):
        L.aesgcm_prf12_create.argtypes = [ctypes.POINTER(vp), cint, sz, sz]
        L.aesgcm_prf12_set.argtypes = [vp, sz, sz, vp, vp, vp, vp]
        L.aesgcm_prf12_set_dev.argtypes = [vp, sz, vp, vp, vp, vp, vp]
        L.aesgcm_prf12_clear.argtypes = [vp, sz, sz, vp]
        L.aesgcm_prf12_install_dev.argtypes = [vp, vp, sz, vp, vp, vp, vp]
        L.aesgcm_prf12_export_srtp_dev.argtypes = [vp, vp, sz, vp, vp, vp, vp]
        L.aesgcm_prf12_status.argtypes = [vp, ctypes.POINTER(cint), ctypes.POINTER(u64)]
        L.aesgcm_prf12_destroy.argtypes = [vp]
        L._prf12_typed = True
    return L


PRF12_MASTER_LEN, PRF12_RANDOM_LEN = 48, 32                         # bytes of a master secret and of a hello random
PRF12_NONE = 0xFFFFFFFF                                             # an entry of a slot / record array that installs nothing for that direction


class MasterSecretTable(_Table):
    """aesgcm_prf12: n_masters device-resident TLS 1.2 / DTLS 1.2 master secrets with their client and server randoms, of one PRF hash (hash_len 32 = SHA-256, 48 =
    SHA-384).  install_dev cuts a connection's AES-GCM key block (RFC 5246 6.3) into key-table slots, export_srtp_dev the DTLS-SRTP exporter's output (RFC 5764 4.2)
    into a MasterKeyTable; no record is ever read back (include/aesgcm.h "TLS 1.2 PRF").  Protect the table like keys."""
    _prefix = "aesgcm_prf12"

    def __init__(self, hash_len, n_masters, device=0):
        self._create(_prf12_typed, device, hash_len, n_masters)
        self.hash_len, self.n_masters = hash_len, n_masters

    def set(self, first, masters, client_randoms, server_randoms, stream=None):
        """aesgcm_prf12_set: host master secrets (one bytes-like of n * 48 bytes, or a list) and the connections' randoms (n * 32 bytes each, or lists) into records
        first, first + 1, ..."""
        mb, n = _per_slot(masters, PRF12_MASTER_LEN, "master secrets must be a multiple of 48 bytes")
        what = "a random is 32 bytes, one client random and one server random per master secret"
        cb, nc = _per_slot(client_randoms, PRF12_RANDOM_LEN, what)
        sb, ns = _per_slot(server_randoms, PRF12_RANDOM_LEN, what)
        if nc != n or ns != n:
            raise AesGcmError(EARG, what)
        _chk(self._lib.aesgcm_prf12_set(self._h, first, n, mb, cb, sb, stream))
        return self

    def set_dev(self, n, d_idx, d_masters, d_client_randoms, d_server_randoms, stream=None):
        """aesgcm_prf12_set_dev: n master secrets (n x 48 bytes) and randoms (n x 32 bytes each) from device memory into the records d_idx (n uint32, device memory)"""
        _chk(self._lib.aesgcm_prf12_set_dev(self._h, n, d_idx, d_masters, d_client_randoms, d_server_randoms, stream))
        return self

    def clear(self, first, n=1, stream=None):
        """aesgcm_prf12_clear: records first .. first + n - 1 zeroed and unset (their entries are refused)"""
        _chk(self._lib.aesgcm_prf12_clear(self._h, first, n, stream))
        return self

    def install_dev(self, keytab, n, d_idx, d_client_slots, d_server_slots, stream=None):
        """aesgcm_prf12_install_dev: entry i cuts the key block of record d_idx[i] into slot d_client_slots[i] (client_write_key, client_write_IV) and slot
        d_server_slots[i] (the server's) of keytab (a KeyTable); either array may be None, an entry PRF12_NONE installs nothing (all uint32, device memory)"""
        _chk(self._lib.aesgcm_prf12_install_dev(self._h, keytab._h, n, d_idx, d_client_slots, d_server_slots, stream))

    def export_srtp_dev(self, master_table, n, d_idx, d_client_recs, d_server_recs, stream=None):
        """aesgcm_prf12_export_srtp_dev: entry i writes the DTLS-SRTP exporter's client key and salt of record d_idx[i] into record d_client_recs[i] of master_table
        (a MasterKeyTable of key_len 16 or 32) and the server's into d_server_recs[i]; None and PRF12_NONE as install_dev"""
        _chk(self._lib.aesgcm_prf12_export_srtp_dev(self._h, master_table._h, n, d_idx, d_client_recs, d_server_recs, stream))

    def _both(self, idx, a, b, call):
        n = len(idx)
        if not n or (a is None and b is None) or any(x is not None and len(x) != n for x in (a, b)):
            raise AesGcmError(EARG, "idx and the client / server arrays (at least one) must be equally long and not empty")
        up = {"idx": ("I", idx)}
        if a is not None:
            up["c"] = ("I", a)
        if b is not None:
            up["s"] = ("I", b)
        _device_call(self.device, up, {}, lambda m: call(n, m["idx"].ptr, m["c"].ptr if a is not None else None, m["s"].ptr if b is not None else None))
        return self

    def install(self, keytab, idx, client_slots, server_slots):
        """Host convenience (tests, examples): install_dev over host lists, waited for.  Refused entries are what status() reports"""
        return self._both(idx, client_slots, server_slots, lambda n, i, c, s: self.install_dev(keytab, n, i, c, s))

    def export_srtp(self, master_table, idx, client_recs, server_recs):
        """Host convenience (tests, examples): export_srtp_dev over host lists, waited for"""
        return self._both(idx, client_recs, server_recs, lambda n, i, c, s: self.export_srtp_dev(master_table, n, i, c, s))


# ---------------------------------------------------------------- IKEv2's prf+ on the device (aesgcm_prfplus_*)
def _prfplus_typed(L):
    """type the aesgcm_prfplus_* symbols on first use, as _kdf_typed does: a library that lacks them still loads"""
    if not getattr(L, "_prfplus_typed", False):
        L.aesgcm_prfplus_create.argtypes = [ctypes.POINTER(vp), cint, sz, sz]
        L.aesgcm_prfplus_set.argtypes = [vp, sz, sz, vp, vp]
        L.aesgcm_prfplus_set_dev.argtypes = [vp, sz, vp, vp, vp]
        L.aesgcm_prfplus_clear.argtypes = [vp, sz, sz, vp]
        L.aesgcm_prfplus_install_dev.argtypes = [vp, vp, sz, vp, vp, vp, vp, vp, vp]
        L.aesgcm_prfplus_status.argtypes = [vp, ctypes.POINTER(cint), ctypes.POINTER(u64)]
        L.aesgcm_prfplus_destroy.argtypes = [vp]
        L._prfplus_typed = True
    return L


PRFP_SEED_MAX = 2048                                                # bytes of the longest seed an install entry may name
PRFP_NONE = 0xFFFFFFFF                                              # an entry of a slot array that installs nothing for that direction


class IkeSaTable(_Table):
    """aesgcm_prfplus: n_keys device-resident SK_d values of IKE SAs, of one prf (hash_len 32 = HMAC-SHA-256, 48 = -384, 64 = -512).  install_dev cuts the ESP AES-GCM
    keying material of Child SAs, prf+(SK_d, seed) of RFC 7296 2.13 / 2.17, into key-table slots: key and four salt bytes per direction; no SK_d is ever read back
    (include/aesgcm.h "IKEv2 PRF+").  Protect the table like keys."""
    _prefix = "aesgcm_prfplus"

    def __init__(self, hash_len, n_keys, device=0):
        self._create(_prfplus_typed, device, hash_len, n_keys)
        self.hash_len, self.n_keys = hash_len, n_keys

    def set(self, first, keys, stream=None):
        """aesgcm_prfplus_set: host SK_d values (one bytes-like of n * hash_len bytes, or a list) into records first, first + 1, ..."""
        kb, n = _per_slot(keys, self.hash_len, "SK_d values must be a multiple of %d bytes" % self.hash_len)
        _chk(self._lib.aesgcm_prfplus_set(self._h, first, n, kb, stream))
        return self

    def set_dev(self, n, d_idx, d_keys, stream=None):
        """aesgcm_prfplus_set_dev: n SK_d values from device memory (n x hash_len bytes) into the records d_idx (n uint32, device memory)"""
        _chk(self._lib.aesgcm_prfplus_set_dev(self._h, n, d_idx, d_keys, stream))
        return self

    def clear(self, first, n=1, stream=None):
        """aesgcm_prfplus_clear: records first .. first + n - 1 zeroed and unset (their entries are refused)"""
        _chk(self._lib.aesgcm_prfplus_clear(self._h, first, n, stream))
        return self

    def install_dev(self, keytab, n, d_idx, d_seed, d_seed_off, d_i2r_slots, d_r2i_slots, stream=None):
        """aesgcm_prfplus_install_dev: entry i derives KEYMAT = prf+(record d_idx[i], seed i) with seed i = bytes [d_seed_off[i], d_seed_off[i + 1]) of d_seed, and
        installs key_i2r | salt_i2r into slot d_i2r_slots[i] and key_r2i | salt_r2i into slot d_r2i_slots[i] of keytab (a KeyTable); either slot array may be None,
        an entry PRFP_NONE installs nothing (d_idx, d_seed_off and the slots uint32, all device memory)"""
        _chk(self._lib.aesgcm_prfplus_install_dev(self._h, keytab._h, n, d_idx, d_seed, d_seed_off, d_i2r_slots, d_r2i_slots, stream))

    def install(self, keytab, idx, seeds, i2r_slots=None, r2i_slots=None, stream=None):
        """Host convenience (tests, examples): install_dev over host lists, waited for; seeds is a list of bytes, packed side by side here.  Refused entries are what
        status() reports"""
        n = len(idx)
        if not n or len(seeds) != n or (i2r_slots is None and r2i_slots is None) or any(x is not None and len(x) != n for x in (i2r_slots, r2i_slots)):
            raise AesGcmError(EARG, "idx, seeds and the i2r / r2i slot arrays (at least one) must be equally long and not empty")
        packed, off = _joined(seeds)
        if off[-1] >= 1 << 32:
            raise AesGcmError(EARG, "the seeds' offsets are 32-bit")
        up = {"idx": ("I", idx), "seed": packed, "off": ("I", off)}
        if i2r_slots is not None:
            up["i2r"] = ("I", i2r_slots)
        if r2i_slots is not None:
            up["r2i"] = ("I", r2i_slots)
        _device_call(self.device, up, {}, lambda b: self.install_dev(keytab, n, b["idx"].ptr, b["seed"].ptr, b["off"].ptr, b["i2r"].ptr if i2r_slots is not None else None,
                                                                     b["r2i"].ptr if r2i_slots is not None else None, stream))
        return self


# ---------------------------------------------------------------- MACsec's MKA on the device (aesgcm_mka_*)
def _mka_typed(L):
    """type the aesgcm_mka_* symbols on first use, as _kdf_typed does: a library that lacks them still loads"""
    if not getattr(L, "_mka_typed", False):
        L.aesgcm_mka_create.argtypes = [ctypes.POINTER(vp), cint, sz, sz]
        L.aesgcm_mka_set.argtypes = [vp, sz, sz, vp, vp, vp]
        L.aesgcm_mka_set_dev.argtypes = [vp, sz, vp, vp, vp, vp]
        L.aesgcm_mka_clear.argtypes = [vp, sz, sz, vp]
        L.aesgcm_mka_install_dev.argtypes = [vp, vp, sz, vp, vp, vp, vp, vp, vp]
        L.aesgcm_mka_unwrap_dev.argtypes = [vp, vp, sz, vp, vp, vp, vp, vp]
        L.aesgcm_mka_status.argtypes = [vp, ctypes.POINTER(cint), ctypes.POINTER(u64)]
        L.aesgcm_mka_destroy.argtypes = [vp]
        L._mka_typed = True
    return L


MKA_CTX_MAX = 2048                                                  # bytes of the longest context an install entry may name
MKA_KEYID_LEN = 16                                                  # bytes of a Keyid in the C ABI: the CKN's first 16, zero-padded on the right
MKA_INSTALLED, MKA_REFUSED, MKA_BAD_ICV = 0, 1, 2                   # an unwrap entry's verdict byte


def mka_sak_context(ks_nonce, mis, kn):
    """the SAK's KDF context of IEEE 802.1X-2010 9.8.1: KS-nonce | MI-value list | be32(KN) -- the key server's nonce (of the SAK's length), the 12-byte member
    identifiers of the live peers in the order the standard gives them, and the key number"""
    if any(len(mi) != 12 for mi in mis) or not 0 <= kn < 1 << 32:
        raise AesGcmError(EARG, "a member identifier is 12 bytes, a key number 32 bits")
    return bytes(ks_nonce) + b"".join(bytes(mi) for mi in mis) + struct.pack(">I", kn)


class CakTable(_Table):
    """aesgcm_mka: n_caks device-resident MACsec CAKs (cak_len 16 / 32) with their Keyids.  install_dev (the key server) derives SAKs by the AES-CMAC KDF of IEEE
    802.1X-2010 6.2 into key-table slots and, if asked, emits them wrapped under the KEK (RFC 3394); unwrap_dev (any other station) turns a received wrapped SAK into a
    slot or refuses it; no CAK is ever read back (include/aesgcm.h "MACSEC MKA").  Protect the table like keys."""
    _prefix = "aesgcm_mka"

    def __init__(self, cak_len, n_caks, device=0):
        self._create(_mka_typed, device, cak_len, n_caks)
        self.cak_len, self.n_caks = cak_len, n_caks

    def set(self, first, caks, ckns, stream=None):
        """aesgcm_mka_set: host CAKs (one bytes-like of n * cak_len bytes, or a list) and their CKNs (a list, 1 .. 32 bytes each: the Keyid is formed here) into
        records first, first + 1, ..."""
        kb, n = _per_slot(caks, self.cak_len, "CAKs must be a multiple of %d bytes" % self.cak_len)
        if not isinstance(ckns, (list, tuple)) or len(ckns) != n or any(not 1 <= len(c) <= 32 for c in ckns):
            raise AesGcmError(EARG, "a CKN is 1 to 32 bytes, one per CAK")
        ib = b"".join(bytes(c)[:MKA_KEYID_LEN].ljust(MKA_KEYID_LEN, b"\0") for c in ckns)
        _chk(self._lib.aesgcm_mka_set(self._h, first, n, kb, ib, stream))
        return self

    def set_dev(self, n, d_idx, d_caks, d_keyids, stream=None):
        """aesgcm_mka_set_dev: n CAKs (n x cak_len bytes) and Keyids (n x 16 bytes) from device memory into the records d_idx (n uint32, device memory)"""
        _chk(self._lib.aesgcm_mka_set_dev(self._h, n, d_idx, d_caks, d_keyids, stream))
        return self

    def clear(self, first, n=1, stream=None):
        """aesgcm_mka_clear: records first .. first + n - 1 zeroed and unset (their entries are refused)"""
        _chk(self._lib.aesgcm_mka_clear(self._h, first, n, stream))
        return self

    def install_dev(self, keytab, n, d_idx, d_ctx, d_ctx_off, d_slots, d_wrapped=None, stream=None):
        """aesgcm_mka_install_dev: entry i derives SAK = KDF(record d_idx[i], "IEEE8021 SAK", context i) with context i = bytes [d_ctx_off[i], d_ctx_off[i + 1]) of
        d_ctx into slot d_slots[i] of keytab (a KeyTable of key_len 16 or 32) and, where d_wrapped is not None, its key_len + 8 wrapped bytes to d_wrapped + i *
        (key_len + 8) (d_idx, d_ctx_off and d_slots uint32, all device memory)"""
        _chk(self._lib.aesgcm_mka_install_dev(self._h, keytab._h, n, d_idx, d_ctx, d_ctx_off, d_slots, d_wrapped, stream))

    def unwrap_dev(self, keytab, n, d_idx, d_wrapped, d_slots, d_verdict=None, stream=None):
        """aesgcm_mka_unwrap_dev: entry i unwraps the key_len + 8 bytes at d_wrapped + i * (key_len + 8) under the KEK of record d_idx[i] into slot d_slots[i] of
        keytab, or refuses; d_verdict (n bytes, device memory, or None) gets MKA_INSTALLED, MKA_REFUSED or MKA_BAD_ICV per entry"""
        _chk(self._lib.aesgcm_mka_unwrap_dev(self._h, keytab._h, n, d_idx, d_wrapped, d_slots, d_verdict, stream))

    def install(self, keytab, idx, contexts, slots, wrapped=False, stream=None):
        """Host convenience (tests, examples): install_dev over host lists, waited for; contexts is a list of bytes, packed side by side here.  -> the list of wrapped
        SAKs where wrapped is true (a refused entry's bytes are what the buffer held: zeros), else self.  Refused entries are what status() reports"""
        n = len(idx)
        if not n or len(contexts) != n or len(slots) != n:
            raise AesGcmError(EARG, "idx, contexts and slots must be equally long and not empty")
        packed, off = _joined(contexts)
        if off[-1] >= 1 << 32:
            raise AesGcmError(EARG, "the contexts' offsets are 32-bit")
        w = keytab.key_len + 8
        up = {"idx": ("I", idx), "ctx": packed, "off": ("I", off), "slots": ("I", slots)}
        if wrapped:
            up["wrapped"] = bytes(n * w)
        got = _device_call(self.device, up, {"wrapped": ("%ds" % w, n)} if wrapped else {},
                           lambda b: self.install_dev(keytab, n, b["idx"].ptr, b["ctx"].ptr, b["off"].ptr, b["slots"].ptr, b["wrapped"].ptr if wrapped else None, stream))
        return got["wrapped"] if wrapped else self

    def unwrap(self, keytab, idx, wrapped, slots, stream=None):
        """Host convenience (tests, examples): unwrap_dev over host lists, waited for; wrapped is a list of key_len + 8 bytes each.  -> the list of verdicts"""
        n = len(idx)
        if not n or len(wrapped) != n or len(slots) != n or any(len(x) != keytab.key_len + 8 for x in wrapped):
            raise AesGcmError(EARG, "idx, wrapped and slots must be equally long and not empty, a wrapped SAK key_len + 8 bytes")
        got = _device_call(self.device, {"idx": ("I", idx), "wrapped": b"".join(bytes(x) for x in wrapped), "slots": ("I", slots), "verdict": b"\xff" * n}, {"verdict": ("B", n)},
                           lambda b: self.unwrap_dev(keytab, n, b["idx"].ptr, b["wrapped"].ptr, b["slots"].ptr, b["verdict"].ptr, stream))
        return got["verdict"]


# ---------------------------------------------------------------- SSH's key derivation on the device (aesgcm_sshkdf_*)
def _sshkdf_typed(L):
    """type the aesgcm_sshkdf_* symbols on first use, as _kdf_typed does: a library that lacks them still loads"""
    if not getattr(L, "_sshkdf_typed", False):
        L.aesgcm_sshkdf_create.argtypes = [ctypes.POINTER(vp), cint, sz, sz, sz]
        L.aesgcm_sshkdf_set.argtypes = [vp, sz, sz, vp, vp, vp, vp]
        L.aesgcm_sshkdf_set_dev.argtypes = [vp, sz, vp, vp, vp, vp, vp]
        L.aesgcm_sshkdf_clear.argtypes = [vp, sz, sz, vp]
        L.aesgcm_sshkdf_install_dev.argtypes = [vp, vp, sz, vp, vp, vp, vp]
        L.aesgcm_sshkdf_status.argtypes = [vp, ctypes.POINTER(cint), ctypes.POINTER(u64)]
        L.aesgcm_sshkdf_destroy.argtypes = [vp]
        L._sshkdf_typed = True
    return L


SSHK_SECRET_MAX = 2048                                              # the most that max_secret_len may be
SSHK_NONE = 0xFFFFFFFF                                              # an entry of a slot array that installs nothing for that direction


class SshKexTable(_Table):
    """aesgcm_sshkdf: n_recs device-resident key-exchange outputs of SSH connections -- secret = K_enc | H (K as the exchange encodes it: mpint or string, with its
    length prefix) and the session identifier --, of one hash (hash_len 32 = SHA-256, 48 = SHA-384, 64 = SHA-512).  install_dev derives the AES-GCM key and the initial
    IV of either direction by RFC 4253 7.2 into key-table slots, which crypt_ssh then uses; no record is ever read back (include/aesgcm.h "SSH KEY DERIVATION").
    Protect the table like keys."""
    _prefix = "aesgcm_sshkdf"

    def __init__(self, hash_len, n_recs, max_secret_len=SSHK_SECRET_MAX, device=0):
        self._create(_sshkdf_typed, device, hash_len, max_secret_len, n_recs)
        self.hash_len, self.n_recs, self.max_secret_len = hash_len, n_recs, max_secret_len

    def set(self, first, secrets, session_ids, stream=None):
        """aesgcm_sshkdf_set: host secrets (a list of bytes, K_enc | H each, 1 .. max_secret_len bytes) and session identifiers (one bytes-like of n * hash_len bytes,
        or a list) into records first, first + 1, ..."""
        sb, n = _per_slot(session_ids, self.hash_len, "a session identifier is %d bytes" % self.hash_len)
        if len(secrets) != n:
            raise AesGcmError(EARG, "one secret and one session identifier per record")
        packed, off = _joined(secrets)
        if off[-1] >= 1 << 32:
            raise AesGcmError(EARG, "the secrets' offsets are 32-bit")
        _chk(self._lib.aesgcm_sshkdf_set(self._h, first, n, packed, struct.pack("<%dI" % (n + 1), *off), sb, stream))
        return self

    def set_dev(self, n, d_idx, d_secrets, d_secret_off, d_session_ids, stream=None):
        """aesgcm_sshkdf_set_dev: n secrets (byte-packed, secret i = bytes [d_secret_off[i], d_secret_off[i + 1]) of d_secrets) and session identifiers (n x hash_len
        bytes) from device memory into the records d_idx (d_idx and d_secret_off uint32, device memory)"""
        _chk(self._lib.aesgcm_sshkdf_set_dev(self._h, n, d_idx, d_secrets, d_secret_off, d_session_ids, stream))
        return self

    def clear(self, first, n=1, stream=None):
        """aesgcm_sshkdf_clear: records first .. first + n - 1 zeroed and unset (their entries are refused)"""
        _chk(self._lib.aesgcm_sshkdf_clear(self._h, first, n, stream))
        return self

    def install_dev(self, keytab, n, d_idx, d_c2s_slots, d_s2c_slots, stream=None):
        """aesgcm_sshkdf_install_dev: entry i derives, from record d_idx[i], key HASH(K | H | "C" | session_id) and IV HASH(K | H | "A" | session_id) into slot
        d_c2s_slots[i] of keytab (a KeyTable) and those of "D" / "B" into slot d_s2c_slots[i]; either slot array may be None, an entry SSHK_NONE installs nothing
        (all uint32, device memory)"""
        _chk(self._lib.aesgcm_sshkdf_install_dev(self._h, keytab._h, n, d_idx, d_c2s_slots, d_s2c_slots, stream))

    def install(self, keytab, idx, c2s_slots=None, s2c_slots=None, stream=None):
        """Host convenience (tests, examples): install_dev over host lists, waited for.  Refused entries are what status() reports"""
        n = len(idx)
        if not n or (c2s_slots is None and s2c_slots is None) or any(x is not None and len(x) != n for x in (c2s_slots, s2c_slots)):
            raise AesGcmError(EARG, "idx and the c2s / s2c slot arrays (at least one) must be equally long and not empty")
        up = {"idx": ("I", idx)}
        if c2s_slots is not None:
            up["c2s"] = ("I", c2s_slots)
        if s2c_slots is not None:
            up["s2c"] = ("I", s2c_slots)
        _device_call(self.device, up, {}, lambda b: self.install_dev(keytab, n, b["idx"].ptr, b["c2s"].ptr if c2s_slots is not None else None,
                                                                     b["s2c"].ptr if s2c_slots is not None else None, stream))
        return self


# ---------------------------------------------------------------- the exchange step (RCCL inside the library)
def comm_unique_id():
    """128-byte RCCL unique id (rank 0 makes it, every rank passes it to Comm)."""
    b = ctypes.create_string_buffer(128)
    _chk(load().aesgcm_comm_unique_id(b))
    return b.raw


class Comm:
    """aesgcm_comm: one rank of an RCCL communicator (ncclCommInitRank), one process per GPU."""

    def __init__(self, unique_id, n_ranks, rank, device=0):
        self._c = None
        c = vp()
        _chk(load().aesgcm_comm_create(ctypes.byref(c), device, _fixed(unique_id, 128, "unique id"), n_ranks, rank))
        self._c = c.value
        n, r = cint(0), cint(0)
        _chk(load().aesgcm_comm_ranks(self._c, ctypes.byref(n), ctypes.byref(r)))
        self.n_ranks, self.rank = n.value, r.value        # what RCCL reports

    def allgather_dev(self, d_send, d_recv, bytes_per_rank, stream=None):
        _chk(load().aesgcm_comm_allgather_dev(self._c, d_send, d_recv, bytes_per_rank, stream))

    def allreduce(self, value, op="max"):
        v = ctypes.c_double(value)
        _chk(load().aesgcm_comm_allreduce_f64(self._c, ctypes.byref(v), {"max": 0, "min": 1, "sum": 2}[op]))
        return v.value

    def barrier(self):
        _chk(load().aesgcm_comm_barrier(self._c))

    def close(self):
        if self._c:
            load().aesgcm_comm_destroy(self._c)
            self._c = None

    __del__ = close


class MultiGpu:
    """aesgcm_mgpu: one process, ndev GPUs (ncclCommInitAll); one message sharded over them."""

    def __init__(self, key, devices):
        self._m = None
        devices = list(devices)
        arr = (cint * len(devices))(*devices)
        m = vp()
        key = bytes(key)
        _chk(load().aesgcm_mgpu_create(ctypes.byref(m), len(devices), arr, key, len(key)))
        self._m, self.devices = m.value, devices
        n = cint(0)
        _chk(load().aesgcm_mgpu_ranks(self._m, ctypes.byref(n)))
        self.n_ranks = n.value                             # communicator size RCCL reports

    def crypt_dev(self, decrypt, iv, d_in, shard_len, d_out, d_aad=None, aad_len=0, want_tag=True):
        """d_in / d_out / shard_len: one entry per device -> tag.  want_tag=False: the message is only enqueued (up to 8 may wait); last_tags() collects"""
        g = len(self.devices)
        if not (len(d_in) == len(d_out) == len(shard_len) == g):
            raise AesGcmError(EARG, "one shard per device")
        pin, pout, ln = (vp * g)(*d_in), (vp * g)(*d_out), (sz * g)(*shard_len)
        tag = ctypes.create_string_buffer(16) if want_tag else None
        _chk(load().aesgcm_mgpu_crypt_dev(self._m, int(bool(decrypt)), _fixed(iv, 12, "iv"), d_aad, aad_len, pin, ln, pout, tag))
        return tag.raw if want_tag else None

    def last_tags(self, n):
        """the tags of the OLDEST n messages still queued (want_tag=False), in the order queued; they leave the queue, the rest stays (one finalize launch on the first device)"""
        t = ctypes.create_string_buffer(16 * n)
        _chk(load().aesgcm_mgpu_last_tags(self._m, n, t))
        return [t.raw[16 * k:16 * k + 16] for k in range(n)]

    def sync(self):
        _chk(load().aesgcm_mgpu_sync(self._m))

    def context(self, g):
        """device g's Context, borrowed from the mgpu object (closing it is a no-op)"""
        c = vp()
        _chk(load().aesgcm_mgpu_ctx(self._m, g, ctypes.byref(c)))
        ctx = Context.__new__(Context)
        ctx._c, ctx.device, ctx._borrowed, ctx._owner, ctx._lib = c.value, self.devices[g], True, self, load()
        return ctx

    def close(self):
        if self._m:
            load().aesgcm_mgpu_destroy(self._m)
            self._m = None

    __del__ = close
