"""Drives the calls that include/aesgcm.h names capture-safe (CAPTURE: key tables, receive windows, send counters' assign, the key derivations' install and update, the TLS 1.2 PRF's install and export;
the five-array batch calls plan their launch as a key table's) through the fake HIP runtime (fakehip.cpp) twice each: an ordinary warm-up call, then the same call while the caller's stream captures.  Asserted per call:
  * nothing a capture cannot carry was done while the stream captured -- no hipMalloc or hipFree, no synchronous copy or memset, no host synchronisation, and no
    stream outside the capture waits on an event the capture recorded (fake_capture_violations: each entry names the HIP call);
  * the captured call launches what the warm-up call launched, line by line of the launch log -- except that a captured call is never ordered by length class: where
    the warm-up's log has the counting sort (k_len_*) and a launch order (the `perm` bit of p=), the captured one has neither;
  * the capture holds the call's operations (the dispenser's memset node and the launches), and ordinary ordered calls afterwards -- one per order slot of the
    device -- raise nothing either and launch what the warm-up did.
Packet counts: 300, and 262 144 where the library's own rule orders AES-128 and AES-256 batches; on the -DAESGCM_DEBUG_KNOBS build 300 with batch_order forced, at 8 and
16 lanes per packet.  The launchers launch nothing, so every array is 16 bytes.  Without AESGCM_LIB it runs itself on libaesgcm_fake.so and on libaesgcm_fake_dbg.so.

    make -C tests/fake_hip -s libaesgcm_fake.so dbg && python tests/fake_hip/capture_drive.py"""
import ctypes
import os
import re
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
if not os.environ.get("AESGCM_LIB"):
    for so in ("libaesgcm_fake.so", "libaesgcm_fake_dbg.so"):
        subprocess.run([sys.executable, os.path.abspath(__file__)], env=dict(os.environ, AESGCM_LIB=os.path.join(HERE, so)), check=True)
    sys.exit(0)

sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import aesgcm_amd  # noqa: E402,F401
from aesgcm_amd import lib  # noqa: E402

lib.load()
F = ctypes.CDLL(os.environ["AESGCM_LIB"])
F.fake_log.restype = ctypes.c_size_t
F.fake_log.argtypes = [ctypes.c_char_p, ctypes.c_size_t]
F.fake_name_stream.argtypes = [ctypes.c_void_p, ctypes.c_char_p]
F.fake_begin_capture.argtypes = F.fake_end_capture.argtypes = [ctypes.c_void_p]
F.fake_end_capture.restype = ctypes.c_long
KNOBS = hasattr(F, "aesgcm_debug_force_shape")
ORDER_SLOTS = 4                                                         # DeviceState::order

bufs = [lib.DeviceBuffer(16) for _ in range(16)]
d_slots, d_ivs, d_aad, d_in, d_out, d_tags, d_expect, d_auth, d_off, d_aoff, d_keys, d_num, d_hi, d_hp, d_pn_off, d_why = (b.ptr for b in bufs)
caller_ctx = lib.Context(bytes(32))                                     # its stream is the caller's: a created stream, as a capture needs
caller = caller_ctx.stream()
F.fake_name_stream(caller, b"caller")


def violations():
    out = []
    for read in (F.fake_violations, F.fake_capture_violations):
        b = ctypes.create_string_buffer(1 << 16)
        if read(b, len(b)):
            out += b.value.decode().splitlines()
    return out


def logged(call, capture=False):
    """-> (the call's launch log, the operations the capture holds or None)"""
    F.fake_reset()
    held = None
    if capture:
        assert F.fake_begin_capture(caller) == 0
    try:
        call()
    finally:
        if capture:
            held = F.fake_end_capture(caller)
    b = ctypes.create_string_buffer(1 << 16)
    assert F.fake_log(b, len(b)) <= len(b)
    return b.value.decode().splitlines(), held


def in_array_order(log):
    """what a call's log becomes when its launch is not ordered: no counting sort, and p='s twelfth pointer (perm) unset in the launches that had it"""
    out = []
    for line in log:
        if line.startswith("k_len_* "):
            continue
        out.append(re.sub(r" p=([01]{11})1\b", r" p=\g<1>0", line))
    return out


def calls(kt, rw, tx, sec, mk, ms, n, key_len):
    """every device call of the families, by name; all on the caller's stream"""
    W, X, T, D, S, R = lib.WireFormat, lib.WireFormatX, lib.TlsFormat, lib.DtlsFormat, lib.SrtpFormat, lib.RxFormat
    c = {}
    for dec in (0, 1):
        a = d_auth if dec else None
        c["keytab crypt_dev offsets", dec] = lambda dec=dec, a=a: kt.crypt_dev(dec, n, d_slots, d_ivs, d_in, d_off, d_out, d_tags, d_aad=d_aad, d_aad_off=d_aoff,
                                                                               d_expect_tags=d_expect if dec else None, d_auth=a, stream=caller)
        c["frames macsec", dec] = lambda dec=dec, a=a: kt.frames_crypt_dev(dec, W.macsec(), n, d_slots, d_in, d_off, d_out, d_auth=a, stream=caller)
        c["frames_x esn", dec] = lambda dec=dec, a=a: kt.frames_crypt_x_dev(dec, X.esp_esn(16), n, d_slots, d_hi, d_in, d_off, d_out, d_auth=a, stream=caller)
        c["records tls13", dec] = lambda dec=dec, a=a: kt.records_crypt_dev(dec, T.tls13(), n, d_slots, d_num, d_in, d_off, d_out, d_auth=a, stream=caller)
        c["quic", dec] = lambda dec=dec, a=a: kt.quic_crypt_dev(dec, n, d_slots, d_hp, d_num, d_pn_off, d_in, d_off, d_out, d_pn_out=d_num if dec else None, d_auth=a, stream=caller)
        c["dtls13", dec] = lambda dec=dec, a=a: kt.dtls_crypt_dev(dec, D.dtls13(), n, d_slots, d_in, d_off, d_out, d_sn_slots=d_hp, d_seq=d_num, d_sn_off=d_pn_off,
                                                                  d_seq_out=d_num if dec else None, d_auth=a, stream=caller)
        c["dtls12", dec] = lambda dec=dec, a=a: kt.dtls_crypt_dev(dec, D.dtls12(), n, d_slots, d_in, d_off, d_out, d_auth=a, stream=caller)
        c["srtp rtp", dec] = lambda dec=dec, a=a: kt.srtp_crypt_dev(dec, S.rtp(4), n, d_slots, d_in, d_off, d_out, d_roc=d_hi, d_auth=a, stream=caller)
        c["srtp rtcp", dec] = lambda dec=dec, a=a: kt.srtp_crypt_dev(dec, S.rtcp(), n, d_slots, d_in, d_off, d_out, d_auth=a, stream=caller)
        c["batch five arrays, offsets", dec] = lambda dec=dec, a=a: lib.batch_crypt_var_dev(dec, n, key_len, d_keys, d_ivs, d_in, d_off, d_out, d_tags, d_aad=d_aad, d_aad_off=d_aoff,
                                                                                            d_expect_tags=d_expect if dec else None, d_auth=a, stream=caller)
        c["batch five arrays, fixed", dec] = lambda dec=dec, a=a: lib.batch_crypt_dev(dec, n, key_len, d_keys, d_ivs, d_in, 256, d_out, d_tags, d_expect_tags=d_expect if dec else None,
                                                                                      d_auth=a, stream=caller)
    c["rxwin recover", 1] = lambda: rw.recover_dev(R.esp_esn(), n, d_slots, d_in, d_off, d_num, d_hi, stream=caller)
    c["rxwin recover expect", 1] = lambda: rw.recover_dev(R.expect(), n, d_slots, None, None, d_num, None, stream=caller)
    c["rxwin commit", 1] = lambda: rw.commit_dev(n, d_slots, d_num, d_auth, d_auth, d_why, stream=caller)
    c["txnum assign", 0] = lambda: tx.assign_dev(lib.TxFormat.esp_esn(), n, d_slots, d_in, d_off, d_num, d_hi, stream=caller)
    c["kdf install", 0] = lambda: sec.install_dev(lib.KdfFormat.quic_v1(), kt, n, d_slots, d_hp, d_pn_off, stream=caller)
    c["kdf update", 0] = lambda: sec.update_dev(lib.KdfFormat.tls13(), n, d_slots, d_hp, stream=caller)
    c["srtp_kdf install", 0] = lambda: mk.install_dev(lib.SRTP_RTP, kt, n, d_slots, d_hp, d_num, stream=caller)
    c["prf12 install", 0] = lambda: ms.install_dev(kt, n, d_slots, d_hp, d_pn_off, stream=caller)
    c["prf12 export_srtp", 0] = lambda: ms.export_srtp_dev(mk, n, d_slots, d_hp, d_pn_off, stream=caller)

    def loop():                                                         # the receive loop of INTEGRATION.md: four stream-ordered steps
        rw.recover_dev(R.esp_esn(), n, d_slots, d_in, d_off, d_num, d_hi, stream=caller)
        kt.frames_crypt_x_dev(1, X.esp_esn(16), n, d_slots, d_hi, d_in, d_off, d_out, d_auth=d_auth, stream=caller)
        rw.commit_dev(n, d_slots, d_num, d_auth, d_auth, d_why, stream=caller)
        lib.wipe_failed_dev(n, d_out, d_auth, d_data_off=d_off, stream=caller)
    c["receive loop", 1] = loop
    return c


def drive(n, key_len, want_ordered, label):
    with lib.KeyTable(key_len, 16) as kt, lib.RxWindows(4, 64) as rw, lib.TxCounters(4, n) as tx, lib.SecretTable(32, 4) as sec, lib.MasterKeyTable(key_len, 4) as mk, \
            lib.MasterSecretTable(48, 4) as ms:
        kt.set(0, bytes(key_len * 16))
        F.fake_capture_clear()
        ordered_seen = 0
        for (name, dec), call in calls(kt, rw, tx, sec, mk, ms, n, key_len).items():
            what = "%s, %s %s n=%d AES-%d" % (label, name, "dec" if dec else "enc", n, 8 * key_len)
            warm, _ = logged(call)
            assert warm and not violations(), (what, "the warm-up call", warm, violations())
            ordered = any(line.startswith("k_len_* ") for line in warm)
            ordered_seen += ordered
            got, held = logged(call, capture=True)
            assert not violations(), "%s: under capture\n  %s" % (what, "\n  ".join(violations()))
            want = in_array_order(warm) if ordered else warm
            assert ordered == (want != warm)                            # (the order shows in the log: the sort's line and the perm bit)
            assert got == want, "%s: the captured call launches\n  %s\nand the warm-up call%s\n  %s" % (what, "\n  ".join(got), ", taken in array order," if ordered else "", "\n  ".join(want))
            assert not any(" p=" in line and re.search(r" p=[01]{11}1\b", line) for line in got if line.startswith(("k_kt_", "k_batch3 "))), (what, got)
            batch = sum(line.startswith(("k_kt_batch", "k_kt_wire", "k_kt_tls", "k_kt_quic ", "k_kt_dtls ", "k_kt_srtp", "k_batch3")) for line in got)
            assert held == len(got) + batch, (what, "the capture holds", held, got)      # every launch, and a dispenser's memset node per planned launch
            for k in range(ORDER_SLOTS if ordered else 1):              # ordinary calls afterwards: every order slot comes round
                again, _ = logged(call)
                assert again == warm and not violations(), "%s: ordinary call %d after the capture\n  %s" % (what, k, "\n  ".join(violations() or again))
        assert (ordered_seen > 0) == want_ordered, (label, n, key_len, ordered_seen)
        return ordered_seen


def selftest():
    """the detector: calls that a capture cannot carry, made through the library while the caller's stream captures, are listed by the HIP call's name"""
    def listed(call, capture=True):
        F.fake_capture_clear()
        logged(call, capture=capture)
        b = ctypes.create_string_buffer(1 << 16)
        F.fake_capture_violations(b, len(b))
        return [v.split()[0] for v in b.value.decode().splitlines()]
    with lib.KeyTable(16, 4) as kt, lib.RxWindows(2, 64) as rw, lib.MasterSecretTable(32, 4) as ms:
        kt.set(0, bytes(64))
        clean = lambda: kt.frames_crypt_dev(0, lib.WireFormat.macsec(), 300, d_slots, d_in, d_off, d_out, stream=caller)
        assert listed(clean) == [] and listed(clean, capture=False) == []
        keep = []
        assert listed(lambda: keep.append(lib.DeviceBuffer(16))) == ["hipMalloc"]
        assert listed(lambda: keep[0].upload(bytes(16))) == ["hipMemcpy"]
        assert listed(lambda: keep.pop().free()) == ["hipFree"]
        assert listed(lambda: lib.dev_sync()) == ["hipDeviceSynchronize"]
        assert listed(lambda: rw.get(stream=caller)) == ["hipStreamSynchronize"]
        made = listed(lambda: lib.KeyTable(16, 1).close())
        assert {"hipMalloc", "hipMemset", "hipDeviceSynchronize", "hipFree"} <= set(made), made
        assert listed(lambda: lib.DeviceBuffer(16).free(), capture=False) == []          # ... and none of it outside a capture
        # a setter records the table's staging event: inside a capture that event belongs to the graph, and the next setter's wait from outside is listed -- after
        # the capture has ended
        assert listed(lambda: kt.set(1, bytes(16), stream=caller)) == []
        assert listed(lambda: kt.set(2, bytes(16)), capture=False) == ["hipStreamWaitEvent"]
        assert listed(lambda: kt.set(3, bytes(16)), capture=False) == []                  # (that setter recorded it again, outside)
        ms.set(0, bytes(48), bytes(32), bytes(32))                                        # (the stage and its event are made: an ordinary call before a capture)
        assert listed(lambda: ms.set(1, bytes(48), bytes(32), bytes(32), stream=caller)) == []
        assert listed(lambda: ms.set(2, bytes(48), bytes(32), bytes(32)), capture=False) == ["hipStreamWaitEvent"]
        assert listed(lambda: ms.set(3, bytes(48), bytes(32), bytes(32)), capture=False) == []
    F.fake_capture_clear()
    print("FAKE CAPTURE SELFTEST OK")


if "--selftest" in sys.argv:
    selftest()
    sys.exit(0)

if KNOBS:
    F.aesgcm_debug_force_shape.argtypes = [ctypes.c_char_p, ctypes.c_int]
    total = 0
    for lanes in (8, 16):
        assert F.aesgcm_debug_force_shape(b"batch_lanes", lanes) == 0 and F.aesgcm_debug_force_shape(b"batch_order", 1) == 0
        total += drive(300, (16, 32)[lanes == 16], True, "batch_order forced, %d lanes" % lanes)
    F.aesgcm_debug_force_shape(b"batch_order", 0)
    F.aesgcm_debug_force_shape(b"batch_lanes", 0)
    print("FAKE CAPTURE OK (forced order: %d ordered calls captured in array order)" % total)
else:
    total = 0
    for key_len in (16, 32):
        drive(300, key_len, False, "the library's rules")
        total += drive(262144, key_len, True, "the library's rules")
    print("FAKE CAPTURE OK (%d ordered calls captured in array order)" % total)
