"""Prints what the host side's LAUNCH PLANNERS decide, call by call, from the fake runtime's launch log (fakehip.cpp: fake_log): the packet calls under a context's
key (fixed-size records, routed calls with offset arrays, messages wherever they live, the frames probe) and the per-packet-key batch calls (fixed, variable, the
probe) over a grid that stands on both sides of every threshold of the planners, then -- on the -DAESGCM_DEBUG_KNOBS build -- under every forced shape.  Nothing
runs: every buffer is 16 bytes, the fake device has 256 CUs.  Per call: a `==` line that names it, the log (a line per launch: kernel, stream, scalar arguments, the
parameter struct's scalars, pointers as 0 / 1), an `rc=` line when the call was refused, and `->` with what aesgcm_packets_shape / aesgcm_batch_shape answer for it.

    make -C tests/fake_hip -s libaesgcm_fake.so dbg && python tests/fake_hip/plan_drive.py > tests/golden/launch_plan.txt

Without AESGCM_LIB it runs itself twice, on libaesgcm_fake.so (the library's own rules) and on libaesgcm_fake_dbg.so (the forced shapes), and prints both parts;
tests/test_fake_hip.py compares that with the fixture.  The fixture is taken from the commit BEFORE a change to the planners: equal logs are equal launches."""
import ctypes
import os
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
KNOBS = hasattr(F, "aesgcm_debug_force_shape")
KEYS = {16: bytes(range(16)), 32: bytes(range(32))}

bufs = [lib.DeviceBuffer(16) for _ in range(12)]
d_ivs, d_aad, d_in, d_out, d_tags, d_expect, d_auth, d_off, d_aoff, d_keys, d_len, d_alen = (b.ptr for b in bufs)
# A stream of the caller's: the own stream of a context that lives as long as the driver and makes no call (a context that ends hands its stream to the device's
# next one).  Every other context's own stream is named "own", so the log tells the stream a call was given from the one its context holds; what stays unnamed is
# a stream the library made for itself, and the log calls it "side".
caller_ctx = lib.Context(KEYS[32])
caller = caller_ctx.stream()
F.fake_name_stream(caller, b"caller")


def context(key=32):
    c = lib.Context(KEYS[key])
    assert c.stream() != caller
    F.fake_name_stream(c.stream(), b"own")
    return c


def show(title, call, shape=None):
    """one call: its name, what it launched, how it ended when refused, and the shape query's answer"""
    F.fake_reset()
    print("== " + title)
    try:
        call()
    except lib.AesGcmError as e:
        print("rc=%d" % e.code)
    b = ctypes.create_string_buffer(1 << 16)
    assert F.fake_log(b, len(b)) <= len(b)
    sys.stdout.write(b.value.decode())
    if shape:
        print("-> %d" % shape())


# the crossings of a call: AAD none / 13 bytes, encrypt / decrypt with expected tags and verdicts / the same with wipe_on_auth_fail, output aligned or not
DIR = ("enc", "dec", "wipe")                                            # (wipe: decrypt with the context option wipe_on_auth_fail)
CROSS = [(aad, dec, al) for aad in (0, 13) for dec in (0, 1, 2) for al in (1, 0)]


def packets(n, length, aad=0, dec=0, al=1, ctx=None, opts=(), key=32):
    """aesgcm_packets_crypt_dev with fixed-size records"""
    c = ctx or context(key)
    for o, v in opts:
        c.set_option(o, v)
    c.set_option("wipe_on_auth_fail", int(dec == 2))
    title = "packets %dx%d%s %s%s" % (n, length, " aad" if aad else "", DIR[dec], "" if al else " out+1")
    title += "".join(" %s=%d" % ov for ov in opts) + (" key=%d" % key if key != 32 else "")
    show(title, lambda: c.packets_crypt_dev(dec != 0, n, d_ivs, d_in, d_out + (0 if al else 1), d_tags, pkt_len=length, d_aad=d_aad if aad else None, aad_len=aad,
                                            d_expect_tags=d_expect if dec else None, d_auth=d_auth if dec else None, stream=caller),
         lambda: c.packets_shape(n, length))


def routed(n, aad=False, dec=0, ctx=None):
    """... with offset arrays: every message routed on the device"""
    c = ctx or context()
    c.set_option("wipe_on_auth_fail", int(dec == 2))
    show("routed %d%s %s" % (n, " aad" if aad else "", DIR[dec]),
         lambda: c.packets_crypt_dev(dec != 0, n, d_ivs, d_in, d_out, d_tags, d_data_off=d_off, d_aad=d_aad if aad else None, d_aad_off=d_aoff if aad else None,
                                     d_expect_tags=d_expect if dec else None, d_auth=d_auth if dec else None, stream=caller),
         lambda: c.packets_shape(n, 0, var_len=True))


def messages(n, aad=False, dec=0):
    c = context()
    c.set_option("wipe_on_auth_fail", int(dec == 2))
    show("messages %d%s %s" % (n, " aad" if aad else "", DIR[dec]),
         lambda: c.messages_crypt_dev(dec != 0, n, d_ivs, d_in, d_len, d_out, d_tags, d_aad_ptr=d_aad if aad else None, d_aad_len=d_alen if aad else None,
                                      d_expect_tags=d_expect if dec else None, d_auth=d_auth if dec else None, stream=caller),
         lambda: c.packets_shape(n, 0, var_len=True))


def frames_probe(n, aad=False):
    c = context()
    show("frames_probe %d%s" % (n, " aad" if aad else ""), lambda: c.frames_ceiling_probe_dev(n, d_ivs, d_off, d_tags, d_aad=d_aad if aad else None, d_aad_off=d_aoff if aad else None, stream=caller),
         lambda: c.packets_shape(n, 0, var_len=True))


def batch(n, length, key, aad=0, dec=0, al=1, st=None):
    show("batch %dx%d key=%d%s %s%s" % (n, length, key, " aad" if aad else "", DIR[dec], "" if al else " out+1"),
         lambda: lib.batch_crypt_dev(dec, n, key, d_keys, d_ivs, d_in, length, d_out + (0 if al else 1), d_tags, d_aad=d_aad if aad else None, aad_len=aad,
                                     d_expect_tags=d_expect if dec else None, d_auth=d_auth if dec else None, stream=st),
         lambda: lib.batch_shape(n, length))


def batch_var(n, key, aad=False, dec=0, st=None):
    show("batch_var %d key=%d%s %s" % (n, key, " aad" if aad else "", DIR[dec]),
         lambda: lib.batch_crypt_var_dev(dec, n, key, d_keys, d_ivs, d_in, d_off, d_out, d_tags, d_aad=d_aad if aad else None, d_aad_off=d_aoff if aad else None,
                                         d_expect_tags=d_expect if dec else None, d_auth=d_auth if dec else None, stream=st),
         lambda: lib.batch_shape(n, 0, var_len=True))


def batch_probe(n, length, key):
    show("batch_probe %dx%d key=%d" % (n, length, key), lambda: lib.batch_ceiling_probe_dev(n, key, d_keys, d_ivs, length, d_tags, stream=caller), lambda: lib.batch_shape(n, length))


N_FIXED = (1, 63, 64, 65, 4096, 16383, 16384, 32768, 49151, 49152, 98304, 131072, 196608, 300000, 300001, 1 << 20)
L_FIXED = (0, 16, 64, 65, 256, 257, 512, 1024, 1025, 2048, 4096, 8448, 9000, 16384, 65536)
N_ROUTED = (1, 64, 4096, 4097, 98304, 1 << 20)
N_CU = 256


def rules():
    print("# the library's own rules (libaesgcm_fake.so).  Per launch: kernel, stream, arguments (w = workgroups), then the parameter struct: p = its pointers, set or not,")
    print("# n = n_pkts, len = pkt_len, aad = aad_len, al = aligned, pl = plain, d = deal, cb = counter_base, sc = scattered, cap = slot_cap, prio = prio_rows; what is 0 is left out")
    # every (count, size) of the fixed-size grid once, the crossings dealt round; then a few cells under every crossing
    i = 0
    for n in N_FIXED:
        for length in L_FIXED:
            packets(n, length, *CROSS[i % len(CROSS)])
            i += 5
    for cr in CROSS:
        packets(4096, 1024, *cr)
    for aad, al in ((0, 0), (13, 1), (13, 0)):
        packets(65536, 256, aad, 0, al)
    # the packet kernels' own choice where the library's default sends the call by rows, and the quarter mark of rows_min at other values
    for n in (1, 4096, 49152, 1 << 20):
        for length in (2048, 4096, 8448, 65536):
            packets(n, length, opts=(("rows_min", 0),))
    for n, length in ((16384, 1024), (16385, 1024), (16385, 4096), (16385, 4095)):
        packets(n, length, opts=(("rows_min", 4096),))
    for key in (16,):                                                   # (the round count travels to the launcher)
        packets(4096, 1024, key=key)
        packets(65536, 256, key=key)
    for n in N_ROUTED:
        routed(n, aad=n in (64, 4097), dec=(0, 2)[n in (4096, 4097)])
        messages(n, aad=n in (64, 4097), dec=(0, 2)[n in (4096, 4097)])
        frames_probe(n, aad=n == 4096)
    routed(4096, dec=1)
    # two calls on one context: the dispenser's base moves on
    for n, length in ((65536, 256), (4096, 1024)):
        c = context()
        packets(n, length, ctx=c)
        packets(n, length, ctx=c)
        routed(n, ctx=c)                                                # (a routed call has a dispenser of its own and leaves the context's alone)
        packets(n, length, dec=1, ctx=c)
    # per-packet keys: both sides of 64 and 256 packets per CU, of 2 KiB and 8 KiB, of the order's thresholds (which differ with the key length)
    i = 0
    for key in (16, 32):
        for n in (64 * N_CU - 1, 64 * N_CU, 256 * N_CU - 1, 256 * N_CU):
            for length in (256, 2048, 2049, 8192, 8193):
                aad, dec, al = CROSS[i % len(CROSS)]
                batch(n, length, key, aad, int(dec != 0), al, st=caller if i % 2 else None)
                i += 5
        for aad, dec, al in CROSS:
            if dec < 2 and key == 16:
                batch(4096, 1024, key, aad, dec, al)
        for n in (1, 64 * N_CU - 1, 64 * N_CU, 98303, 98304, 262143, 262144):
            batch_var(n, key, aad=bool(n & 1), dec=n & 1, st=caller if n & 1 else None)
        for n, length in ((64 * N_CU - 1, 2048), (64 * N_CU, 2048), (64 * N_CU, 2049), (256 * N_CU - 1, 8192), (256 * N_CU, 8192), (256 * N_CU, 8193)) if key == 16 else ((256 * N_CU, 256),):
            batch_probe(n, length, key)
    batch(1, 1024, 24)


def knobs():
    print("# forced shapes (libaesgcm_fake_dbg.so, aesgcm_debug_force_shape)")
    F.aesgcm_debug_force_shape.argtypes = [ctypes.c_char_p, ctypes.c_int]

    def forced(what, values, calls):
        for v in values:
            print("#### %s=%d%s" % (what, v, "" if F.aesgcm_debug_force_shape(what.encode(), v) == 0 else " refused"))
            for call in calls:
                call()
        F.aesgcm_debug_force_shape(what.encode(), 0)

    forced("pkt_lanes", (1, 4, 8, 16, 64), [lambda: packets(1, 16), lambda: packets(4096, 1024), lambda: packets(4096, 4096), lambda: packets(65536, 256, aad=13, dec=1, al=0),
                                            lambda: packets(1 << 20, 65536), lambda: routed(4096)])
    forced("pkt_lanes", (16, 64), [lambda: messages(4096), lambda: frames_probe(4096)])     # (messages wherever they live have no wave-per-packet form)
    forced("pkt_ilp", (1, 2), [lambda: packets(4096, 1024), lambda: packets(65536, 256), lambda: packets(300000, 64), lambda: packets(1 << 20, 1024)])
    F.aesgcm_debug_force_shape(b"pkt_lanes", 1)
    forced("pkt_ilp", (1, 2), [lambda: packets(63, 1024), lambda: packets(4096, 1024)])
    F.aesgcm_debug_force_shape(b"pkt_lanes", 0)
    forced("pkt_deal", (1, 8, 24, 64, 65), [lambda: packets(4096, 1024), lambda: packets(49152, 4096), lambda: packets(4096, 8192, opts=(("rows_min", 0),))])
    forced("pkt_deal", (8, 65), [lambda: routed(4096)])
    forced("pkt_rows", (1, 2), [lambda: packets(4096, 256), lambda: packets(4096, 65536), lambda: packets(1 << 20, 0), lambda: routed(4096)])
    forced("batch_lanes", (8, 16, 64), [lambda: batch(4096, 256, 16), lambda: batch(65536, 8192, 32), lambda: batch_var(4096, 32), lambda: batch_var(262144, 32), lambda: batch_probe(4096, 256, 16)])
    forced("batch_deal", (1, 7, 4096, 4097), [lambda: batch(65536, 256, 16), lambda: batch(65536, 8193, 32), lambda: batch_var(4096, 32)])
    forced("batch_order", (1, 2), [lambda: batch_var(4096, 32), lambda: batch_var(262144, 16), lambda: batch_var(262144, 32), lambda: batch(4096, 256, 32)])
    F.aesgcm_debug_force_shape(b"batch_lanes", 64)
    forced("batch_order", (1,), [lambda: batch_var(4096, 32)])          # (a wave per packet is never ordered)
    F.aesgcm_debug_force_shape(b"batch_lanes", 0)


knobs() if KNOBS else rules()
