"""Host cost of a whole-message call: wall time per aesgcm_encrypt_dev over the fake runtime (tests/fake_hip: nothing runs, a launch is a function call), so what
is timed is the library's own host side -- planning the launches and walking them -- plus the binding's constant.  One line per run:

    AESGCM_LIB=.../libaesgcm_fake.so python profiles/msgplan/host_cost.py [calls]

Run it alternately on the fake library of two commits (profiles/msgplan/ab.txt)."""
import ctypes
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import aesgcm_amd  # noqa: E402,F401
from aesgcm_amd import lib  # noqa: E402

L = lib.load()
calls = int(sys.argv[1]) if len(sys.argv) > 1 else 200000
c = lib.Context(bytes(range(32)))
d_in, d_out = lib.DeviceBuffer(16), lib.DeviceBuffer(16)
iv = bytes(range(1, 13))
tag = ctypes.create_string_buffer(16)
f = L.aesgcm_encrypt_dev
out = []
for n in (1000, 4 << 20):
    best = None
    for rep in range(3):                                                # the best of three passes: the least disturbed
        t0 = time.perf_counter()
        for _ in range(calls):
            f(c._c, iv, None, 0, d_in.ptr, n, d_out.ptr, tag, None)
        dt = (time.perf_counter() - t0) / calls * 1e9
        best = dt if best is None or dt < best else best
    out.append("%d bytes: %.0f ns per call" % (n, best))
print("; ".join(out))
