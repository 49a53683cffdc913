"""The reference the send-counter tests hold the library to (tests/test_txnum_cpu.py through the CPU harness tests/txnum_emul, tests/test_gpu_txnum.py on the GPU): a
dict of counters walked in array order, written from the text of include/aesgcm.h "SEND COUNTERS" alone.  No device, no library."""
NONE = 2 ** 64 - 1
FROM_END, KEEP_TOP, WHOLE = 1, 2, 4
FORMATS = {                                   # name: (num_off, num_len, dup_off, flags), the issue's table
    "macsec": (16, 4, 0, WHOLE), "macsec_xpn": (16, 4, 0, 0), "esp": (4, 4, 0, WHOLE), "esp_esn": (4, 4, 0, 0), "tls12": (5, 8, 0, WHOLE),
    "dtls12": (5, 6, 15, WHOLE), "srtcp": (4, 4, 0, FROM_END | KEEP_TOP | WHOLE), "srtcp_mki4": (8, 4, 0, FROM_END | KEEP_TOP | WHOLE), "number_only": (0, 0, 0, 0),
}


def assign(fmt, counters, ctrs, data=b"", offs=None):
    """One assign call.  counters = {ctr: [next, limit]} for every counter of the table (changed in place); fmt = (num_off, num_len, dup_off, flags).
    -> (nums, his, refused, data afterwards, lowest refused index or None)"""
    num_off, L, dup_off, flags = fmt
    out, nums, refused = bytearray(data), [], []
    for p, c in enumerate(ctrs):
        num = None
        if c in counters and counters[c][0] < counters[c][1]:
            num = counters[c][0]
            counters[c][0] += 1                                               # counted: what refuses the packet from here on burns the number
        if num is not None and L:
            bits = 8 * L - (1 if flags & KEEP_TOP else 0)
            b, e = offs[p], offs[p + 1]
            places = [len_ - o if flags & FROM_END else o for o in ([num_off, dup_off] if dup_off else [num_off]) for len_ in (e - b,)]
            if (flags & WHOLE and num >> bits) or e < b or any(at < 0 or at + L > e - b for at in places):
                num = None
            else:
                for at in places:
                    field = (num & ((1 << bits) - 1)) | (((out[b + at] >> 7) << bits) if flags & KEEP_TOP else 0)
                    out[b + at:b + at + L] = field.to_bytes(L, "big")
        nums.append(NONE if num is None else num)
        refused.append(num is None)
    his = [n >> 32 for n in nums]
    return nums, his, refused, bytes(out), (refused.index(True) if True in refused else None)
