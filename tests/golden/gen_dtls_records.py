"""Records tests/golden/dtls12_records.json: DTLS 1.2 application-data records as the system's own OpenSSL puts them on the wire, with what is needed to derive their
keys -- read by tests/dtls_fixture.py for tests/test_dtls_cpu.py and tests/test_gpu_dtls.py.

    python tests/golden/gen_dtls_records.py           # rewrites dtls12_records.json (new certificate, new randoms: the file changes every time)

Python's ssl has no DTLS, so this drives libssl through ctypes: client and server in one process over memory BIOs (no socket), a key-log callback for the master secret.
Two connections, ECDHE-RSA-AES128-GCM-SHA256 and ECDHE-RSA-AES256-GCM-SHA384, and in both directions writes of 1, 15, 16, 17, 100 and 1400 bytes.  Stored as
tls_records.json stores its TLS 1.2 connections: master secret and randoms, and per write the record as it left the BIO and the seed of its plaintext
(util.splitmix_bytes(seed, n): the written bytes are not stored).  The certificate is made with the `openssl` command into a temporary directory and never kept.
OpenSSL 3.0 has no DTLS 1.3: there is nothing of that version to record."""
import base64
import ctypes
import ctypes.util
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

WRITES = (1, 15, 16, 17, 100, 1400)
CONNECTIONS = [("ECDHE-RSA-AES128-GCM-SHA256", 16, "sha256"), ("ECDHE-RSA-AES256-GCM-SHA384", 32, "sha384")]
DTLS1_2_VERSION = 0xFEFD
SSL_CTRL_SET_MTU, SSL_CTRL_SET_MIN_PROTO_VERSION, SSL_CTRL_SET_MAX_PROTO_VERSION = 17, 123, 124
SSL_OP_NO_QUERY_MTU = 0x1000
BIO_C_SET_BUF_MEM_EOF_RETURN = 130
SSL_ERROR_WANT_READ = 2
KEYLOG = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.c_char_p)


def _libssl():
    S = ctypes.CDLL(ctypes.util.find_library("ssl") or "libssl.so.3")
    C = ctypes.CDLL(ctypes.util.find_library("crypto") or "libcrypto.so.3")
    vp, ci, cl, cp = ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_char_p
    for lib, name, res, args in (
            (S, "DTLS_method", vp, []), (S, "SSL_CTX_new", vp, [vp]), (S, "SSL_CTX_free", None, [vp]), (S, "SSL_CTX_ctrl", cl, [vp, ci, cl, vp]),
            (S, "SSL_CTX_set_cipher_list", ci, [vp, cp]), (S, "SSL_CTX_use_certificate_file", ci, [vp, cp, ci]), (S, "SSL_CTX_use_PrivateKey_file", ci, [vp, cp, ci]),
            (S, "SSL_CTX_set_keylog_callback", None, [vp, KEYLOG]), (S, "SSL_new", vp, [vp]), (S, "SSL_free", None, [vp]), (S, "SSL_set_bio", None, [vp, vp, vp]),
            (S, "SSL_set_connect_state", None, [vp]), (S, "SSL_set_accept_state", None, [vp]), (S, "SSL_do_handshake", ci, [vp]), (S, "SSL_get_error", ci, [vp, ci]),
            (S, "SSL_write", ci, [vp, cp, ci]), (S, "SSL_read", ci, [vp, cp, ci]), (S, "SSL_ctrl", cl, [vp, ci, cl, vp]), (S, "SSL_set_options", ctypes.c_uint64, [vp, ctypes.c_uint64]),
            (S, "SSL_get_version", cp, [vp]), (S, "SSL_get_current_cipher", vp, [vp]), (S, "SSL_CIPHER_get_name", cp, [vp]),
            (C, "BIO_s_mem", vp, []), (C, "BIO_new", vp, [vp]), (C, "BIO_read", ci, [vp, cp, ci]), (C, "BIO_write", ci, [vp, cp, ci]), (C, "BIO_ctrl", cl, [vp, ci, cl, vp])):
        f = getattr(lib, name)
        f.restype, f.argtypes = res, args
    return S, C


def _records(blob):
    out, at = [], 0
    while at < len(blob):
        n = int.from_bytes(blob[at + 11:at + 13], "big")
        out.append(blob[at:at + 13 + n])
        at += 13 + n
    assert at == len(blob)
    return out


def connection(S, C, idx, tmp):
    from util import splitmix_bytes
    suite, key_len, hname = CONNECTIONS[idx]
    log = []
    cb = KEYLOG(lambda ssl, line: log.append(line.decode()))
    ctx, ssl, rbio, wbio = {}, {}, {}, {}
    for who in ("client", "server"):
        c = ctx[who] = S.SSL_CTX_new(S.DTLS_method())
        assert c
        assert S.SSL_CTX_ctrl(c, SSL_CTRL_SET_MIN_PROTO_VERSION, DTLS1_2_VERSION, None) == 1 and S.SSL_CTX_ctrl(c, SSL_CTRL_SET_MAX_PROTO_VERSION, DTLS1_2_VERSION, None) == 1
        assert S.SSL_CTX_set_cipher_list(c, suite.encode()) == 1
        S.SSL_CTX_set_keylog_callback(c, cb)
        if who == "server":
            assert S.SSL_CTX_use_certificate_file(c, os.path.join(tmp, "cert.pem").encode(), 1) == 1
            assert S.SSL_CTX_use_PrivateKey_file(c, os.path.join(tmp, "key.pem").encode(), 1) == 1
        s = ssl[who] = S.SSL_new(c)
        assert s
        rbio[who], wbio[who] = C.BIO_new(C.BIO_s_mem()), C.BIO_new(C.BIO_s_mem())
        for b in (rbio[who], wbio[who]):
            C.BIO_ctrl(b, BIO_C_SET_BUF_MEM_EOF_RETURN, -1, None)              # an empty BIO means "try again", not end of file
        S.SSL_set_bio(s, rbio[who], wbio[who])                                 # (the SSL owns both from here)
        S.SSL_set_options(s, SSL_OP_NO_QUERY_MTU)
        S.SSL_ctrl(s, SSL_CTRL_SET_MTU, 4096, None)                            # a memory BIO has no path MTU: every write fits one record
        (S.SSL_set_connect_state if who == "client" else S.SSL_set_accept_state)(s)
    peer = {"client": "server", "server": "client"}
    first = {}
    buf = ctypes.create_string_buffer(1 << 16)

    def pump(who):
        out = b""
        while True:
            n = C.BIO_read(wbio[who], buf, len(buf))
            if n <= 0:
                break
            out += buf.raw[:n]
        if out:
            first.setdefault(who, out)
            assert C.BIO_write(rbio[peer[who]], out, len(out)) == len(out)
        return out

    done = set()
    for _ in range(20):
        for who in ("client", "server"):
            if who not in done:
                r = S.SSL_do_handshake(ssl[who])
                if r == 1:
                    done.add(who)
                else:
                    assert S.SSL_get_error(ssl[who], r) == SSL_ERROR_WANT_READ, (who, S.SSL_get_error(ssl[who], r))
            pump(who)
        if len(done) == 2:
            break
    assert len(done) == 2
    assert S.SSL_get_version(ssl["client"]) == b"DTLSv1.2" and S.SSL_CIPHER_get_name(S.SSL_get_current_cipher(ssl["client"])) == suite.encode()
    # ClientHello / ServerHello: record header (13), handshake header (12: type, length, message sequence, fragment offset and length), version (2), random (32)
    rnd = {who: first[who][27:59] for who in ("client", "server")}
    assert first["client"][0] == 22 and first["client"][13] == 1 and first["server"][0] == 22 and first["server"][13] == 2
    secrets = {}
    for line in log:
        f = line.split()
        if len(f) == 3 and f[0] == "CLIENT_RANDOM":
            assert bytes.fromhex(f[1]) == rnd["client"]
            secrets[f[0]] = f[2]
    conn = {"version": "dtls1.2", "suite": suite, "key_len": key_len, "hash": hname, "master_secret": secrets["CLIENT_RANDOM"],
            "client_random": rnd["client"].hex(), "server_random": rnd["server"].hex(), "dirs": {}}
    for who in ("client", "server"):
        recs = []
        for w, n in enumerate(WRITES):
            seed = 0xD7150000 + (idx << 12) + ((who == "server") << 8) + w
            pt = splitmix_bytes(seed, n)
            assert S.SSL_write(ssl[who], pt, n) == n
            wire = _records(pump(who))
            assert len(wire) == 1 and wire[0][0] == 23 and wire[0][3:5] == b"\x00\x01" and len(wire[0]) == n + 37, (n, [len(r) for r in wire])
            assert S.SSL_read(ssl[peer[who]], buf, len(buf)) == n and buf.raw[:n] == pt
            recs.append({"seed": seed, "len": n, "wire": base64.b64encode(wire[0]).decode()})
        conn["dirs"][who] = {"records": recs}
    for who in ("client", "server"):
        S.SSL_free(ssl[who])
        S.SSL_CTX_free(ctx[who])
    return conn


def main():
    S, C = _libssl()
    with tempfile.TemporaryDirectory() as tmp:
        subprocess.run(["openssl", "req", "-x509", "-newkey", "rsa:2048", "-nodes", "-keyout", os.path.join(tmp, "key.pem"), "-out", os.path.join(tmp, "cert.pem"),
                        "-days", "2", "-subj", "/CN=dtls-records.invalid"], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        conns = [connection(S, C, idx, tmp) for idx in range(len(CONNECTIONS))]
    import ssl as pyssl
    doc = {"about": "DTLS 1.2 application-data records of %s through libssl over memory BIOs; tests/golden/gen_dtls_records.py.  wire: base64 of the record as sent; "
                    "plaintext = util.splitmix_bytes(seed, len)" % pyssl.OPENSSL_VERSION,
           "connections": conns}
    with open(os.path.join(HERE, "dtls12_records.json"), "w") as f:
        json.dump(doc, f, indent=0, separators=(",", ":"))
        f.write("\n")


if __name__ == "__main__":
    main()
