"""Records tests/golden/dtls_srtp_exporter.json: what the system's own OpenSSL exports under the DTLS-SRTP label from a DTLS 1.2 connection, beside the connection's
master secret and randoms -- read by tests/test_prf12_cpu.py and tests/test_gpu_prf12.py, which hold aesgcm_prf12_export_srtp_dev to it.

    python tests/golden/gen_dtls_srtp_exporter.py     # rewrites dtls_srtp_exporter.json (new certificate, new randoms: the file changes every time)

As gen_dtls_records.py: libssl through ctypes, client and server in one process over memory BIOs (no socket), a key-log callback for the master secret.  The exported
bytes are SSL_export_keying_material(ssl, out, 88, "EXTRACTOR-dtls_srtp", 19, NULL, 0, use_context = 0) -- the call behind `openssl s_client -keymatexport
EXTRACTOR-dtls_srtp -keymatexportlen 88` -- asked of the client AND of the server, which must agree.  88 = 2 * 32 + 2 * 12 + room: an exporter's output of n bytes
is the first n bytes of a longer one, so the 56 bytes of an AES-128 profile (2 * 16 + 2 * 12) are these 88's first 56.  Two connections, one per PRF hash:
ECDHE-RSA-AES128-GCM-SHA256 and ECDHE-RSA-AES256-GCM-SHA384.  No use_srtp extension is negotiated: RFC 5705's output depends on label, master secret and randoms
alone."""
import ctypes
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE), HERE]

import gen_dtls_records as G  # noqa: E402

LABEL = b"EXTRACTOR-dtls_srtp"
EXPORT_LEN = 88


def connection(S, C, idx, tmp):
    suite, key_len, hname = G.CONNECTIONS[idx]
    S.SSL_export_keying_material.restype = ctypes.c_int
    S.SSL_export_keying_material.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int]
    log = []
    cb = G.KEYLOG(lambda ssl, line: log.append(line.decode()))
    ctx, ssl, rbio, wbio = {}, {}, {}, {}
    for who in ("client", "server"):
        c = ctx[who] = S.SSL_CTX_new(S.DTLS_method())
        assert c
        assert S.SSL_CTX_ctrl(c, G.SSL_CTRL_SET_MIN_PROTO_VERSION, G.DTLS1_2_VERSION, None) == 1 and S.SSL_CTX_ctrl(c, G.SSL_CTRL_SET_MAX_PROTO_VERSION, G.DTLS1_2_VERSION, None) == 1
        assert S.SSL_CTX_set_cipher_list(c, suite.encode()) == 1
        S.SSL_CTX_set_keylog_callback(c, cb)
        if who == "server":
            assert S.SSL_CTX_use_certificate_file(c, os.path.join(tmp, "cert.pem").encode(), 1) == 1
            assert S.SSL_CTX_use_PrivateKey_file(c, os.path.join(tmp, "key.pem").encode(), 1) == 1
        s = ssl[who] = S.SSL_new(c)
        assert s
        rbio[who], wbio[who] = C.BIO_new(C.BIO_s_mem()), C.BIO_new(C.BIO_s_mem())
        for b in (rbio[who], wbio[who]):
            C.BIO_ctrl(b, G.BIO_C_SET_BUF_MEM_EOF_RETURN, -1, None)
        S.SSL_set_bio(s, rbio[who], wbio[who])
        S.SSL_set_options(s, G.SSL_OP_NO_QUERY_MTU)
        S.SSL_ctrl(s, G.SSL_CTRL_SET_MTU, 4096, None)
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

    done = set()
    for _ in range(20):
        for who in ("client", "server"):
            if who not in done:
                r = S.SSL_do_handshake(ssl[who])
                if r == 1:
                    done.add(who)
                else:
                    assert S.SSL_get_error(ssl[who], r) == G.SSL_ERROR_WANT_READ, (who, S.SSL_get_error(ssl[who], r))
            pump(who)
        if len(done) == 2:
            break
    assert len(done) == 2
    assert S.SSL_get_version(ssl["client"]) == b"DTLSv1.2" and S.SSL_CIPHER_get_name(S.SSL_get_current_cipher(ssl["client"])) == suite.encode()
    rnd = {who: first[who][27:59] for who in ("client", "server")}            # (where the randoms lie: gen_dtls_records.py)
    assert first["client"][0] == 22 and first["client"][13] == 1 and first["server"][0] == 22 and first["server"][13] == 2
    master = [f.split()[2] for f in log if len(f.split()) == 3 and f.split()[0] == "CLIENT_RANDOM" and bytes.fromhex(f.split()[1]) == rnd["client"]][0]
    got = {}
    for who in ("client", "server"):
        out = ctypes.create_string_buffer(EXPORT_LEN)
        assert S.SSL_export_keying_material(ssl[who], out, EXPORT_LEN, LABEL, len(LABEL), None, 0, 0) == 1
        got[who] = out.raw
    assert got["client"] == got["server"]
    for who in ("client", "server"):
        S.SSL_free(ssl[who])
        S.SSL_CTX_free(ctx[who])
    return {"version": "dtls1.2", "suite": suite, "hash": hname, "master_secret": master, "client_random": rnd["client"].hex(), "server_random": rnd["server"].hex(),
            "label": LABEL.decode(), "exported": got["client"].hex()}


def main():
    S, C = G._libssl()
    with tempfile.TemporaryDirectory() as tmp:
        subprocess.run(["openssl", "req", "-x509", "-newkey", "rsa:2048", "-nodes", "-keyout", os.path.join(tmp, "key.pem"), "-out", os.path.join(tmp, "cert.pem"),
                        "-days", "2", "-subj", "/CN=dtls-srtp-exporter.invalid"], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        conns = [connection(S, C, idx, tmp) for idx in range(len(G.CONNECTIONS))]
    import ssl as pyssl
    doc = {"about": "SSL_export_keying_material of %s under the DTLS-SRTP label, without context, %d bytes, from DTLS 1.2 connections over memory BIOs; "
                    "tests/golden/gen_dtls_srtp_exporter.py" % (pyssl.OPENSSL_VERSION, EXPORT_LEN),
           "connections": conns}
    with open(os.path.join(HERE, "dtls_srtp_exporter.json"), "w") as f:
        json.dump(doc, f, indent=0, separators=(",", ":"))
        f.write("\n")


if __name__ == "__main__":
    main()
