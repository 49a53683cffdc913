"""Records tests/golden/tls_records.json: application-data records as the system's own TLS stack (Python's ssl on OpenSSL) puts them on the wire, with what is needed to
derive their keys -- the fixture of tests/test_tls_cpu.py and tests/test_gpu_tls.py.

    python tests/golden/gen_tls_records.py            # rewrites tls_records.json (new certificate, new randoms: the file changes every time)

Four connections, client and server in one process over ssl.MemoryBIO with a key log: TLS 1.3 with TLS_AES_128_GCM_SHA256 and with TLS_AES_256_GCM_SHA384, TLS 1.2
with ECDHE-RSA-AES128-GCM-SHA256 and with ECDHE-RSA-AES256-GCM-SHA384.  Python's ssl cannot choose a TLS 1.3 suite, so every connection runs in a child process of this
script whose OPENSSL_CONF names a throw-away configuration with the one suite.  The certificate is made with the `openssl` command into a temporary directory and
never kept.  Per connection and direction: the traffic secret (1.3) or master secret and randoms (1.2), and for writes of 1, 15, 16, 17, 100 and 1400 bytes -- in one
connection per version also one of 16384 -- the record as it left the BIO, its sequence number and the seed of its plaintext (util.splitmix_bytes(seed, n): the written
bytes are not stored).  No session tickets (num_tickets = 0), so the server's first application record of TLS 1.3 has sequence number 0; in TLS 1.2 the Finished
message took 0."""
import base64
import json
import os
import ssl
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

WRITES = (1, 15, 16, 17, 100, 1400)
BIG = 16384
CONNECTIONS = [
    # version, suite, key_len, hash, with the 16384-byte write
    ("1.3", "TLS_AES_128_GCM_SHA256", 16, "sha256", False),
    ("1.3", "TLS_AES_256_GCM_SHA384", 32, "sha384", True),
    ("1.2", "ECDHE-RSA-AES128-GCM-SHA256", 16, "sha256", True),
    ("1.2", "ECDHE-RSA-AES256-GCM-SHA384", 32, "sha384", False),
]
CONF = """openssl_conf = openssl_init
[openssl_init]
ssl_conf = ssl_sect
[ssl_sect]
system_default = system_default_sect
[system_default_sect]
%s = %s
"""


def _records(blob):
    out, at = [], 0
    while at < len(blob):
        n = int.from_bytes(blob[at + 3:at + 5], "big")
        out.append(blob[at:at + 5 + n])
        at += 5 + n
    assert at == len(blob)
    return out


def connection(idx, tmp):
    from util import splitmix_bytes
    version, suite, key_len, hname, big = CONNECTIONS[idx]
    v = ssl.TLSVersion.TLSv1_3 if version == "1.3" else ssl.TLSVersion.TLSv1_2
    keylog = os.path.join(tmp, "keylog%d.txt" % idx)
    sctx = ssl.SSLContext(ssl.PROTOCOL_TLS_SERVER)
    sctx.load_cert_chain(os.path.join(tmp, "cert.pem"), os.path.join(tmp, "key.pem"))
    cctx = ssl.SSLContext(ssl.PROTOCOL_TLS_CLIENT)
    cctx.check_hostname = False
    cctx.verify_mode = ssl.CERT_NONE
    for ctx in (sctx, cctx):
        ctx.minimum_version = ctx.maximum_version = v
        ctx.keylog_filename = keylog
        if version == "1.2":
            ctx.set_ciphers(suite)
    sctx.num_tickets = 0
    bio = {"client": (ssl.MemoryBIO(), ssl.MemoryBIO()), "server": (ssl.MemoryBIO(), ssl.MemoryBIO())}       # (incoming, outgoing)
    obj = {"client": cctx.wrap_bio(*bio["client"], server_side=False), "server": sctx.wrap_bio(*bio["server"], server_side=True)}
    peer = {"client": "server", "server": "client"}
    first = {}

    def pump(who):
        data = bio[who][1].read()
        if data:
            first.setdefault(who, data)
            bio[peer[who]][0].write(data)
        return data

    done = set()
    for _ in range(20):
        for who in ("client", "server"):
            if who not in done:
                try:
                    obj[who].do_handshake()
                    done.add(who)
                except ssl.SSLWantReadError:
                    pass
            pump(who)
        if len(done) == 2:
            break
    assert len(done) == 2
    for who in ("client", "server"):                                      # nothing of the handshake is left on its way
        try:
            obj[who].read(1)
        except ssl.SSLWantReadError:
            pass
        assert not pump(who)
    assert obj["client"].version() == "TLSv" + version and obj["client"].cipher()[0] == suite, (obj["client"].version(), obj["client"].cipher())

    # ClientHello / ServerHello: record header (5), handshake header (4), legacy version (2), random (32)
    rnd = {who: first[who][11:43] for who in ("client", "server")}
    assert first["client"][0] == 22 and first["client"][5] == 1 and first["server"][0] == 22 and first["server"][5] == 2
    log = {}
    for line in open(keylog):
        f = line.split()
        if len(f) == 3 and not line.startswith("#"):
            assert bytes.fromhex(f[1]) == rnd["client"]
            log[f[0]] = f[2]
    conn = {"version": version, "suite": suite, "key_len": key_len, "hash": hname, "dirs": {}}
    if version == "1.2":
        conn.update(master_secret=log["CLIENT_RANDOM"], client_random=rnd["client"].hex(), server_random=rnd["server"].hex())
    seq = {"client": 0, "server": 0} if version == "1.3" else {"client": 1, "server": 1}
    for who in ("client", "server"):
        recs = []
        sizes = WRITES + ((BIG,) if big and who == "client" else ())
        for w, n in enumerate(sizes):
            seed = 0x7150000 + (idx << 12) + ((who == "server") << 8) + w
            pt = splitmix_bytes(seed, n)
            assert obj[who].write(pt) == n
            wire = _records(pump(who))
            assert len(wire) == 1 and wire[0][0] == 23, (n, [len(r) for r in wire])
            got = b""
            while len(got) < n:
                got += obj[peer[who]].read(n - len(got))
            assert got == pt
            recs.append({"seq": seq[who], "seed": seed, "len": n, "wire": base64.b64encode(wire[0]).decode()})
            seq[who] += 1
        d = {"records": recs}
        if version == "1.3":
            d["traffic_secret"] = log["%s_TRAFFIC_SECRET_0" % who.upper()]
        conn["dirs"][who] = d
    return conn


def main():
    if len(sys.argv) == 4 and sys.argv[1] == "--connection":
        json.dump(connection(int(sys.argv[2]), sys.argv[3]), sys.stdout)
        return
    with tempfile.TemporaryDirectory() as tmp:
        subprocess.run(["openssl", "req", "-x509", "-newkey", "rsa:2048", "-nodes", "-keyout", os.path.join(tmp, "key.pem"), "-out", os.path.join(tmp, "cert.pem"),
                        "-days", "2", "-subj", "/CN=tls-records.invalid"], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        conns = []
        for idx, (version, suite, _, _, _) in enumerate(CONNECTIONS):
            conf = os.path.join(tmp, "openssl%d.cnf" % idx)
            with open(conf, "w") as f:
                f.write(CONF % (("Ciphersuites", suite) if version == "1.3" else ("CipherString", suite)))
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--connection", str(idx), tmp], check=True, stdout=subprocess.PIPE,
                                 env=dict(os.environ, OPENSSL_CONF=conf)).stdout
            conns.append(json.loads(out))
    doc = {"about": "application-data records of %s through Python's ssl over MemoryBIO; tests/golden/gen_tls_records.py.  wire: base64 of the record as sent; "
                    "plaintext = util.splitmix_bytes(seed, len)" % ssl.OPENSSL_VERSION,
           "connections": conns}
    with open(os.path.join(HERE, "tls_records.json"), "w") as f:
        json.dump(doc, f, indent=0, separators=(",", ":"))
        f.write("\n")


if __name__ == "__main__":
    main()
