"""The broadcast wire test (tests/test_broadcast.py, tests/test_broadcast_api.py):
frame_stress --mode server --broadcast-tag T against Python oracle peers.

A packet whose proto id is T is echoed to its sender and then broadcast to
every linked session of the sender's accepter (SessionManager::broadcastAccepter),
the sender included.  Every client decrypts its WHOLE received stream with one
continuous oracle RC4, so one wrong or misplaced byte garbles everything
behind it, and must find its own echoes in order, every broadcast of its
accepter in one order common to all of its clients, and each of its own
broadcasts directly behind that packet's echo.

Phases (threading.Barrier between them), so that the paths of interest are
certain to run and not left to timing:
  1. every client sends one ordinary packet and reads its echo: all linked;
  2. the first client of each accepter sends ONE tagged packet while every
     session is idle: every other session takes the shared-source path at
     offset 0 and the sender takes it behind its staged echo;
  3. all clients send their packets, tagged ones among them, in random
     chunkings at once (in-flight blocks, queued sends, copies)."""
import json
import random
import socket
import struct
import subprocess
import threading

from conftest import ROOT

ORACLE_HOOKS = "host:" + str(ROOT / "oracle" / "liboracle.so")
KEY = b"bcast-parity-key\x00with-nul"   # NUL bytes count (makeSBox takes std::string)
TAG = 0x7B1C


def rc4(key=KEY):
    import pyoracle
    return pyoracle.Rc4(key)


class _Plain:
    """RC4 off (_rc4TcpEncryption empty): the wire carries the plaintext."""

    def encryption(self, b):
        return bytes(b)


def packet(rng, size, tag, ident=None):
    """proto4z.h:704-748: u32 length, u16 reserve, u16 proto id, body.  ident
    (client, sequence number) makes a tagged packet unique."""
    body = bytes(rng.getrandbits(8) for _ in range(size - 8))
    if ident is not None:
        body = struct.pack("<II", *ident) + body[8:]
    return struct.pack("<IHH", size, 0, tag & 0xFFFF) + body


def split_packets(stream):
    out, pos = [], 0
    while pos < len(stream):
        assert len(stream) - pos >= 8, f"{len(stream) - pos} stray bytes at the end of the stream"
        ln = struct.unpack_from("<I", stream, pos)[0]
        assert 8 <= ln <= len(stream) - pos, f"bad packet length {ln} at stream byte {pos}"
        out.append(stream[pos:pos + ln])
        pos += ln
    return out


def tag_of(p):
    return struct.unpack_from("<H", p, 6)[0]


def recv_exact(s, n):
    out = bytearray()
    while len(out) < n:
        b = s.recv(n - len(out))
        if not b:
            raise EOFError(f"peer closed after {len(out)} of {n} bytes")
        out += b
    return bytes(out)


class Server:
    """frame_stress --mode server --plain-accepter --broadcast-tag TAG."""

    def __init__(self, stress, hooks, exit_after, *extra, key=KEY):
        self.p = subprocess.Popen([str(stress), "--mode", "server", "--rc4", hooks, "--key-hex", key.hex(),
                                   "--seconds", "60", "--warmup", "0", "--exit-after", str(exit_after),
                                   "--plain-accepter", "--broadcast-tag", str(TAG), *extra],
                                  stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        ports = []
        for want in ("PORT ", "PORT2 "):
            line = self.p.stdout.readline()
            if not line.startswith(want):
                self.p.kill()
                raise RuntimeError(f"server did not start: {line!r} {self.p.stderr.read()}")
            ports.append(int(line.split()[1]))
        self.port, self.port2 = ports

    def finish(self, timeout=60):
        out, err = self.p.communicate(timeout=timeout)
        assert self.p.returncode == 0, err
        return json.loads(out.strip().splitlines()[-1])


class Client:
    """One peer: what it sends is fixed by its seed before anything runs, so
    every client knows how many bytes its stream will carry."""

    def __init__(self, idx, member, keyed, seed, npk):
        self.idx, self.member, self.keyed = idx, member, keyed   # member: position among its accepter's clients
        self.rng = rng = random.Random(seed)
        self.hello = packet(rng, 40, 1)
        self.quiet = packet(rng, 600, TAG, (idx, 0)) if member == 0 else None
        self.blast = []
        for i in range(npk):
            if rng.random() < 0.25:
                self.blast.append(packet(rng, rng.choice([24, 64, 1000, 1024, 4096, 9000]), TAG, (idx, i + 1)))
            else:
                self.blast.append(packet(rng, rng.choice([8, 9, 64, 1000, 1024, 4096, 20000, rng.randint(8, 3000)]),
                                         i + 2 if (i + 2) & 0xFFFF != TAG else 2))
        self.sent = [self.hello] + ([self.quiet] if self.quiet else []) + self.blast
        self.got = bytearray()
        self.error = None

    def own_broadcasts(self):
        return [p for p in self.sent if tag_of(p) == TAG]

    def run(self, port, barrier, quiet_len, total):
        try:
            wr = rc4() if self.keyed else _Plain()
            with socket.create_connection(("127.0.0.1", port), timeout=30) as s:
                s.setsockopt(socket.IPPROTO_TCP, socket.TCP_NODELAY, 1)
                s.sendall(wr.encryption(self.hello))
                self.got += recv_exact(s, len(self.hello))
                barrier.wait(60)
                if self.quiet:
                    s.sendall(wr.encryption(self.quiet))
                self.got += recv_exact(s, quiet_len * (2 if self.quiet else 1))
                barrier.wait(60)
                wire = wr.encryption(b"".join(self.blast))
                pos = 0
                while pos < len(wire):
                    n = self.rng.choice([1, 3, 7, 100, 1500, 9000, 40000])
                    s.sendall(wire[pos:pos + n])
                    pos += n
                    s.setblocking(False)
                    try:
                        while True:
                            b = s.recv(1 << 16)
                            if not b:
                                break
                            self.got += b
                    except BlockingIOError:
                        pass
                    s.setblocking(True)
                s.settimeout(30)
                self.got += recv_exact(s, total - len(self.got))
                barrier.wait(60)                                  # nobody leaves while a broadcast may name it
        except Exception as e:                                    # noqa: BLE001
            self.error = repr(e)
            barrier.abort()


def run_broadcast_parity(stress, hooks, nkeyed=6, nplain=2, npk=24, extra=(), seed0=4000, key=KEY):
    """Returns the server's stats after every check on every client's stream."""
    clients = [Client(i, i, True, seed0 + i, npk) for i in range(nkeyed)] + \
              [Client(nkeyed + i, i, False, seed0 + nkeyed + i, npk) for i in range(nplain)]
    groups = [[c for c in clients if c.keyed], [c for c in clients if not c.keyed]]
    srv = Server(stress, hooks, len(clients), *extra, key=key)
    barrier = threading.Barrier(len(clients))
    th = []
    for g, port in zip(groups, (srv.port, srv.port2)):
        if not g:
            continue
        bc = sum(len(p) for c in g for p in c.own_broadcasts())
        for c in g:
            total = sum(len(p) for p in c.sent) + bc
            th.append(threading.Thread(target=c.run, args=(port, barrier, len(g[0].quiet), total)))
    for t in th:
        t.start()
    for t in th:
        t.join(120)
    bad = [(c.idx, c.error) for c in clients if c.error]
    if bad or any(t.is_alive() for t in th):
        srv.p.kill()
        _, err = srv.p.communicate(timeout=30)
        raise AssertionError(f"clients did not finish: {bad}; server stderr: {err[-3000:]}")
    stats = srv.finish()

    for g in groups:
        order = None
        expected = sorted(p for c in g for p in c.own_broadcasts())
        for c in g:
            wire = bytes(c.got)
            stream = (rc4(key) if c.keyed else _Plain()).encryption(wire)
            if c.keyed:
                assert wire != stream
            pk = split_packets(stream)
            seen, k, i = [], 0, 0
            while i < len(pk):
                p = pk[i]
                if k < len(c.sent) and p == c.sent[k]:            # its own echo, in order
                    k += 1
                    if tag_of(p) == TAG:                          # ... with its broadcast directly behind
                        assert i + 1 < len(pk) and pk[i + 1] == p, \
                            f"client {c.idx}: broadcast {k - 1} is not directly behind its echo"
                        seen.append(p)
                        i += 1
                else:
                    assert tag_of(p) == TAG, f"client {c.idx}: packet {i} is neither its next echo nor a broadcast"
                    seen.append(p)
                i += 1
            assert k == len(c.sent), f"client {c.idx}: {k} of {len(c.sent)} echoes"
            assert sorted(seen) == expected, f"client {c.idx}: wrong set of broadcasts"
            if order is None:
                order = seen
            assert seen == order, f"client {c.idx}: broadcast order differs from client {g[0].idx}'s"
        for c in g:                                               # each sender's broadcasts in its send order
            assert [p for p in (order or []) if struct.unpack_from("<I", p, 8)[0] == c.idx] == c.own_broadcasts()

    ncalls = sum(len(c.own_broadcasts()) for c in clients)
    assert stats["recv_packs"] == sum(len(c.sent) for c in clients)
    assert stats["linked"] == len(clients)
    assert stats["bcast_calls"] == ncalls
    assert stats["bcast_shared"] + stats["bcast_copied"] == sum(len(c.own_broadcasts()) * len(g)
                                                                 for g in groups for c in g)
    return stats
