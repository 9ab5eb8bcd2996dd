"""A websocket client for the viewer's tests, written from socket, os and struct alone (RFC 6455: the opening handshake,
masked frames in the three length forms); it shares no code with tinysplat_amd/viewer.py."""
import base64
import json
import os
import socket
import struct


class Client:
    def __init__(self, port):
        self.sock = socket.create_connection(("127.0.0.1", port), timeout=10)
        self.key = base64.b64encode(os.urandom(16)).decode()
        self.sock.sendall((f"GET / HTTP/1.1\r\nHost: 127.0.0.1:{port}\r\nUpgrade: websocket\r\nConnection: Upgrade\r\n"
                           f"Sec-WebSocket-Key: {self.key}\r\nSec-WebSocket-Version: 13\r\n\r\n").encode())
        head = b""
        while not head.endswith(b"\r\n\r\n"):
            head += self._read(1)
        self.status, *lines = head.decode().split("\r\n")
        self.fields = {k.lower(): v.strip() for k, _, v in (ln.partition(":") for ln in lines) if v}

    def _read(self, n):
        out = b""
        while len(out) < n:
            part = self.sock.recv(n - len(out))
            if not part:
                raise ConnectionError("closed")
            out += part
        return out

    def send(self, opcode, payload, length_form=None):
        """A masked final frame; length_form forces the 16- or 64-bit form for a short payload."""
        n, mask = len(payload), os.urandom(4)
        if length_form == 64 or n >= 65536:
            head = struct.pack("!BBQ", 0x80 | opcode, 0x80 | 127, n)
        elif length_form == 16 or n >= 126:
            head = struct.pack("!BBH", 0x80 | opcode, 0x80 | 126, n)
        else:
            head = struct.pack("!BB", 0x80 | opcode, 0x80 | n)
        self.sock.sendall(head + mask + bytes(c ^ mask[i & 3] for i, c in enumerate(payload)))

    def send_json(self, data, **kw):
        self.send(0x1, json.dumps(data).encode(), **kw)

    def recv(self):
        """-> (opcode, payload, the length form the server chose)."""
        b0, b1 = self._read(2)
        assert b0 & 0x80 and not b1 & 0x80                     # final, and a server never masks
        n, form = b1 & 0x7F, 7
        if n == 126:
            (n,), form = struct.unpack("!H", self._read(2)), 16
        elif n == 127:
            (n,), form = struct.unpack("!Q", self._read(8)), 64
        return b0 & 0x0F, self._read(n), form

    def close(self):
        self.sock.close()
