"""Forward-only viewer frame.

Mirrors the render half of /root/reference/tinysplat/viewer.py:79-98 (``process_async_queue``):
take a pose from a client message, update the client's camera, render under ``torch.no_grad()``
with a black background, bring the image to the host and scale it to 0..255.  ``render_jpeg`` is the
request as the reference serves it (viewer.py:22-27): the frame encoded as a JPEG, here on the GPU
(jpeg.py), and ``Viewer`` is the websocket server around it (viewer.py:33-98)
on the standard library alone.  The browser client is not part of this package.

What is MI355X-specific: the frame runs through ``frame.render_view`` - the render kernels with
every backward-only output dropped - and the x255 scaling is done on the GPU into a pinned host
buffer, so a request costs the kernels plus one 24.9 MB (1080p float32) or 6.2 MB (uint8) copy;
``render_jpeg`` hands the frame to the encoder's kernels where it lies and copies only the file.
"""
from __future__ import annotations

import asyncio
import base64
import copy
import hashlib
import json
import struct
import threading
from typing import Optional

import numpy as np
import torch

from .scene import Scene


class ViewRenderer:
    def __init__(self, model, camera, device="cuda:0"):
        """``camera``: the template every client camera is copied from (viewer.py:61-62 copies
        ``scene.cameras[0]``)."""
        self.device = torch.device(device)
        self.model = model
        self.camera = copy.copy(camera)
        self.scene = Scene([self.camera], model, device=self.device)      # viewer.py:61-62, :92
        self.rasterizer = self.scene.rasterizer
        self._pinned = {}
        self._encoders = {}

    def _host_buffer(self, shape, dtype):
        """Two pinned buffers per (shape, dtype), used alternately: the array handed out by one
        request stays valid while the next request renders (an encoder / websocket send may still
        hold it, viewer.py:44-56) and is overwritten by the request after that."""
        key = (tuple(shape), dtype)
        pair = self._pinned.get(key)
        if pair is None:
            pair = [torch.empty(shape, dtype=dtype, pin_memory=True) for _ in range(2)]
            self._pinned = {key: pair}
        pair.reverse()
        return pair[0]

    def render(self, position, quat, as_uint8: bool = False) -> np.ndarray:
        """One ``renderRequest`` (viewer.py:82-95) -> image [H, W, 3] scaled to 0..255:
        float32 exactly as the reference hands it to its encoder (``img * 255``), or rounded
        uint8 when ``as_uint8`` (what a JPEG encoder consumes).  The returned array is a view of a
        pinned host buffer that stays untouched until the SECOND following call (double-buffered);
        copy it to keep it longer."""
        self.camera.update_view_matrix(np.asarray(position, dtype=np.float32),
                                       np.asarray(quat, dtype=np.float32))                 # :84-87
        with torch.no_grad():                                                               # :90
            self.model.background = torch.zeros(3, device=self.device)                     # :91
            img, _extras = self.scene.render(self.camera)                                   # :92
            img = img * 255                                                                 # :94
            if as_uint8:
                img = img.clamp_(0, 255).round_().to(torch.uint8)
            host = self._host_buffer(img.shape, img.dtype)
            host.copy_(img, non_blocking=True)                                              # :93
        torch.cuda.current_stream(self.device).synchronize()
        return host.numpy()

    def _frame(self, position, quat) -> torch.Tensor:
        """The request's image on the device, float32 [H, W, 3] in 0..1, as the compositing kernel left it."""
        self.camera.update_view_matrix(np.asarray(position, dtype=np.float32),
                                       np.asarray(quat, dtype=np.float32))                 # :84-87
        with torch.no_grad():                                                               # :90
            self.model.background = torch.zeros(3, device=self.device)                     # :91
            img, _extras = self.scene.render(self.camera)                                   # :92
        return img

    def render_jpeg(self, position, quat, quality: int = 90, subsampling: str = "420") -> bytes:
        """One ``renderRequest`` -> a baseline JPEG file of the frame: the pose handling and the black background of
        ``render``, the samples of ``render(as_uint8=True)``, encoded on the GPU from the tensor ``scene.render``
        returned (an interleaved RGB + depth frame is read with its stride of 4 floats: no copy, no permute)."""
        from .jpeg import JpegEncoder
        img = self._frame(position, quat)
        key = (img.shape[1], img.shape[0], subsampling)
        enc = self._encoders.get(key)
        if enc is None:
            enc = JpegEncoder(img.shape[1], img.shape[0], quality, subsampling, device=self.device)
            self._encoders = {key: enc}
        return enc.encode(img, quality)


# ------------------------------------------------------------------------------------------------------- the server
_WS_GUID = b"258EAFA5-E914-47DA-95CA-C5AB0DC85B11"                  # RFC 6455 section 1.3
_MAX_MESSAGE = 1 << 20                                              # a client message is a few hundred bytes of JSON


def websocket_accept(key: str) -> str:
    """Sec-WebSocket-Accept of a client's Sec-WebSocket-Key (RFC 6455 section 4.2.2)."""
    return base64.b64encode(hashlib.sha1(key.strip().encode("ascii") + _WS_GUID).digest()).decode("ascii")


def websocket_frame(opcode: int, payload: bytes) -> bytes:
    """One unmasked, final frame as a server sends it: the 7-, 16- or 64-bit length form (RFC 6455 section 5.2)."""
    n = len(payload)
    if n < 126:
        head = struct.pack("!BB", 0x80 | opcode, n)
    elif n < 65536:
        head = struct.pack("!BBH", 0x80 | opcode, 126, n)
    else:
        head = struct.pack("!BBQ", 0x80 | opcode, 127, n)
    return head + payload


class _Client:
    def __init__(self, writer):
        self.writer = writer
        self.camera = None
        self.closed = False

    def send(self, opcode: int, payload: bytes) -> None:
        """On the network thread only."""
        if not self.closed and not self.writer.is_closing():
            self.writer.write(websocket_frame(opcode, payload))

    def send_json(self, data) -> None:
        self.send(0x1, json.dumps(data).encode("utf-8"))


class Viewer:
    """The reference's viewer server (tinysplat/viewer.py:33-98) without its dependencies: an RFC 6455 server on
    ``asyncio.start_server`` in a background thread, and a one-slot mailbox between it and the thread that owns the GPU.

    Protocol (text frames of JSON): ``{"type": "cameraInfo"}`` gives the client a copy of the renderer's template camera;
    ``{"type": "renderRequest", "position": [x, y, z], "quat": [w, x, y, z]}`` is put into the mailbox, where a newer
    request evicts an older one (:73-77); the answer is ``{"image": "<base64 of the JPEG file>"}`` (:22-27).

    The network thread never touches the GPU: ``service()``, called by the thread that renders (between training steps:
    ``fit(on_step=...)``, or in ``run_forever()`` for a saved scene), renders at most the one pending request through
    ``renderer.render_jpeg`` and hands the bytes back to the network thread."""

    def __init__(self, renderer, ip: str = "127.0.0.1", port: int = 8765, quality: int = 90, subsampling: str = "420"):
        self.renderer, self.ip, self.port = renderer, ip, int(port)
        self.quality, self.subsampling = int(quality), subsampling
        self.rendered = 0
        self._lock = threading.Lock()
        self._mailbox = None
        self._wake = threading.Event()
        self._stopping = threading.Event()
        self._ready = threading.Event()
        self._error = None
        self._clients = set()
        self._loop = asyncio.new_event_loop()
        self._thread = threading.Thread(target=self._network, name="tinysplat-viewer", daemon=True)
        self._thread.start()
        self._ready.wait()
        if self._error is not None:
            raise self._error

    # ---- network thread
    def _network(self) -> None:
        asyncio.set_event_loop(self._loop)
        try:
            self._server = self._loop.run_until_complete(asyncio.start_server(self._handle, self.ip, self.port))
            self.port = self._server.sockets[0].getsockname()[1]
        except Exception as e:                       # the address is taken, ...: the constructor raises it
            self._error = e
            self._ready.set()
            return
        self._ready.set()
        try:
            self._loop.run_forever()
        finally:
            self._loop.run_until_complete(self._shutdown())
            self._loop.close()

    async def _shutdown(self) -> None:
        self._server.close()
        for c in list(self._clients):
            c.writer.close()
        tasks = [t for t in asyncio.all_tasks() if t is not asyncio.current_task()]
        if tasks:
            _done, pending = await asyncio.wait(tasks, timeout=2.0)      # the handlers see their connection end
            for t in pending:
                t.cancel()

    async def _handshake(self, reader, writer) -> bool:
        try:
            head = await reader.readuntil(b"\r\n\r\n")
        except (asyncio.IncompleteReadError, asyncio.LimitOverrunError, ConnectionError):
            return False
        lines = head.decode("latin-1").split("\r\n")
        fields = {k.strip().lower(): v.strip() for k, colon, v in (ln.partition(":") for ln in lines[1:]) if colon}
        key = fields.get("sec-websocket-key")
        if not lines[0].startswith("GET ") or "websocket" not in fields.get("upgrade", "").lower() or not key:
            writer.write(b"HTTP/1.1 400 Bad Request\r\nConnection: close\r\nContent-Length: 0\r\n\r\n")
            return False
        writer.write(("HTTP/1.1 101 Switching Protocols\r\nUpgrade: websocket\r\nConnection: Upgrade\r\n"
                      f"Sec-WebSocket-Accept: {websocket_accept(key)}\r\n\r\n").encode("ascii"))
        return True

    async def _handle(self, reader, writer) -> None:
        client = _Client(writer)
        try:
            if not await self._handshake(reader, writer):
                return
            self._clients.add(client)
            message = bytearray()
            while True:
                b0, b1 = await reader.readexactly(2)
                opcode, n = b0 & 0x0F, b1 & 0x7F
                if n == 126:
                    n, = struct.unpack("!H", await reader.readexactly(2))
                elif n == 127:
                    n, = struct.unpack("!Q", await reader.readexactly(8))
                if not b1 & 0x80 or n + len(message) > _MAX_MESSAGE:     # unmasked client frame (1002) / too big (1009)
                    client.send(0x8, struct.pack("!H", 1009 if b1 & 0x80 else 1002))
                    return
                mask = await reader.readexactly(4)
                data = await reader.readexactly(n)
                data = bytes(c ^ mask[i & 3] for i, c in enumerate(data))
                if opcode == 0x8:                                         # close: echo the status code and leave
                    client.send(0x8, data[:2])
                    return
                if opcode == 0x9:
                    client.send(0xA, data)
                elif opcode in (0x0, 0x1):
                    message += data
                    if b0 & 0x80:
                        self._message(client, bytes(message))
                        message.clear()
        except (asyncio.IncompleteReadError, ConnectionError):
            pass
        finally:
            client.closed = True
            self._clients.discard(client)
            with self._lock:
                if self._mailbox is not None and self._mailbox[0] is client:
                    self._mailbox = None
            try:
                await writer.drain()
            except ConnectionError:
                pass
            writer.close()

    def _message(self, client, text: bytes) -> None:
        try:
            msg = json.loads(text.decode("utf-8"))
            kind = msg["type"]
        except (ValueError, KeyError, TypeError):
            client.send_json({"error": "expected a JSON object with a type"})
            return
        if kind == "cameraInfo":
            client.camera = copy.copy(getattr(self.renderer, "camera", None))             # :59-62
        elif kind == "renderRequest":
            if not (isinstance(msg.get("position"), list) and len(msg["position"]) == 3
                    and isinstance(msg.get("quat"), list) and len(msg["quat"]) == 4):
                client.send_json({"error": "renderRequest needs position [3] and quat [4]"})
                return
            with self._lock:
                self._mailbox = (client, msg)                                             # :74-77: the newer request stays
            self._wake.set()

    # ---- the thread that owns the GPU
    def service(self, *_unused) -> bool:
        """Renders the pending request, if there is one, and queues the answer for sending -> whether it rendered.
        Extra arguments are ignored, so the method itself serves as ``fit``'s ``on_step``."""
        with self._lock:
            pending, self._mailbox = self._mailbox, None
            self._wake.clear()
        if pending is None:
            return False
        client, msg = pending
        data = self.renderer.render_jpeg(msg["position"], msg["quat"], self.quality, self.subsampling)
        self.rendered += 1
        text = json.dumps({"image": base64.b64encode(data).decode("ascii")}).encode("ascii")
        self._loop.call_soon_threadsafe(client.send, 0x1, text)
        return True

    def run_forever(self, poll: float = 0.25) -> None:
        """Serves requests until ``stop()`` (from another thread) or KeyboardInterrupt."""
        try:
            while not self._stopping.is_set():
                self._wake.wait(poll)
                self.service()
        except KeyboardInterrupt:
            pass

    def stop(self) -> None:
        if self._stopping.is_set():
            return
        self._stopping.set()
        self._wake.set()
        if self._error is None:
            self._loop.call_soon_threadsafe(self._loop.stop)
        self._thread.join()
