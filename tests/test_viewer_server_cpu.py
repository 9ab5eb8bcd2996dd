"""The viewer's websocket server without a GPU (tinysplat_amd/viewer.py: Viewer): a client written from socket, hashlib
and base64 (tests/ws_client.py) talks to a Viewer around a stub renderer on the loopback interface."""
import base64
import hashlib
import inspect
import json
import struct

import pytest

from ws_client import Client
from tinysplat_amd import Viewer
from tinysplat_amd.training import fit


class StubRenderer:
    """Answers a request with bytes that name its pose; the length comes from the first coordinate."""
    camera = {"template": True}

    def __init__(self):
        self.calls = []

    def render_jpeg(self, position, quat, quality=90, subsampling="420"):
        self.calls.append((list(position), list(quat), quality, subsampling))
        return (json.dumps([position, quat]).encode() + b"\xff\xd9") * max(1, int(position[0]))


@pytest.fixture()
def served():
    stub = StubRenderer()
    viewer = Viewer(stub, ip="127.0.0.1", port=0, quality=77, subsampling="444")
    client = Client(viewer.port)
    yield viewer, stub, client
    client.close()
    viewer.stop()


def _request(x, tag=0.0):
    return {"type": "renderRequest", "position": [x, tag, 2.0], "quat": [1.0, 0.0, 0.0, 0.0]}


def _serve(viewer, n=1):
    """Waits for a request to arrive (the wake-up event, no sleep) and renders it."""
    done = 0
    while done < n:
        assert viewer._wake.wait(10)
        done += viewer.service()


def test_handshake_accept_key(served):
    viewer, _, client = served
    want = base64.b64encode(hashlib.sha1(client.key.encode() + b"258EAFA5-E914-47DA-95CA-C5AB0DC85B11").digest()).decode()
    assert client.status.startswith("HTTP/1.1 101") and client.fields["sec-websocket-accept"] == want
    assert client.fields["upgrade"].lower() == "websocket" and viewer.port != 0
    # the example of RFC 6455 section 1.3
    from tinysplat_amd.viewer import websocket_accept
    assert websocket_accept("dGhlIHNhbXBsZSBub25jZQ==") == "s3pPLMBiTxaQ9kYGzzhZRbK+xOo="


def test_short_and_long_answers_use_the_16_and_64_bit_lengths(served):
    viewer, stub, client = served
    client.send_json({"type": "cameraInfo"})
    assert not viewer.service()                                  # cameraInfo alone renders nothing
    for x, form in ((10.0, 16), (1500.0, 64)):
        client.send_json(_request(x))
        _serve(viewer)
        opcode, payload, got = client.recv()
        data = base64.b64decode(json.loads(payload)["image"])
        assert opcode == 0x1 and got == form and data == stub.render_jpeg([x, 0.0, 2.0], [1.0, 0.0, 0.0, 0.0])
        assert (len(payload) > 65535) == (form == 64)
    assert stub.calls[0][2:] == (77, "444")
    # a client may use the long forms for a short message too
    client.send_json(_request(1.0, 16.0), length_form=16)
    _serve(viewer)
    assert json.loads(base64.b64decode(json.loads(client.recv()[1])["image"])[:-2])[0][1] == 16.0
    client.send_json(_request(1.0, 64.0), length_form=64)
    _serve(viewer)
    assert json.loads(base64.b64decode(json.loads(client.recv()[1])["image"])[:-2])[0][1] == 64.0


def test_ping_is_answered_with_pong(served):
    _, _, client = served
    client.send(0x9, b"are you there")
    assert client.recv() == (0xA, b"are you there", 7)


def test_close_handshake(served):
    _, _, client = served
    client.send(0x8, struct.pack("!H", 1000) + b"bye")
    opcode, payload, _ = client.recv()
    assert opcode == 0x8 and payload == struct.pack("!H", 1000)
    with pytest.raises(ConnectionError):
        client._read(1)                                          # the server closed the connection behind its close frame


def test_a_newer_request_evicts_the_pending_one(served):
    viewer, stub, client = served
    client.send_json(_request(1.0, 1.0))
    client.send_json(_request(1.0, 2.0))
    client.send(0x9, b"")                                        # the pong says both requests have been read
    assert client.recv()[0] == 0xA
    assert viewer.service() and not viewer.service()
    assert [c[0][1] for c in stub.calls] == [2.0] and viewer.rendered == 1
    assert json.loads(base64.b64decode(json.loads(client.recv()[1])["image"])[:-2])[0][1] == 2.0


def test_malformed_messages_get_an_error_and_unmasked_frames_a_close(served):
    viewer, _, client = served
    client.send(0x1, b"not json")
    assert "error" in json.loads(client.recv()[1])
    client.send_json({"type": "renderRequest", "position": [1, 2]})
    assert "error" in json.loads(client.recv()[1]) and not viewer.service()
    client.sock.sendall(struct.pack("!BB", 0x81, 2) + b"hi")     # unmasked
    opcode, payload, _ = client.recv()
    assert opcode == 0x8 and payload == struct.pack("!H", 1002)


def test_fit_on_step_defaults_to_none():
    assert inspect.signature(fit).parameters["on_step"].default is None
