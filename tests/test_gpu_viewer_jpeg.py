"""A viewer request as a JPEG encoded on the GPU (ViewRenderer.render_jpeg, Viewer) on the golden
256 x 256 scene."""
import base64
import io
import json

import numpy as np
import pytest
import torch
from PIL import Image

import jpeg_oracle as JO
from test_golden import load_case
from ws_client import Client
from tinysplat_amd import Viewer, encode_jpeg
from tinysplat_amd.jpeg import jpeg_coefficients
from tinysplat_amd.viewer import ViewRenderer

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
POSE = ([0.3, -0.2, -1.0], [1.0, 0.0, 0.0, 0.0])


@pytest.fixture(scope="module")
def renderer():
    _, model, cam, _ = load_case("frame_n1000_sh3_256")
    return ViewRenderer(model.to(DEV), cam, DEV)


def test_render_jpeg_is_the_file_of_the_uint8_frame(renderer):
    data = renderer.render_jpeg(*POSE)
    im = Image.open(io.BytesIO(data))
    im.load()
    assert im.size == (256, 256) and im.mode == "RGB"
    u8 = renderer.render(*POSE, as_uint8=True).copy()
    assert u8.std() > 10                                                 # a picture, not a blank frame
    dev_u8 = torch.from_numpy(u8).to(DEV)
    for sub in ("420", "444"):
        frame = renderer._frame(*POSE)
        for a, b in zip(jpeg_coefficients(frame, 90, sub), jpeg_coefficients(dev_u8, 90, sub)):
            assert torch.equal(a, b)
        assert renderer.render_jpeg(*POSE, 90, sub) == encode_jpeg(dev_u8, 90, sub)
    assert data == encode_jpeg(dev_u8, 90, "420")
    # against libjpeg's own file at the same quality and subsampling, both decoded by libjpeg
    buf = io.BytesIO()
    Image.fromarray(u8).save(buf, format="JPEG", quality=90, subsampling=2, optimize=False)
    theirs = Image.open(io.BytesIO(buf.getvalue()))
    deficit = JO.psnr(np.asarray(theirs), u8) - JO.psnr(np.asarray(im), u8)
    print(f"PSNR deficit against libjpeg's own file {deficit:.3f} dB, {len(data)} against {len(buf.getvalue())} bytes")
    assert deficit <= 0.25


def test_a_request_through_the_server_returns_that_file(renderer):
    viewer = Viewer(renderer, ip="127.0.0.1", port=0)
    try:
        client = Client(viewer.port)
        client.send_json({"type": "cameraInfo"})
        client.send_json({"type": "renderRequest", "position": POSE[0], "quat": POSE[1]})
        assert viewer._wake.wait(10) and viewer.service()
        opcode, payload, _ = client.recv()
        client.close()
    finally:
        viewer.stop()
    assert opcode == 0x1 and base64.b64decode(json.loads(payload)["image"]) == renderer.render_jpeg(*POSE)
