"""The JPEG encoder on the GPU (csrc/jpeg.hip) against the host build of csrc/jpeg_math.h
(tests/hostmath/jpeg.cpp), which tests/test_jpeg_cpu.py holds against the float64 oracle and libjpeg: the same
coefficients and the same file, byte for byte, for every case, both subsamplings and restart intervals 1, 2 and one MCU
row."""
import numpy as np
import pytest
import torch

import jpeg_cases as JC
from tinysplat_amd import JpegEncoder, encode_jpeg
from tinysplat_amd.jpeg import jpeg_coefficients

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ALL = [(name, sub) for name in JC.CASES for sub in JC.SUBSAMPLINGS]
INTERVALS = (1, 2, None)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return JC.build_host(tmp_path_factory.mktemp("jpeg"))


@pytest.fixture(scope="module")
def expected(host):
    """name, subsampling -> (the host build's coefficients, {restart interval: its file}), computed once."""
    out = {}
    for name, sub in ALL:
        img, q, _ = JC.CASES[name]
        coef = JC.host_coefficients(host, img, q, sub)
        out[name, sub] = (coef, {ri: JC.host_encode(host, coef, img.shape[1], img.shape[0], q, sub, ri) for ri in INTERVALS})
    return out


@pytest.mark.parametrize("name,sub", ALL)
def test_coefficients_and_file_are_the_host_builds(expected, name, sub):
    img, q, _ = JC.CASES[name]
    coef, files = expected[name, sub]
    dev = torch.from_numpy(img).to(DEV)
    got = jpeg_coefficients(dev, q, sub)
    want = JC.split_components(coef, img.shape[1], img.shape[0], sub)
    for g, w, what in zip(got, want, "Y Cb Cr".split()):
        assert g.dtype == torch.int16 and tuple(g.shape) == w.shape and np.array_equal(g.cpu().numpy(), w), what
    for ri in INTERVALS:
        first = encode_jpeg(dev, q, sub, ri)
        assert first == files[ri], (ri, len(first), len(files[ri]))
        assert encode_jpeg(dev, q, sub, ri) == first                     # the same bytes on every run


@pytest.mark.parametrize("sub", JC.SUBSAMPLINGS)
def test_float_frame_with_a_stride_of_four_is_the_file_of_its_bytes(sub):
    rng = np.random.default_rng(11)
    frame = torch.from_numpy(rng.uniform(-0.05, 1.05, (70, 130, 4)).astype(np.float32)).to(DEV)
    frame[0, :64, 1] = (torch.arange(64, device=DEV) + 0.5) / 255           # ties: half to even, as torch rounds
    rgb = frame[:, :, :3]                                                   # a view: pixels 4 floats apart
    assert rgb.stride() == (520, 4, 1)
    u8 = (rgb * 255).clamp_(0, 255).round_().to(torch.uint8)               # ViewRenderer.render(as_uint8=True)
    want = encode_jpeg(u8, 90, sub)
    assert encode_jpeg(rgb, 90, sub) == want and encode_jpeg(rgb.contiguous(), 90, sub) == want
    # one encoder, many frames: the workspace and the buffers are reused
    enc = JpegEncoder(130, 70, 90, sub, device=DEV)
    assert enc.encode(rgb) == want and enc.encode(u8) == want and enc.encode(u8, quality=50) == encode_jpeg(u8, 50, sub)


def test_a_capacity_below_the_worst_case_is_refused():
    img = torch.from_numpy(JC.noise()).to(DEV)
    enc = JpegEncoder(40, 24, 90, "420", device=DEV)
    with pytest.raises(ValueError, match="TS_E_BADARG"):
        enc.launch(img, out_capacity=enc.capacity - 1)
    enc.launch(img, out_capacity=enc.capacity)
    assert enc.collect() == encode_jpeg(img, 90, "420")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        encode_jpeg(torch.from_numpy(JC.noise()), 90)


def test_more_blocks_and_segments_than_one_scan_workgroup(host):
    """264 x 264 at 4:4:4 with a restart interval of 1: 3 267 blocks in 1 089 segments, so both scans (1 024 entries per
    workgroup) add their workgroups' sums."""
    img = JC.waves(264, 264, seed=3)
    dev = torch.from_numpy(img).to(DEV)
    for sub in JC.SUBSAMPLINGS:
        coef = JC.host_coefficients(host, img, 90, sub)
        for ri in (1, None):
            assert encode_jpeg(dev, 90, sub, ri) == JC.host_encode(host, coef, 264, 264, 90, sub, ri), (sub, ri)
