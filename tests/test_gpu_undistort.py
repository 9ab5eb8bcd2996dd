"""The undistortion kernel (csrc/undistort.hip) against the float64 oracle of
tests/undistort_oracle.py, on the cases and with the tolerance of tests/undistort_cases.py: sources of uniform random
bytes, so that an error of e pixels in a source coordinate costs up to 255 e levels."""
import numpy as np
import pytest
import torch

import undistort_cases as UC
import undistort_oracle as UO
from tinysplat_amd.dataset import undistort_image

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _run(name, dtype):
    src, sk, dk, d, size = UC.cases()[name]
    out = undistort_image(torch.from_numpy(src).to(DEV), sk, dk, d, size, dtype=dtype)
    assert out.dtype == dtype and tuple(out.shape) == (size[1], size[0], 3) and out.is_contiguous()
    return out.cpu().numpy()


@pytest.mark.parametrize("name", list(UC.cases()))
def test_float_image_is_within_tau_of_the_oracle(name):
    got = _run(name, torch.float32).astype(np.float64) * 255.0
    err = float(np.abs(got - UC.oracle(name)).max())
    print(f"{name}: max |out 255 - oracle| = {err:.5f} levels (tau {UC.TAU})")
    assert err <= UC.TAU


@pytest.mark.parametrize("name", list(UC.cases()))
def test_byte_image_is_the_rounded_oracle(name):
    UO.check_uint8(_run(name, torch.uint8), UC.oracle(name), UC.TAU, name)


def test_byte_image_is_the_rounded_float_image():
    """Both outputs come from one value: the byte is rint(255 x the float) wherever 255 x the float32 quotient is not
    within a float32 rounding of a boundary."""
    for name in ("opencv", "opencv_max40", "opencv_5x3"):
        levels = _run(name, torch.float32).astype(np.float64) * 255.0
        UO.check_uint8(_run(name, torch.uint8), levels, 1e-4, f"{name} against its float image")


def test_undistorted_camera_in_reference_mode_returns_the_source_bytes():
    src, sk, dk, d, size = UC.cases()["none"]
    assert not np.any(d) and np.abs(sk - dk).max() < 1e-4 and size == UO.SIZE
    assert np.array_equal(_run("none", torch.uint8), src)
    same = undistort_image(torch.from_numpy(src).to(DEV), sk, sk, d, size)
    assert np.array_equal(same.cpu().numpy(), src)


def test_two_runs_are_bit_identical():
    for name in ("full", "opencv_max40", "opencv_257x130"):
        for dtype in (torch.uint8, torch.float32):
            assert np.array_equal(_run(name, dtype), _run(name, dtype)), (name, dtype)


def test_upscaling_and_a_sliced_source():
    """An output larger than the source takes one sample per pixel, and a non-contiguous source is made contiguous."""
    src, sk, dk, d, _ = UC.cases()["opencv"]
    big = UC.scale_intrinsics(dk, 2.0, 2.0)
    out = undistort_image(torch.from_numpy(src).to(DEV), sk, big, d, (194, 122), dtype=torch.float32)
    want = UO.remap(src, sk, big, d, (194, 122))
    assert float(np.abs(out.cpu().numpy().astype(np.float64) * 255 - want).max()) <= UC.TAU
    wide = torch.from_numpy(np.concatenate([src, src], axis=1)).to(DEV)[:, :UO.SIZE[0]]
    assert not wide.is_contiguous()
    assert np.array_equal(undistort_image(wide, sk, dk, d, UO.SIZE).cpu().numpy(), _run("opencv", torch.uint8))


def test_cpu_tensors_and_bad_arguments_are_refused():
    src, sk, dk, d, size = UC.cases()["opencv"]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        undistort_image(torch.from_numpy(src), sk, dk, d, size)
    img = torch.from_numpy(src).to(DEV)
    with pytest.raises(ValueError):
        undistort_image(img.float(), sk, dk, d, size)
    with pytest.raises(ValueError):
        undistort_image(img[:, :, :2], sk, dk, d, size)
    with pytest.raises(ValueError):
        undistort_image(img, sk, dk, d, size, dtype=torch.float16)
    with pytest.raises(ValueError):
        undistort_image(img, sk, dk, d, (0, 5))
    with pytest.raises(ValueError):
        undistort_image(img, sk, dk, list(d) + [0.0], size)
