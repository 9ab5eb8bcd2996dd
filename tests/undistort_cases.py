"""The resampling cases that the CPU and GPU tests of the undistortion kernel share, and the
tolerance that goes with them.  Sources are uniform random bytes: neighbouring pixels differ by up to 255 levels, so an
error of e pixels in a source coordinate shows as up to 255 e levels."""
import functools

import numpy as np

import undistort_oracle as UO

# the largest difference between the oracle run in float32 and in float64 over the cases below, in levels, and the
# tolerance of the float32 image: 4 x that, room for another legal order of the float32 operations.  Both are pinned by
# tests/test_undistort_cpu.py::test_tolerance_is_four_times_the_float32_error.
F32_ERROR = 0.0045
TAU = 4 * F32_ERROR


def scale_intrinsics(k, sx, sy):
    """intrinsics in pixel indices of the same camera on a frame sx, sy times the size"""
    return np.array([k[0] * sx, k[1] * sy, (k[2] + 0.5) * sx - 0.5, (k[3] + 0.5) * sy - 0.5])


def _source(w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (src uint8 [H,W,3], src_k, dst_k, d, (out_w, out_h)); intrinsics as float32 values"""
    w, h = UO.SIZE
    out = {}
    for seed, (name, (k, d)) in enumerate(UO.CAMERAS.items()):
        out[name] = (_source(w, h, seed), k, UO.new_matrix_reference(k, d, w, h), d, (w, h))
    k, d = UO.CAMERAS["opencv"]
    for max_dim in (40, 96):                                     # 40 x 25 with n = 3, 96 x 60 with n = 2
        size, dst = UO.scaled(UO.new_matrix_center(k, d, w, h), w, h, max_dim)
        out[f"opencv_max{max_dim}"] = (_source(w, h, 10 + max_dim), k, dst, d, size)
    for sw, sh in ((5, 3), (257, 130)):                          # 15 pixels: below a wave, a tail of 3; 33 workgroups
        ks = scale_intrinsics(k, sw / w, sh / h)
        out[f"opencv_{sw}x{sh}"] = (_source(sw, sh, sw), ks, UO.new_matrix_reference(ks, d, sw, sh), d, (sw, sh))
    return {name: (src, *UO.as_kernel_inputs(sk, dk, d), size) for name, (src, sk, dk, d, size) in out.items()}


@functools.lru_cache(maxsize=None)
def oracle(name):
    """the float64 image of a case in levels, computed once"""
    src, sk, dk, d, size = cases()[name]
    levels = UO.remap(src, sk, dk, d, size, np.float64)
    levels.setflags(write=False)
    return levels
