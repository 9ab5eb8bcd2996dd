"""Training and evaluation masks without a GPU: where masks come from and the small operations on
them, the host build of csrc/mask_math.h against a float64 restatement, the new C entries' argument checks, and the
refusal in the sharded trainer."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import mask_cases as KC
from tinysplat_amd import TrainingMasks, combine_masks, dilate_ignored, mask_coverage, masks_from_labels
from tinysplat_amd.masks import as_mask, mask_weights


def _dataset(names, h=12, w=16):
    return SimpleNamespace(cameras=[SimpleNamespace(name=n, height=h, width=w) for n in names])


def _png(path, array):
    from PIL import Image
    Image.fromarray(array).save(path)


def test_file_names_precedence_and_nonzero_means_keep(tmp_path):
    """<image name>.png before <stem>.png before <image name>.npy; any nonzero value keeps the pixel."""
    h, w = 12, 16
    a = np.zeros((h, w), np.uint8)
    a[:, :5] = 1                                        # nonzero, not 255
    b = np.zeros((h, w), np.uint8)
    b[:3] = 200
    c = np.zeros((h, w), np.int64)
    c[5, 7] = -4
    rgb = np.zeros((h, w, 3), np.uint8)
    rgb[2, 3, 1] = 9                                    # one channel nonzero
    _png(tmp_path / "a.jpg.png", a)
    _png(tmp_path / "a.png", b)                         # loses to a.jpg.png
    np.save(tmp_path / "a.jpg.npy", c)
    _png(tmp_path / "b.png", b)                         # the stem's file: b.jpg has no b.jpg.png
    np.save(tmp_path / "b.jpg.npy", c)
    np.save(tmp_path / "c.jpg.npy", c)
    _png(tmp_path / "d.png.png", rgb)
    masks = TrainingMasks(_dataset(["a.jpg", "b.jpg", "c.jpg", "d.png"], h, w), tmp_path, device="cpu")
    assert len(masks) == 4 and [f.rsplit("/", 1)[-1] for f in masks.files] == ["a.jpg.png", "b.png", "c.jpg.npy", "d.png.png"]
    for got, src in zip(masks, (a, b, c, rgb.any(axis=2))):
        assert got.dtype == torch.uint8 and got.shape == (h, w)
        assert np.array_equal(got.numpy(), np.where(src != 0, 255, 0).astype(np.uint8))


def test_missing_files_are_listed_and_a_wrong_size_is_refused(tmp_path):
    _png(tmp_path / "a.jpg.png", np.full((12, 16), 255, np.uint8))
    with pytest.raises(FileNotFoundError, match=r"no mask in .* for: b\.jpg, c\.jpg"):
        TrainingMasks(_dataset(["a.jpg", "b.jpg", "c.jpg"]), tmp_path, device="cpu")
    _png(tmp_path / "b.jpg.png", np.full((12, 15), 255, np.uint8))
    with pytest.raises(ValueError, match="fits neither size"):
        TrainingMasks(_dataset(["a.jpg", "b.jpg"]), tmp_path, device="cpu")
    # the photo's size alone does not do where the photo was not resampled: the camera's size is the file's then
    ds = _dataset(["b.jpg"])
    ds.setups, ds.source_sizes = [SimpleNamespace(resample=False)], [(15, 12)]
    with pytest.raises(ValueError, match="fits neither size"):
        TrainingMasks(ds, tmp_path, device="cpu")


def _min_filter(mask, radius):
    h, w = mask.shape
    out = np.empty_like(mask)
    for y in range(h):
        for x in range(w):
            out[y, x] = mask[max(0, y - radius):y + radius + 1, max(0, x - radius):x + radius + 1].min()
    return out


@pytest.mark.parametrize("radius", [0, 1, 3, 10, 40])
def test_dilate_ignored_is_a_minimum_filter(radius):
    """Against a numpy minimum filter cut at the border, soft bytes included; radius 0 is the identity, a radius larger
    than the image (40 > 23 x 31) spreads the smallest byte everywhere."""
    g = np.random.default_rng(radius)
    mask = np.full((23, 31), 255, np.uint8)
    mask[g.integers(0, 23, 6), g.integers(0, 31, 6)] = g.integers(0, 255, 6)
    got = dilate_ignored(torch.from_numpy(mask), radius)
    assert got.dtype == torch.uint8 and np.array_equal(got.numpy(), _min_filter(mask, radius))
    if radius == 0:
        assert np.array_equal(got.numpy(), mask)
    if radius == 40:
        assert np.all(got.numpy() == mask.min())
    with pytest.raises(ValueError):
        dilate_ignored(torch.from_numpy(mask), -1)


def test_masks_from_labels():
    labels = np.array([[0, 1, 2, 3], [255, 2, 2, 0], [4, 4, 1, 255]], np.uint8)
    maps = SimpleNamespace(maps=[torch.from_numpy(labels), torch.from_numpy(labels.T.copy())], num_classes=5)
    got = masks_from_labels(maps, [2, 4])
    want = np.where(np.isin(labels, (2, 4)), 0, 255).astype(np.uint8)         # the ignore label (255) is kept
    assert np.array_equal(got[0].numpy(), want) and np.array_equal(got[1].numpy(), want.T)
    assert want[1, 0] == 255 and want[0, 2] == 0
    grown = masks_from_labels(maps, [2, 4], dilate=1)
    assert np.array_equal(grown[0].numpy(), _min_filter(want, 1))
    assert np.all(masks_from_labels(maps, [])[0].numpy() == 255)
    with pytest.raises(ValueError):
        masks_from_labels(maps, [5])


def test_combine_coverage_and_bool_input():
    a = torch.tensor([[255, 0, 100], [7, 255, 255]], dtype=torch.uint8)
    b = torch.tensor([[255, 255, 50], [200, 0, 255]], dtype=torch.uint8)
    assert torch.equal(combine_masks(a, b), torch.tensor([[255, 0, 50], [7, 0, 255]], dtype=torch.uint8))
    assert mask_coverage(a) == pytest.approx((255 + 0 + 100 + 7 + 255 + 255) / 6 / 255)
    assert mask_coverage(torch.zeros(3, 3, dtype=torch.uint8)) == 0.0 and mask_coverage(torch.ones(3, 3, dtype=torch.bool)) == 1.0
    keep = torch.tensor([[True, False], [False, True]])
    assert torch.equal(as_mask(keep), torch.tensor([[255, 0], [0, 255]], dtype=torch.uint8))
    assert torch.equal(combine_masks(keep, torch.full((2, 2), 9, dtype=torch.uint8)), torch.tensor([[9, 0], [0, 9]], dtype=torch.uint8))
    w = mask_weights(a)
    assert w.dtype == torch.float32 and w[0, 0] == 1.0 and w[0, 1] == 0.0 and w[0, 2] == np.float32(100) / np.float32(255)
    for bad in (torch.zeros(3, 3), torch.zeros(3, dtype=torch.uint8), torch.zeros(2, 2, 3, dtype=torch.uint8)):
        with pytest.raises(ValueError):
            as_mask(bad)
    with pytest.raises(ValueError):
        combine_masks(a, b[:, :2])


def test_host_build_of_mask_math_against_a_float64_restatement(tmp_path):
    """The weights are the correctly rounded quotients; the blend is within one float32 ulp of the float64 restatement
    (the fused multiply-add rounds once, the restatement twice), and exact where the byte is 0 (the target) and 255 (the
    image)."""
    lib = KC.build_host(tmp_path)
    table = np.array([lib.kh_weight(b) for b in range(256)], np.float32)
    assert np.array_equal(table, np.arange(256, dtype=np.float32) / np.float32(255.0)) and table[0] == 0.0 and table[255] == 1.0
    for h, w in KC.SHAPES:
        frame, tgt, _ = KC.inputs(h, w)
        image = frame[:, :, :3].contiguous()
        for name, mask in KC.masks(h, w).items():
            got = KC.host_blend(lib, image, tgt, mask).numpy()
            ref = KC.blend_restatement(image, tgt, mask)
            assert np.all(np.abs(got.astype(np.float64) - ref.astype(np.float64)) <= np.spacing(np.abs(ref))), (h, w, name)
            m = mask.numpy()
            assert np.array_equal(got[m == 0], tgt.numpy()[m == 0]) and np.array_equal(got[m == 255], image.numpy()[m == 255])
    # images far from [0, 1] too: 0 and 255 stay exact
    g = torch.Generator().manual_seed(5)
    x, y = 1e3 * torch.randn(9, 13, 3, generator=g), 1e-3 * torch.randn(9, 13, 3, generator=g)
    mask = torch.randint(0, 256, (9, 13), generator=g).to(torch.uint8)
    mask[0, :6], mask[1, :6] = 0, 255
    got, ref = KC.host_blend(lib, x, y, mask).numpy(), KC.blend_restatement(x, y, mask)
    assert np.all(np.abs(got.astype(np.float64) - ref.astype(np.float64)) <= np.spacing(np.abs(ref)))
    assert np.array_equal(got[0, :6], y.numpy()[0, :6]) and np.array_equal(got[1, :6], x.numpy()[1, :6])


def test_argument_errors_of_the_masked_entries_without_a_gpu():
    from tinysplat_amd import _lib
    lib = _lib.load()
    f, b, d = (ctypes.c_float * 4)(), (ctypes.c_uint8 * 4)(), (ctypes.c_double * 8)()
    P = lambda a: ctypes.cast(a, ctypes.c_void_p).value     # noqa: E731

    def refused(**fields):
        """the entry's answer to a descriptor that is sound (64 x 64, 3 floats, image, target and workspace set) but for
        ``fields``"""
        loss = _lib.TsLoss(**{**dict(height=64, width=64, pixel_floats=3, image=P(f), target=P(f), w_l1=0.1, w_ssim=-0.1,
                                     ws=P(f)), **fields})
        return lib.ts_photometric_loss_rgbd(ctypes.byref(loss), None) == -1
    masked = dict(flags=_lib.LOSS_MASKED, mask=P(b))
    rgbd, planes = dict(pixel_floats=4), dict(depth=P(f))
    assert lib.ts_photometric_loss_rgbd(None, None) == -1                                    # no descriptor
    # the mask and its flag come together; no other flag bit exists
    assert refused(flags=_lib.LOSS_MASKED) and refused(**rgbd, flags=_lib.LOSS_MASKED)
    assert refused(**planes, flags=_lib.LOSS_MASKED)
    assert refused(mask=P(b)) and refused(**rgbd, mask=P(b)) and refused(**planes, mask=P(b))
    assert refused(flags=2) and refused(**{**masked, "flags": 3}) and refused(flags=-2)
    # H or W <= 10, a null image, target or workspace, floats per pixel other than 3 or 4: with and without the mask
    for more in ({}, masked):
        assert refused(height=10, **more) and refused(width=10, **more)
        assert refused(height=8, **rgbd, **more) and refused(width=9, **planes, **more)
        assert refused(image=None, **more) and refused(target=None, **more) and refused(ws=None, **more)
        assert refused(pixel_floats=5, **more) and refused(pixel_floats=2, **more)
        # a depth target needs a rendered depth: the fourth channel or the plane, and never both
        assert refused(depth_target=P(f), w_depth=0.1, **more)
        assert refused(**rgbd, **planes, **more)
        # the depth plane's gradient needs the plane, and the image's gradient beside it
        assert refused(v_image=P(f), v_depth=P(f), **more) and refused(**rgbd, v_image=P(f), v_depth=P(f), **more)
        assert refused(**planes, v_depth=P(f), **more)
    assert lib.ts_mask_blend(64, 64, f, f, None, f, None) == -1 and lib.ts_mask_blend(0, 64, f, f, b, f, None) == -1
    assert lib.ts_mask_blend(64, 64, f, f, b, None, None) == -1
    # the metrics entry: a null mask, small sizes, and a row whose byte offsets do not fit 32 bits
    assert lib.ts_image_metrics_masked(64, 64, 3, f, f, 0, None, d, d, None) == -1
    assert lib.ts_image_metrics_masked(10, 64, 3, f, f, 0, b, d, d, None) == -1
    assert lib.ts_image_metrics_masked(64, 64, 2, f, f, 0, b, d, d, None) == -1
    assert lib.ts_image_metrics_masked(64, (1 << 27) + 1, 3, f, f, 1, b, d, d, None) == -1
    assert lib.ts_image_metrics_masked_ws_bytes(10, 64) == 0
    for h, w in ((11, 11), (96, 128), (1080, 1920)):
        assert lib.ts_image_metrics_masked_ws_bytes(h, w) * 3 == lib.ts_image_metrics_ws_bytes(h, w) * 5


def test_python_entries_refuse_bad_masks_before_any_launch():
    """The wrappers' own checks need no GPU either: a mask of the wrong type, and CPU tensors altogether."""
    from tinysplat_amd.metrics import image_metrics
    from tinysplat_amd.training import photometric_loss
    img = torch.zeros(20, 20, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        photometric_loss(img, img, 0.2, mask=torch.ones(20, 20, dtype=torch.bool))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        image_metrics(img, img, mask=torch.ones(20, 20, dtype=torch.bool))


def test_the_sharded_trainer_refuses_masks():
    from tinysplat_amd.sharded import render_sharded
    with pytest.raises(ValueError, match="sharded trainer does not take masks"):
        render_sharded(None, None, "cpu", None, None, mask=torch.ones(4, 4, dtype=torch.uint8))
