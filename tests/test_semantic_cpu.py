"""Label votes without a GPU: the host build of csrc/vote_math.h against numpy, SemanticMaps'
file handling, the export tool's argument errors and the argument errors of the two C entries."""
import ctypes
import importlib.util
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(Path(__file__).resolve().parent))

import semantic_cases as SC  # noqa: E402
import semantic_oracle as SO  # noqa: E402
from tinysplat_amd import semantic as S  # noqa: E402


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return SC.build_host(tmp_path_factory.mktemp("votes_host"))


# ------------------------------------------------------------------------------------------------------ the host build
def test_host_quantisation_is_rint_of_the_exact_product(host):
    r = np.random.default_rng(0)
    w = np.concatenate([r.random(4000, dtype=np.float32), r.random(2000, dtype=np.float32) * np.float32(1e-6),
                        np.array([0.0, 2.0 ** -25, 2.0 ** -24, 1.5 * 2.0 ** -24, 2.5 * 2.0 ** -24, 3.5 * 2.0 ** -24,
                                  np.nextafter(np.float32(2.0 ** -25), np.float32(1)), 0.5,
                                  np.nextafter(np.float32(1), np.float32(0))], dtype=np.float32)])
    got = np.array([host.vh_quantise(float(v)) for v in w], dtype=np.int64)
    assert np.array_equal(got, SO.quantise(w))
    # half-way cases go to the even integer, and the largest weight stays below 2^24
    assert host.vh_quantise(2.0 ** -25) == 0 and host.vh_quantise(1.5 * 2.0 ** -24) == 2 and host.vh_quantise(2.5 * 2.0 ** -24) == 2
    assert host.vh_quantise(float(np.nextafter(np.float32(1), np.float32(0)))) == (1 << 24) - 1


@pytest.mark.parametrize("min_share", SC.MIN_SHARES)
def test_host_labels_against_numpy(host, min_share):
    rows = SC.vote_rows()
    labels, conf, top, total = SC.host_labels(host, rows, min_share)
    want = SO.labels_from_votes(rows, min_share)
    assert np.array_equal(labels, want[0]) and conf.tobytes() == want[1].tobytes()
    assert np.array_equal(top, want[2]) and np.array_equal(total, want[3])


def test_host_label_rule_edges(host):
    rows = SC.vote_rows()
    labels, conf, _, _ = SC.host_labels(host, rows, 0.25)
    assert labels[1] == 1 and labels[2] == 0                      # ties go to the smaller column
    assert labels[4] == 255 and conf[4] == 0.0                    # an empty row
    assert labels[5] == 0 and conf[5] == np.float32(0.25)         # top == min_share * total exactly: kept
    labels, _, _, _ = SC.host_labels(host, rows, 0.375)
    assert labels[7] == 1 and labels[6] == 255 and labels[5] == 255          # 3/8 kept at 0.375, 1/3 and 1/4 not
    r = np.random.default_rng(1)
    big = r.integers(0, 1 << 40, size=(500, 150))
    big[r.random(500) < 0.1] = 0
    for share in (0.0, 0.01, 0.02):
        got = SC.host_labels(host, big, share)
        want = SO.labels_from_votes(big, share)
        assert np.array_equal(got[0], want[0]) and got[1].tobytes() == want[1].tobytes()


# ------------------------------------------------------------------------------------------------------- SemanticMaps
def _cams(sizes):
    return [SC.camera(w, h, name=f"img{i:02d}.jpg") for i, (w, h) in enumerate(sizes)]


def test_maps_round_trip_the_references_files(tmp_path):
    cams = _cams([(20, 12), (20, 12)])
    r = np.random.default_rng(2)
    stored = []
    for c in cams:
        m = r.integers(0, 150, size=(12, 20))
        m[r.random((12, 20)) < 0.1] = 255
        np.save(tmp_path / (c.name + ".npy"), torch.from_numpy(m))           # int64 [H, W], as semantic.py:33 writes it
        stored.append(m)
    maps = S.SemanticMaps(cams, tmp_path, device="cpu")
    assert len(maps) == 2 and maps.num_columns == 150 and maps.class_ids == list(range(150))
    for got, want in zip(maps.maps, stored):
        assert got.dtype == torch.uint8 and np.array_equal(got.numpy(), want.astype(np.uint8))
    assert np.array_equal(maps.class_map.numpy(), SC.identity_map(150))
    # another integer dtype, a singleton axis and an ignore label of its own
    np.save(tmp_path / (cams[0].name + ".npy"), np.where(stored[0] == 255, -1, stored[0]).astype(np.int16)[None])
    again = S.SemanticMaps(cams[:1], tmp_path, ignore_label=-1, device="cpu")
    assert np.array_equal(again.maps[0].numpy(), stored[0].astype(np.uint8))


def test_maps_refuse_bad_files_by_name(tmp_path):
    cams = _cams([(8, 6)])
    path = tmp_path / (cams[0].name + ".npy")
    with pytest.raises(FileNotFoundError, match="img00.jpg"):
        S.SemanticMaps(cams, tmp_path, device="cpu")
    good = np.zeros((6, 8), np.int64)
    for bad, what in ((np.where(np.eye(6, 8) > 0, 150, 0), "150"), (np.full((6, 8), -3), "-3"),
                      (np.zeros((2, 6, 8), np.int64), "rows, columns"), (np.zeros(48, np.int64), "rows, columns"),
                      (np.zeros((6, 8), np.float32), "integers")):
        np.save(path, bad)
        with pytest.raises(ValueError, match="img00.jpg") as e:
            S.SemanticMaps(cams, tmp_path, device="cpu")
        assert what in str(e.value)
    np.save(path, good)
    assert len(S.SemanticMaps(cams, tmp_path, device="cpu")) == 1
    np.save(path, np.array([{"a": 1}], dtype=object), allow_pickle=True)      # pickles are not loaded
    with pytest.raises(ValueError):
        S.SemanticMaps(cams, tmp_path, device="cpu")


@pytest.mark.parametrize("src,dst", [((6, 8), (12, 16)), ((12, 16), (6, 8)), ((7, 5), (10, 13)), ((10, 13), (3, 4)),
                                     ((1, 1), (4, 5))])
def test_maps_resample_nearest_at_pixel_centres(tmp_path, src, dst):
    r = np.random.default_rng(3)
    m = r.integers(0, 10, size=src)
    cams = _cams([(dst[1], dst[0])])
    np.save(tmp_path / (cams[0].name + ".npy"), m)
    got = S.SemanticMaps(cams, tmp_path, num_classes=10, device="cpu").maps[0].numpy()
    rows = np.floor((np.arange(dst[0]) + 0.5) * src[0] / dst[0]).astype(int)
    cols = np.floor((np.arange(dst[1]) + 0.5) * src[1] / dst[1]).astype(int)
    assert np.array_equal(got, m[rows][:, cols].astype(np.uint8))


def test_classes_build_the_class_map(tmp_path):
    cams = _cams([(8, 6)])
    np.save(tmp_path / (cams[0].name + ".npy"), np.zeros((6, 8), np.int64))
    maps = S.SemanticMaps(cams, tmp_path, num_classes=20, classes=[7, 2, 19], device="cpu")
    want = np.full(256, 255, np.uint8)
    want[7], want[2], want[19] = 0, 1, 2
    assert np.array_equal(maps.class_map.numpy(), want) and maps.num_columns == 3 and maps.class_ids == [7, 2, 19]
    for bad in ([], [20], [-1], [3, 3]):
        with pytest.raises(ValueError):
            S.SemanticMaps(cams, tmp_path, num_classes=20, classes=bad, device="cpu")
    with pytest.raises(ValueError):
        S.SemanticMaps(cams, tmp_path, num_classes=256, device="cpu")


def test_label_iou_is_a_numpy_count():
    r = np.random.default_rng(4)
    pred = r.integers(0, 6, size=(30, 40)).astype(np.uint8)
    target = r.integers(0, 5, size=(30, 40)).astype(np.uint8)
    pred[r.random(pred.shape) < 0.1] = 255
    target[r.random(pred.shape) < 0.2] = 255
    target[target == 3] = 2                                         # class 3 never occurs in the target
    iou, mean = S.label_iou(torch.from_numpy(pred), torch.from_numpy(target), 7)
    want, want_mean = SO.iou(pred, target, 7)
    assert np.array_equal(iou.numpy(), want, equal_nan=True)        # quotients of integer counts: correctly rounded
    assert abs(mean - want_mean) < 1e-12                            # (the mean's summation order is the library's)
    assert np.isnan(want[6]) and not np.isnan(want[3]) and want[3] == 0.0


# ------------------------------------------------------------------------------------------------------------ the tools
def _tool(name):
    spec = importlib.util.spec_from_file_location(f"tool_{name}", str(ROOT / "tools" / f"{name}.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_export_tool_semantic_flags(capsys):
    tool = _tool("export")
    a = tool.parse(["in.ply", "out.ply", "--filetype", "PLY"])
    assert (a.semantic_dir, a.keep_classes, a.drop_classes, a.min_share) == (None, None, None, 0.0)
    a = tool.parse(["in.ply", "out.ply", "--filetype", "PLY", "--dataset-dir", "d", "--semantic-dir", "d/semantic",
                    "--keep-classes", "19,3", "--min-share", "0.5"])
    assert (a.semantic_dir, a.keep_classes, a.drop_classes, a.min_share) == ("d/semantic", [19, 3], None, 0.5)
    a = tool.parse(["in.ply", "o.splat", "--filetype", "SPLAT", "--dataset-dir", "d", "--semantic-dir", "s",
                    "--drop-classes", "2"])
    assert a.drop_classes == [2] and a.keep_classes is None
    base = ["in.ply", "out.ply", "--filetype", "PLY"]
    for bad, message in ((["--semantic-dir", "s", "--keep-classes", "1"], "--semantic-dir needs --dataset-dir"),
                         (["--dataset-dir", "d", "--semantic-dir", "s", "--keep-classes", "1", "--drop-classes", "2"],
                          "exclude each other"),
                         (["--dataset-dir", "d", "--semantic-dir", "s"], "--keep-classes or --drop-classes"),
                         (["--keep-classes", "1"], "--semantic-dir goes with"),
                         (["--dataset-dir", "d", "--semantic-dir", "s", "--keep-classes", "150"], "outside"),
                         (["--dataset-dir", "d", "--semantic-dir", "s", "--keep-classes", "1,x"], "class numbers"),
                         (["--dataset-dir", "d", "--semantic-dir", "s", "--keep-classes", "1", "--min-share", "1.5"],
                          "--min-share"),
                         (["--min-share", "0.5"], "--min-share goes with")):
        with pytest.raises(SystemExit) as e:
            tool.parse(base + bad)
        assert e.value.code != 0 and message in capsys.readouterr().err
    assert "--semantic-dir" in tool.__doc__ and "--keep-classes" in tool.__doc__


def test_eval_tool_semantic_flags():
    tool = _tool("eval")
    a = tool.parse(["scene.ply", "--dataset-dir", "d"])
    assert (a.semantic_dir, a.semantic_classes, a.min_share) == (None, 150, 0.0)
    a = tool.parse(["scene.ply", "--dataset-dir", "d", "--semantic-dir", "d/semantic", "--semantic-classes", "21"])
    assert (a.semantic_dir, a.semantic_classes) == ("d/semantic", 21)
    with pytest.raises(SystemExit):
        tool.parse(["scene.ply", "--dataset-dir", "d", "--semantic-classes", "256"])


# ----------------------------------------------------------------------------------------------------- the C entries
def test_entries_refuse_bad_arguments_without_a_gpu():
    from tinysplat_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_int64 * 512)()
    p = ctypes.addressof(buf)

    def cam(w=50, h=37, wide=0, tbx=None, rows=None):
        tby = (h + 15) // 16
        return _lib.TsCamera(0.0, 0.0, 0.0, 0.0, w, h, (w + 15) // 16 if tbx is None else tbx, tby, 0,
                             tby if rows is None else rows, 1.0, 0.01, wide, 0)

    def votes(c, flags=0, num_classes=3, ptrs=(p, p, p, p, p, p)):
        return lib.ts_label_votes(flags, c, ptrs[0], ptrs[1], ptrs[2], ptrs[3], ptrs[4], num_classes, ptrs[5], None)

    assert votes(None) == -1                                         # no camera
    assert votes(cam(wide=1)) == -1                                  # wide tile lists
    assert votes(cam(), flags=1) == -1
    for c in (0, -1, 256):
        assert votes(cam(), num_classes=c) == -1
    assert votes(cam(), ptrs=(p, p, p, None, p, p)) == -1            # a class map without labels
    assert votes(cam(), ptrs=(p, p, p, p, None, p)) == -1            # labels without a class map
    for missing in (0, 1, 2, 5):                                     # tile_bins, ids, records, votes
        ptrs = [p] * 6
        ptrs[missing] = None
        assert votes(cam(), ptrs=tuple(ptrs)) == -1
    assert votes(cam(w=0)) == -1 and votes(cam(h=0)) == -1
    assert votes(cam(tbx=5)) == -1 and votes(cam(rows=4)) == -1     # tile bounds that are not the image's
    assert votes(cam(rows=0)) == 0                                   # no tiles: nothing to do

    def labels(n=4, num_classes=3, share=0.0, ptrs=(p, p, p)):
        return lib.ts_votes_labels(n, num_classes, ptrs[0], share, ptrs[1], ptrs[2], None)

    assert labels(n=-1) == -1
    for c in (0, -1, 256):
        assert labels(num_classes=c) == -1
    assert labels(share=float("nan")) == -1
    assert labels(ptrs=(None, p, p)) == -1 and labels(ptrs=(p, None, p)) == -1
    assert labels(n=0, ptrs=(None, None, None)) == 0                 # nothing to do
