"""The evaluation metrics without a GPU: the float64 oracle's known answers, the host build of
csrc/metrics_math.h against the oracle, the hold-out split, the Evaluator's schedule and files, the tools' parsers, and
the C entries' argument checks."""
import csv
import ctypes
import importlib.util
import math
from pathlib import Path

import numpy as np
import pytest
import torch

import metrics_cases as MC
import metrics_oracle as MO

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return MC.build_host(tmp_path_factory.mktemp("metrics_host"))


def _tool(name):
    spec = importlib.util.spec_from_file_location(f"tool_{name}", str(ROOT / "tools" / f"{name}.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ---------------------------------------------------------------------------------------------------------- the oracle
def test_oracle_known_answers():
    img, _, u8 = MC.inputs(40, 40)
    same = MO.metrics(img, img.clone())
    assert same[0] == 0.0 and same[1] == 0.0 and same[3] == math.inf and abs(same[2] - 1.0) < 1e-12
    for d in (0.25, 0.0625, 0.5):                                     # exact in float32, as is 0.25 + d
        base = torch.full((20, 30, 3), 0.25)
        got = MO.metrics(base + d, base)
        assert abs(got[3] - (-20.0 * math.log10(d))) < 1e-12 and abs(got[1] - d) < 1e-15
    _, tgt, _ = MC.inputs(40, 40)
    rounded = MO.metrics(tgt, MC.bytes_as_float(u8))                  # an image against itself rounded to bytes
    assert rounded[3] >= MC.PSNR_OF_BYTE_ROUNDING and abs(MC.PSNR_OF_BYTE_ROUNDING - 54.1514) < 1e-3


# ------------------------------------------------------------------------------------------------------ the host build
def test_host_byte_conversion_is_torchs_quotient(host):
    want = torch.arange(256, dtype=torch.uint8).to(torch.float32) / 255.0
    got = np.array([host.mh_byte_to_float(b) for b in range(256)], dtype=np.float32)
    assert got.tobytes() == want.numpy().tobytes()


def test_host_psnr_and_ssim_term(host):
    assert host.mh_psnr(0.0) == math.inf and host.mh_psnr(1.0) == 0.0
    assert abs(host.mh_psnr(0.01) - 20.0) < 1e-12
    # identical statistics -> 1; uncorrelated constant patches -> the luminance term alone
    assert abs(host.mh_ssim_term(0.5, 0.5, 0.35, 0.35, 0.35) - 1.0) < 1e-6
    # (values exact in float32: the variances cancel to exactly zero)
    lum = (2 * 0.25 * 0.75 + 1e-4) / (0.0625 + 0.5625 + 1e-4)
    assert abs(host.mh_ssim_term(0.25, 0.75, 0.0625, 0.5625, 0.1875) - lum) < 1e-6


@pytest.mark.parametrize("byte_target", [False, True], ids=["float", "uint8"])
@pytest.mark.parametrize("h,w", MC.SHAPES)
def test_host_metrics_against_the_oracle(host, h, w, byte_target):
    img, tgt, u8 = MC.inputs(h, w)
    got = MC.host_metrics(host, img, u8 if byte_target else tgt)
    print(f"{h}x{w} {'uint8' if byte_target else 'float'}: host {got.tolist()} oracle {MC.reference(h, w, byte_target).tolist()}")
    MC.check(got, MC.reference(h, w, byte_target))
    if byte_target:
        assert got[3] < MC.PSNR_OF_BYTE_ROUNDING                     # (the noise, not the rounding, is what is measured)
        as_float = MC.host_metrics(host, img, MC.bytes_as_float(u8))
        assert got.tobytes() == as_float.tobytes()                    # the byte path is the float path, bit for bit
        four = MC.host_metrics(host, MC.with_depth(img), u8)
        assert four.tobytes() == got.tobytes()                        # channel 3 is never read


def test_host_identical_images(host):
    img, _, _ = MC.inputs(40, 40)
    got = MC.host_metrics(host, img, img.clone())
    assert got[0] == 0.0 and got[1] == 0.0 and got[3] == math.inf and abs(got[2] - 1.0) < 1e-6


def test_segmentation_is_a_function_of_the_shape(host):
    from tinysplat_amd import _lib
    lib = _lib.load()
    for h, w in MC.SHAPES + ((1080, 1920), (2160, 3840), (11, 100000)):
        waves = host.mh_waves(h, w)
        blocks_x = -(-(w - 10) // 64)
        seg = host.mh_segment_rows(h - 10, w - 10)
        assert 8 <= seg <= 64 and waves == 3 * blocks_x * -(-(h - 10) // seg)
        first = lib.ts_image_metrics_ws_bytes(h, w)
        assert first == 24 * waves > 0 and lib.ts_image_metrics_ws_bytes(h, w) == first
    assert host.mh_segment_rows(1070, 1910) == 43                     # 1080p: 30 column blocks x 25 segments
    assert host.mh_waves(10, 100) == 0 and host.mh_waves(100, 10) == 0
    assert lib.ts_image_metrics_ws_bytes(10, 100) == 0 and lib.ts_image_metrics_ws_bytes(100, 10) == 0
    assert lib.ts_image_metrics_ws_bytes(-5, 100) == 0


# ----------------------------------------------------------------------------------------------------- the C entries
def test_entries_refuse_bad_arguments_without_a_gpu():
    from tinysplat_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    assert lib.ts_image_metrics(10, 100, 3, p, p, 0, p, p, None) == -1        # H <= 10
    assert lib.ts_image_metrics(100, 10, 3, p, p, 0, p, p, None) == -1        # W <= 10
    assert lib.ts_image_metrics(40, 40, 5, p, p, 0, p, p, None) == -1         # pixel_floats
    assert lib.ts_image_metrics(40, 40, 2, p, p, 1, p, p, None) == -1
    for missing in range(4):
        ptrs = [p, p, p, p]
        ptrs[missing] = None
        assert lib.ts_image_metrics(40, 40, 3, ptrs[0], ptrs[1], 0, ptrs[2], ptrs[3], None) == -1
    assert lib.ts_image_metrics(40, 40, 3, p, p, 0, p + 4, p, None) == -1     # the doubles' alignment
    assert lib.ts_image_metrics(40, 40, 3, p, p, 0, p, p + 4, None) == -1
    assert lib.ts_image_metrics(40, 40, 3, p, p + 1, 0, p, p, None) == -1     # a float target on an odd byte


def test_wrapper_refuses_cpu_tensors_and_bad_shapes():
    from tinysplat_amd import image_metrics
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        image_metrics(torch.zeros(20, 20, 3), torch.zeros(20, 20, 3))


# -------------------------------------------------------------------------------------------------------- the split
def test_holdout_split():
    from tinysplat_amd import holdout_split
    names = [f"img_{i:03d}.jpg" for i in (7, 2, 19, 0, 11, 5, 3, 13, 17, 1, 23, 29, 31, 37, 41, 43, 47)]
    by_name = sorted(range(len(names)), key=lambda i: names[i])
    train, test = holdout_split(names)                                         # every = 8
    assert test == [by_name[0], by_name[8], by_name[16]] and train == [i for i in by_name if i not in test]
    assert holdout_split(names, 0) == (by_name, [])
    assert holdout_split(names, 1) == ([], by_name)
    train, test = holdout_split(names, 8, 3)
    assert test == [by_name[3], by_name[11]]
    for every, offset in ((8, 0), (8, 7), (1, 0), (0, 0), (3, 2)):
        train, test = holdout_split(names, every, offset)
        assert not set(train) & set(test) and sorted(train + test) == list(range(len(names)))
        assert [names[i] for i in train] == sorted(names[i] for i in train)
    assert holdout_split([], 8) == ([], [])
    for every, offset in ((-1, 0), (8, 8), (8, -1), (0, 1)):
        with pytest.raises(ValueError):
            holdout_split(names, every, offset)


# ----------------------------------------------------------------------------------------------------- the Evaluator
class _Model:
    means = torch.zeros(123, 3)


def _stand_in(calls):
    from tinysplat_amd.metrics import EvalResult

    def evaluate(model, cameras, targets, device, background=None):
        calls.append((len(cameras), device, background))
        k = len(calls)
        table = np.array([[1e-3 / k, 0.02 / k, 0.9, 30.0 + k], [3e-3 / k, 0.04 / k, 0.8, 26.0 + k]])
        return EvalResult(table, ["a", "b"])
    return evaluate


def test_evaluator_schedule_line_and_csv(monkeypatch, tmp_path):
    from tinysplat_amd import Evaluator
    from tinysplat_amd import metrics as M
    calls, seen = [], []
    monkeypatch.setattr(M, "evaluate", _stand_in(calls))
    path = tmp_path / "metrics.csv"
    ev = Evaluator(_Model(), ["cam0", "cam1"], ["t0", "t1"], "cuda:0", 20, on_result=lambda row, res: seen.append(row),
                   csv_path=path)
    for step in range(1, 61):
        ev(step, {"loss": 0.0})
    assert [r[0] for r in ev.rows] == [20, 40, 60] and len(calls) == 3 and calls[0] == (2, "cuda:0", None)
    assert ev.rows[0] == (20, 123, 29.0, pytest.approx(0.85), pytest.approx(0.03)) and seen == ev.rows
    assert ev.final(60) == ev.rows[-1] and len(ev.rows) == 3                  # the schedule took step 60 already
    row = ev.final(65)
    assert len(ev.rows) == 4 and row == ev.rows[-1] and row[0] == 65 and len(calls) == 4 and len(ev.results) == 4
    assert Evaluator.format((20, 123, 29.0, 0.85, 0.03)) == \
        "Step: 20         | PSNR: 29.0000    | SSIM: 0.8500     | L1: 0.0300     | N: 123       "
    with open(path, newline="") as f:
        lines = list(csv.reader(f))
    assert lines[0] == ["step", "n", "psnr", "ssim", "l1"] == list(Evaluator.HEADER)
    assert [ln[0] for ln in lines[1:]] == ["20", "40", "60", "65"] and all(ln[1] == "123" for ln in lines[1:])
    assert [float(v) for v in lines[1][2:]] == list(ev.rows[0][2:])           # repr round-trips the doubles
    # a second evaluator appends to the same file without a second header; every = 0 fires only on demand
    ev2 = Evaluator(_Model(), ["cam0"], ["t0"], "cuda:0", 0, csv_path=path)
    for step in range(1, 30):
        ev2(step, None)
    assert ev2.rows == []
    ev2.final(29)
    with open(path, newline="") as f:
        lines = list(csv.reader(f))
    assert len(lines) == 6 and lines[-1][0] == "29" and sum(ln[0] == "step" for ln in lines) == 1
    with pytest.raises(ValueError):
        Evaluator(_Model(), [], [], "cuda:0", -1)


def test_eval_result_means_are_per_view_means():
    from tinysplat_amd.metrics import EvalResult
    r = EvalResult(np.array([[1e-2, 0.1, 0.5, 20.0], [1e-4, 0.3, 0.7, 40.0]]), ["a", "b"])
    assert r.psnr == 30.0 and r.ssim == pytest.approx(0.6) and r.l1 == pytest.approx(0.2) and r.mse == pytest.approx(5.05e-3)
    assert r.psnr != pytest.approx(-10.0 * math.log10(r.mse))                 # not the PSNR of the mean error


# -------------------------------------------------------------------------------------------------------- the tools
def test_train_tool_parser_has_the_evaluation_flags_off_by_default():
    tool = _tool("train")
    args = tool.parse([])
    assert (args.eval_holdout, args.eval_interval, args.metrics_csv) == (0, None, None)
    before = {"device": "cuda:0", "sh_degree": 3, "max_iter": 10_000, "dataset_dir": "datasets/train",
              "colmap_path": "colmap/sparse/0", "images_path": "images", "max_image_dimension": None,
              "principal_point": "reference", "output": "scene.ply", "viewer": False, "viewer_ip": "127.0.0.1",
              "viewer_port": 8765}
    now = vars(args)
    assert {k: now[k] for k in before} == before
    assert set(now) - set(before) == {"eval_holdout", "eval_interval", "metrics_csv"}
    args = tool.parse(["--eval-holdout", "8", "--eval-interval", "500", "--metrics-csv", "m.csv"])
    assert (args.eval_holdout, args.eval_interval, args.metrics_csv) == (8, 500, "m.csv")
    for bad in (["--eval-holdout", "-1"], ["--eval-holdout", "8", "--eval-interval", "0"], ["--metrics-csv", "m.csv"],
                ["--eval-interval", "10"]):
        with pytest.raises(SystemExit):
            tool.parse(bad)


def test_eval_tool_parser_and_table():
    tool = _tool("eval")
    args = tool.parse(["scene.splat", "--dataset-dir", "d"])
    assert (args.scene, args.dataset_dir, args.holdout, args.csv, args.max_image_dimension, args.principal_point,
            args.device) == ("scene.splat", "d", 8, None, None, "reference", "cuda:0")
    args = tool.parse(["s.pth", "--dataset-dir", "d", "--holdout", "0", "--csv", "o.csv", "--max-image-dimension", "800",
                       "--principal-point", "center"])
    assert (args.holdout, args.csv, args.max_image_dimension, args.principal_point) == (0, "o.csv", 800, "center")
    for bad in (["scene.obj", "--dataset-dir", "d"], ["scene.ply"], ["scene.ply", "--dataset-dir", "d", "--holdout", "-2"]):
        with pytest.raises(SystemExit):
            tool.parse(bad)
    from tinysplat_amd.metrics import EvalResult
    rows = tool.table_rows(EvalResult(np.array([[1e-2, 0.1, 0.5, 20.0], [1e-4, 0.3, 0.7, 40.0]]), ["a.jpg", "b.jpg"]))
    assert rows[0] == ("a.jpg", 20.0, 0.5, 0.1, 1e-2) and rows[-1][0] == "mean" and rows[-1][1] == 30.0
