"""The .splat record without a GPU: csrc/splat_record.h, built for the host from
tests/hostmath/splatfile.cpp, against the float64 oracle (tests/splat_oracle.py); the known answer as literal bytes; the
order's tie rule; the C entries' argument checks; the file-size check; the export tool's command line."""
import ctypes
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import splat_cases as SC
import splat_oracle as SO
from tinysplat_amd.formats import export_splat  # noqa: F401  the feature under test: without it nothing here is collected

ROOT = Path(__file__).resolve().parent.parent
F32P, U8P = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_uint8)
KAT_RECORD = bytes.fromhex("0000803f 00000040 00004040" + " 0000803f" * 3 + " 7f7f7f7f" + " ff808080")


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """g++ build of tests/hostmath/splatfile.cpp: the kernels' header compiled for the host."""
    so = tmp_path_factory.mktemp("splat") / "_splatfile.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared",
                    str(ROOT / "tests" / "hostmath" / "splatfile.cpp"), "-o", str(so)], check=True)
    lib = ctypes.CDLL(str(so))
    lib.sr_keys.restype, lib.sr_keys.argtypes = None, [ctypes.c_int64, F32P, F32P, F32P]
    lib.sr_encode.restype, lib.sr_encode.argtypes = None, [ctypes.c_int64, F32P, F32P, F32P, F32P, F32P, U8P]
    lib.sr_decode.restype, lib.sr_decode.argtypes = None, [ctypes.c_int64, U8P, F32P, F32P, F32P, F32P, F32P]
    return lib


def _p(a, t):
    return a.ctypes.data_as(t)


def _encode(host, scene):
    n = scene["means"].shape[0]
    rec = np.zeros((n, 32), np.uint8)
    host.sr_encode(n, *[_p(a, F32P) for a in SC.args(scene)], _p(rec, U8P))
    return rec


def _decode(host, rec):
    n = rec.shape[0]
    out = {"means": np.zeros((n, 3), np.float32), "scales": np.zeros((n, 3), np.float32),
           "colors_dc": np.zeros((n, 3), np.float32), "opacities": np.zeros((n, 1), np.float32),
           "quats": np.zeros((n, 4), np.float32)}
    host.sr_decode(n, _p(np.ascontiguousarray(rec), U8P), *[_p(a, F32P) for a in SC.args(out)])
    return out


# ------------------------------------------------------------------------------------------------ the known answer
def test_known_answer_as_bytes(host):
    f = lambda *v: np.array([v], np.float32)
    scene = {"means": f(1, 2, 3), "scales": f(0, 0, 0), "colors_dc": f(0, 0, 0), "opacities": f(0), "quats": f(1, 0, 0, 0)}
    assert len(KAT_RECORD) == 32
    assert _encode(host, scene).tobytes() == KAT_RECORD
    rec, pre = SO.encode(*SC.args(scene))
    assert rec.tobytes() == KAT_RECORD and pre[0, 24:].tolist() == [127.5] * 4 + [256.0, 128.0, 128.0, 128.0]
    kat = np.frombuffer(KAT_RECORD, np.uint8).reshape(1, 32)
    c, o = (127 / 255 - 0.5) / SO.C0, np.log((127 / 255) / (128 / 255))
    for got in (_decode(host, kat), {k: v.astype(np.float32) for k, v in SO.decode(kat).items()}):
        assert got["means"].tolist() == [[1.0, 2.0, 3.0]] and got["scales"].tolist() == [[0.0, 0.0, 0.0]]
        assert got["quats"].tolist() == [[127 / 128, 0.0, 0.0, 0.0]]
        assert got["colors_dc"].tolist() == [[float(np.float32(c))] * 3] and got["opacities"].tolist() == [[float(np.float32(o))]]


# ------------------------------------------------------------------------------------------------ the header
def test_header_against_the_oracle(host):
    edges, names = SC.edge_scene()
    scene = SC.concat(SC.random_scene(4000, seed=11), edges)
    n = scene["means"].shape[0]
    got = _encode(host, scene)
    rec, pre = SO.encode(*SC.args(scene))
    assert np.array_equal(got[:, :12], scene["means"].view(np.uint8).reshape(n, 12))       # positions: the bits
    SC.check_exp_scales(got, scene["scales"], "host")
    SO.compare_bytes(got, rec, pre, "host encode")
    # every edge rule, on the header's bytes themselves
    e = {k: got[4000 + i, 24:].tolist() for k, i in names.items()}
    assert e["clip_below"][:4] == [0, 0, 0, 0] and e["clip_above"][:4] == [255, 255, 255, 255]
    assert e["inf_color"][:2] == [255, 0] and e["nan_color"][:3] == [0, 127, 0]
    assert e["nan_opacity"][3] == 0 and e["nan_opacity"][:3] == e["plain"][:3]
    for k in ("zero_quat", "nan_quat", "inf_quat", "identity"):
        assert e[k][4:] == [255, 128, 128, 128], k
    assert e["tiny_quat"][4:] == e["plain"][4:] == e["huge_quat"][4:] and e["plain"][4:] != [255, 128, 128, 128]
    assert e["negative_w"][4:] == [0, 128, 128, 128]
    assert e["negative_w_mixed"][4] < 128 and e["negative_w_mixed"][4:] == rec[4000 + names["negative_w_mixed"], 28:].tolist()
    # keys
    keys = np.zeros(n, np.float32)
    host.sr_keys(n, _p(scene["scales"], F32P), _p(scene["opacities"], F32P), _p(keys, F32P))
    SC.check_keys(keys, scene["scales"], scene["opacities"], "host")
    assert np.isnan(keys[4000 + names["nan_opacity"]]) and int(np.isnan(keys).sum()) == 1


def test_decode_against_the_oracle(host):
    scene = SC.random_scene(4000, seed=12)
    rec = np.concatenate([SO.encode(*SC.args(scene))[0], SC.decode_edge_records()])
    got = _decode(host, rec)
    SC.check_decoded(got, rec, "host")
    e = {k: v[4000:] for k, v in got.items()}
    log_min = float(np.log(np.float32(SO.FLT_MIN)))
    assert e["scales"][0].tolist() == [log_min] * 3 and e["scales"][1].tolist() == [log_min] * 3     # 0, negative, NaN, subnormal
    lo, hi = float(np.float32(np.log(1 / 254))), float(np.float32(np.log(254 / 1)))
    assert e["opacities"][:, 0].tolist()[:2] == [lo, hi] and e["opacities"][2, 0] == lo and e["opacities"][3, 0] == hi
    assert e["quats"][1].tolist() == [-1.0, -1 / 128, 0.0, 127 / 128]
    assert np.isfinite(np.concatenate([v.reshape(-1) for k, v in got.items() if k != "means"])).all()


def test_export_then_load_is_not_byte_idempotent(host):
    """Truncation, documented: a decoded colour byte b gives 255 (b / 255) a rounding below b as often as above, and
    trunc then yields b - 1; an alpha byte 255 is decoded as 254 and may come back as 253; a decoded quaternion is up to
    2 / 128 short of unit length (each component lost up to 1 / 128 to truncation), so renormalising moves 128 q by up to
    2 and the second truncation by one more."""
    scene = SC.random_scene(2000, seed=13)
    first = _encode(host, scene)
    back = _decode(host, first)
    second = _encode(host, back)
    assert np.array_equal(second[:, :12], first[:, :12])
    d = np.abs(second[:, 24:].astype(np.int16) - first[:, 24:].astype(np.int16))
    print(f"\nbytes changed by a second export: {float((d != 0).mean()):.2%}")
    assert d[:, :3].max() <= 1 and d[:, 3].max() <= 2 and d[:, 4:].max() <= 3 and (d != 0).any()


# ------------------------------------------------------------------------------------------------ the order
def test_order_tie_rule_matches_numpy_stable_argsort():
    from tinysplat_amd.formats import _order_from_keys
    rng = np.random.default_rng(5)
    keys = rng.choice(np.float32([0.0, -0.0, 1e-30, 0.5, 0.5000001, 2.0, np.inf, np.nan, 1e-45, 3e38]), 5000)
    keys[::7] = rng.random(keys[::7].shape, np.float32)
    keys[1::11] = np.float32(-1.5)                                      # no key is negative, but the map orders them too
    keys[3::13] = -np.float32(np.nan)                                   # a NaN with the sign bit set
    got = _order_from_keys(torch.from_numpy(keys.copy())).numpy()
    assert got.dtype == np.int64 and np.array_equal(got, SO.order(keys))
    assert np.array_equal(got, np.argsort(-keys, kind="stable"))
    nans = int(np.isnan(keys).sum())
    assert nans > 100 and np.isnan(keys[got[-nans:]]).all() and np.all(np.diff(got[-nans:]) > 0)
    assert _order_from_keys(torch.zeros(0)).shape == (0,)
    assert _order_from_keys(torch.full((9,), 0.25)).tolist() == list(range(9))


# ------------------------------------------------------------------------------------------------ entries, files, tool
def test_entry_argument_checks():
    """None of these needs a device: every refusal, and every call with nothing to do, returns before a launch."""
    from tinysplat_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(64)
    # n, scales, opacities, keys, stream
    assert lib.ts_splat_keys(-1, p, p, p, None) == -1 and lib.ts_splat_keys(0, None, None, None, None) == 0
    for i in (1, 2, 3):
        a = [4, p, p, p, None]
        a[i] = None
        assert lib.ts_splat_keys(*a) == -1, i
    # n, m, means, scales, colors_dc, opacities, quats, order, records, stream
    good = [8, 4, p, p, p, p, p, p, p, None]
    for i in (2, 3, 4, 5, 6, 8):
        a = list(good)
        a[i] = None
        assert lib.ts_splat_pack(*a) == -1, i
    assert lib.ts_splat_pack(-1, 4, *good[2:]) == -1 and lib.ts_splat_pack(8, -1, *good[2:]) == -1
    assert lib.ts_splat_pack(4, 8, p, p, p, p, p, None, p, None) == -1          # more records than Gaussians, no order
    assert lib.ts_splat_pack(8, 4, p, p, p, p, p, p, ctypes.c_void_p(72), None) == -1   # records not 16-byte aligned
    assert lib.ts_splat_pack(8, 0, *([None] * 8)) == 0 and lib.ts_splat_pack(0, 0, *([None] * 8)) == 0
    # n, records, means, scales, colors_dc, opacities, quats, stream
    good = [4, p, p, p, p, p, p, None]
    for i in range(1, 7):
        a = list(good)
        a[i] = None
        assert lib.ts_splat_unpack(*a) == -1, i
    assert lib.ts_splat_unpack(-1, *good[1:]) == -1 and lib.ts_splat_unpack(4, ctypes.c_void_p(8), *good[2:]) == -1
    assert lib.ts_splat_unpack(0, *([None] * 7)) == 0
    assert lib.ts_abi_version() == 9 == _lib.ABI_VERSION


def test_load_splat_refuses_a_file_that_is_not_whole_records(tmp_path):
    from tinysplat_amd.formats import load_splat
    (tmp_path / "short.splat").write_bytes(bytes(31))
    with pytest.raises(ValueError, match="32-byte"):
        load_splat(tmp_path / "short.splat", "cuda:0")
    (tmp_path / "long.splat").write_bytes(bytes(65))
    with pytest.raises(ValueError):
        load_splat(tmp_path / "long.splat", "cuda:0")


def test_cpu_tensors_and_bad_options_are_refused():
    from tinysplat_amd import formats
    from tinysplat_amd.synthetic import make_scene
    model = make_scene(10, 0, 64, 64)[0]
    for fn in (formats.splat_records, formats.splat_order):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(model)
    with pytest.raises(ValueError):
        formats.splat_records(model, order="depth")
    with pytest.raises(ValueError):
        formats.splat_records(model, limit=-1)
    model.scales = model.scales.double()
    with pytest.raises(ValueError):
        formats.splat_records(model)


def test_export_tool_help_runs():
    out = subprocess.run([sys.executable, str(ROOT / "tools" / "export.py"), "--help"], capture_output=True, text=True)
    assert out.returncode == 0 and "SPLAT" in out.stdout and "MESH_PLY" in out.stdout and "--limit" in out.stdout
