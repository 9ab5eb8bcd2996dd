"""The baseline JPEG of DESIGN.md section 6m without a GPU: the float64 oracle (tests/jpeg_oracle.py) against libjpeg
through Pillow, and csrc/jpeg_math.h, built for the host from tests/hostmath/jpeg.cpp, against the oracle; the C entries'
argument checks.  Parity with cv2's encoder (the reference's) is not pinned: cv2 is not a dependency of this project."""
import ctypes
import io

import numpy as np
import pytest
from PIL import Image

import jpeg_cases as JC
import jpeg_oracle as JO
from tinysplat_amd.jpeg import jpeg_header  # noqa: F401  the feature under test: without it nothing here is collected

PIL_SUB = {"444": 0, "420": 2}
ALL = [(name, sub) for name in JC.CASES for sub in JC.SUBSAMPLINGS]


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return JC.build_host(tmp_path_factory.mktemp("jpeg"))


@pytest.fixture(scope="module")
def oracle():
    """name, subsampling -> (coefficients, quotients, divisors, file, statistics), computed once."""
    out = {}
    for name, sub in ALL:
        img, q, ri = JC.CASES[name]
        coefs, quot, div = JO.transform(img, q, sub)
        data, stats = JO.write(coefs, img.shape[1], img.shape[0], q, sub, ri)
        out[name, sub] = (coefs, quot, div, data, stats)
    return out


def _pillow_file(img, quality, sub):
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, format="JPEG", quality=quality, subsampling=PIL_SUB[sub], optimize=False)
    return buf.getvalue()


def _open(data):
    im = Image.open(io.BytesIO(data))
    im.load()
    return im


def _segments(data, marker):
    """The payloads of every segment with this marker before SOS."""
    out, at = [], 2
    while data[at + 1] != 0xDA:
        n = int.from_bytes(data[at + 2:at + 4], "big")
        if data[at + 1] == marker:
            out.append(data[at + 4:at + 2 + n])
        at += 2 + n
    return out


def _huffman_tables(data):
    tables = {}
    for seg in _segments(data, 0xC4):
        while seg:
            n = sum(seg[1:17])
            tables[seg[0]] = (list(seg[1:17]), list(seg[17:17 + n]))
            seg = seg[17 + n:]
    return tables


# ------------------------------------------------------------------------------------------ the oracle against libjpeg
@pytest.mark.parametrize("name,sub", ALL)
def test_case_provokes_what_it_is_there_for(oracle, name, sub):
    coefs, _, _, _, stats = oracle[name, sub]
    JC.check(name, sub, stats, sum(c.shape[0] * c.shape[1] for c in coefs))


def test_oracle_tables_are_libjpegs():
    ours = _huffman_tables(JO.header(8, 8, 90, "420", 1))
    theirs = _huffman_tables(_pillow_file(JC.noise(), 90, "420"))
    assert sorted(ours) == [0x00, 0x01, 0x10, 0x11] and ours == theirs
    assert ours[0x10] == JO.AC_LUMA and ours[0x11] == JO.AC_CHROMA and ours[0x00] == JO.DC_LUMA


@pytest.mark.parametrize("name,sub", ALL)
def test_oracle_file_decodes_with_libjpeg(oracle, name, sub):
    img, q, _ = JC.CASES[name]
    coefs, _, _, data, _ = oracle[name, sub]
    ours, theirs = _open(data), _open(_pillow_file(img, q, sub))
    assert ours.size == (img.shape[1], img.shape[0]) and ours.mode == "RGB"
    assert ours.quantization == theirs.quantization
    if sub == "444" and name not in JC.NOISE_BELOW_Q90:
        # an IEEE-1180 IDCT is within 1 of the float one, times 1 + 1.772 through the colour matrix, plus rounding: 3
        mine = JO.decode(coefs, img.shape[1], img.shape[0], q, sub)
        worst = int(np.abs(np.asarray(ours).astype(int) - mine.astype(int)).max())
        print(f"{name}: libjpeg's pixels differ from the oracle's decode by at most {worst}")
        assert worst <= 3
    deficit = JO.psnr(np.asarray(theirs), img) - JO.psnr(np.asarray(ours), img)
    print(f"{name} {sub}: PSNR deficit against libjpeg's own file {deficit:.3f} dB")
    assert deficit <= 0.25 or np.isnan(deficit)          # nan: both files reproduce the source exactly


# --------------------------------------------------------------------------------------- the host build against the oracle
@pytest.mark.parametrize("name,sub", ALL)
def test_host_coefficients_match_float64(host, oracle, name, sub):
    img, q, _ = JC.CASES[name]
    coefs, quot, div, _, _ = oracle[name, sub]
    got = JC.host_coefficients(host, img, q, sub).astype(np.int64)
    if name in JC.HALF_INTEGERS:
        return                                             # its quotients sit on half-integers by construction
    want, quot, div = (JO.scan_order(v, sub)[0] for v in (coefs, quot, div))
    diff = got - want
    near_half = np.abs(np.abs(quot - np.floor(quot)) - 0.5) * div < 2.0 ** -8
    assert np.abs(diff).max() <= 1 and not (diff != 0)[~near_half].any()
    assert near_half.mean() <= 0.02


@pytest.mark.parametrize("name,sub", ALL)
def test_host_file_is_the_oracles_writer_over_its_coefficients(host, name, sub):
    img, q, ri = JC.CASES[name]
    h, w, _ = img.shape
    coef = JC.host_coefficients(host, img, q, sub)
    for interval in {ri, 1, 2, None}:
        want, _ = JO.write(JC.split_components(coef.astype(np.int64), w, h, sub), w, h, q, sub, interval)
        assert JC.host_encode(host, coef, w, h, q, sub, interval) == want


def test_float_samples_are_the_uint8_bytes(host):
    rng = np.random.default_rng(5)
    f = rng.uniform(-0.1, 1.1, (9, 21, 4)).astype(np.float32)
    f[0, :8, 0] = (np.arange(8) + 0.5) / 255                # ties: half to even
    u8 = np.rint(np.clip(f[:, :, :3] * np.float32(255), 0, 255)).astype(np.uint8)
    for sub in JC.SUBSAMPLINGS:
        want = JC.host_coefficients(host, u8, 90, sub)
        assert np.array_equal(JC.host_coefficients(host, f, 90, sub), want)
        assert np.array_equal(JC.host_coefficients(host, np.ascontiguousarray(f[:, :, :3]), 90, sub), want)


# --------------------------------------------------------------------------------------------------- the library, no GPU
def test_header_entry_and_argument_errors_without_a_gpu():
    from tinysplat_amd import _lib
    lib = _lib.load()
    for sub in JC.SUBSAMPLINGS:
        assert jpeg_header(130, 70, 75, sub, 7) == JO.header(130, 70, 75, sub, 7)
        assert jpeg_header(130, 70, 75, sub) == JO.header(130, 70, 75, sub, JO.default_restart(130, sub))
    assert len(jpeg_header(1, 1)) == 629
    buf = (ctypes.c_uint8 * 1024)()
    assert lib.ts_jpeg_header(0, 8, 90, 0, 0, buf, 1024) == -1 and lib.ts_jpeg_header(8, 8, 101, 0, 0, buf, 1024) == -1
    assert lib.ts_jpeg_header(8, 8, 90, 2, 0, buf, 1024) == -1 and lib.ts_jpeg_header(8, 8, 90, 0, 65536, buf, 1024) == -1
    assert lib.ts_jpeg_header(8, 8, 90, 0, 0, buf, 628) == -1 and lib.ts_jpeg_header(8, 8, 90, 0, 0, None, 1024) == -1
    assert lib.ts_jpeg_ws_bytes(65536, 8, 0, 0) == -1 and lib.ts_jpeg_ws_bytes(1920, 1080, 1, 0) > 48960 * 128
    assert lib.ts_jpeg_max_bytes(8, 8, 0, 0) == 629 + 3 * 416 + 4 and lib.ts_jpeg_max_bytes(8, 0, 0, 0) == -1
    one = ctypes.cast(buf, ctypes.c_void_p)                 # never dereferenced: every call below is refused first
    ok = dict(image=one, dtype=0, stride=3, w=8, h=8, q=90, sub=0, ri=0, ws=None, out=one, cap=1 << 20, size=one)

    def call(**kw):
        a = {**ok, **kw}
        return lib.ts_jpeg_encode(a["image"], a["dtype"], a["stride"], a["w"], a["h"], a["q"], a["sub"], a["ri"], a["ws"],
                                  a["out"], a["cap"], a["size"], None, None)
    assert call() == -1                                     # no workspace
    aligned = ctypes.c_void_p((ctypes.addressof(buf) + 255) // 256 * 256)
    assert call(ws=aligned, cap=629 + 3 * 416 + 3) == -1    # one byte short of the worst case
    assert call(ws=aligned, stride=4) == -1 and call(ws=aligned, dtype=1, stride=5) == -1 and call(ws=aligned, dtype=2) == -1
    assert call(ws=aligned, q=0) == -1 and call(ws=aligned, w=0) == -1 and call(ws=aligned, image=None) == -1
    assert call(ws=aligned, size=None) == -1 and call(ws=aligned, out=None) == -1
