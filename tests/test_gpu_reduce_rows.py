"""The gradient-row reduction (``ts_reduce_partials`` / ``ts_reduce_partials_rows``) driven directly on synthetic arrays,
against a host loop that adds every Gaussian's flagged rows in ascending slot order in float64 and rounds once.

* ``v_conic``, ``v_colors`` and ``v_depth`` are those sums (or exact halves of them): bit for bit.
* ``v_xy`` and ``v_opacity`` are float32 expressions of the sums and of the record, restated here in float32 operation by
  operation; the kernel may fuse a product into a sum, so they are held within 2 ulp.  Rows and record entries are
  positive, so that no such sum cancels.

The rows' magnitudes span 2^-20 .. 2^20: their float64 sums are not exact, so an addition order other than ascending shows.
``row_flags`` and ``partials`` live inside larger tensors whose guard bytes carry the CURRENT generation and whose guard
rows - like every row whose flag does not match - carry 1e30: a flag byte outside a Gaussian's own range that reaches a
sum shows in the result instead of faulting.  Slot counts sit around the sizes at which the walk changes path (4 rows per
step, windows of 32 slots, 16-byte flag pieces); every count starts at every residue modulo 16, and the array itself
starts both on and off a 16-byte boundary."""
import functools

import numpy as np
import pytest
import torch

from tinysplat_amd import _lib
from tinysplat_amd.ops import _ptr, _stream

pytestmark = pytest.mark.gpu

COUNTS = (0, 1, 3, 4, 5, 8, 9, 31, 32, 33, 64, 65, 100, 257)
PATTERNS = ("none", "all", "first", "last", "alternating", "one_in_last_window")
LOGIT, SPLIT = 1, 4                        # TS_RASTER_LOGIT_OPACITY, TS_RASTER_SPLIT_BLOCKS
GUARD = 64                                 # guard bytes / guard rows on either side
POISON = np.float32(1e30)


@functools.lru_cache(maxsize=None)
def layout(name):
    """(counts[n], under_test[n]) - 'residues': every count of COUNTS starting at every residue modulo 16, behind a filler
    that moves the start there, between a first and a last Gaussian that own the ends of the array; 'waves': lanes with 0, 1
    and 100 slots side by side."""
    if name == "waves":
        cnt = np.array([1, 0, 100] * 64 + [1], dtype=np.int32)
        return cnt, np.ones(len(cnt), dtype=bool)
    cnt, test, pos = [5], [True], 5
    for r in range(16):
        for c in COUNTS:
            fill = (r - pos) % 16
            cnt += [fill, c]
            test += [False, True]
            pos += fill + c
    cnt.append(5)
    test.append(True)
    return np.array(cnt, dtype=np.int32), np.array(test, dtype=bool)


@functools.lru_cache(maxsize=None)
def scenario(name, gen, pattern, per_slot):
    """Host arrays of one launch: counts, their running sum, flag bytes [I * per_slot], rows [I * per_slot, 12], records
    [n, 12] and the float64 sums [n, 10] of the flagged rows in ascending order, rounded to float32.  per_slot = 4 is the
    split-blocks layout (slot s owns the bytes and rows 4 s .. 4 s + 3, of which 1 - 4 are flagged)."""
    cnt, test = layout(name)
    n, rng = len(cnt), np.random.default_rng(1000 * gen + 10 * PATTERNS.index(pattern) + per_slot)
    cum = np.cumsum(cnt).astype(np.int32)
    total = int(cum[-1])
    stale = np.array([v for v in (0, 1, 2, 199, 200, 201, 255) if v != gen], dtype=np.uint8)
    flagged = np.zeros(total, dtype=bool)
    for i in range(n):
        b, c = int(cum[i]) - int(cnt[i]), int(cnt[i])
        if c == 0:
            continue
        f = np.zeros(c, dtype=bool)
        if not test[i]:
            f = rng.random(c) < 0.5
        elif pattern == "all":
            f[:] = True
        elif pattern == "first":
            f[0] = True
        elif pattern == "last":
            f[-1] = True
        elif pattern == "alternating":
            f[i % 2::2] = True
        elif pattern == "one_in_last_window":
            f[32 * ((c - 1) // 32)] = True
        flagged[b:b + c] = f
    if per_slot == 1:
        row_flagged = flagged
    else:                                 # 1 - 4 rows of a flagged slot, never none
        row_flagged = np.zeros((total, 4), dtype=bool)
        for s in np.nonzero(flagged)[0]:
            k = rng.permutation(4)[:rng.integers(1, 5)]
            row_flagged[s, k] = True
        row_flagged = row_flagged.reshape(-1)
    flags = np.where(row_flagged, np.uint8(gen), stale[rng.integers(0, len(stale), total * per_slot)]).astype(np.uint8)
    rows = (rng.uniform(0.5, 1.5, (total * per_slot, 12)) * 2.0 ** rng.integers(-20, 21, (total * per_slot, 12)))
    rows = rows.astype(np.float32)
    rows[~row_flagged] = POISON
    splats = rng.uniform(0.05, 0.95, (n, 12)).astype(np.float32)
    # the reference: step k adds, for every Gaussian at once, its k-th row if flagged - ascending order per Gaussian
    sums = np.zeros((n, 10), dtype=np.float64)
    begin = (cum - cnt).astype(np.int64) * per_slot
    for k in range(int(cnt.max()) * per_slot):
        live = np.nonzero(k < cnt.astype(np.int64) * per_slot)[0]
        live = live[row_flagged[begin[live] + k]]
        sums[live] += rows[begin[live] + k, :10].astype(np.float64)
    return cnt, cum, flags, rows, splats, sums.astype(np.float32)


def expected(cnt, splats, a, flags, channels, color_mask=None):
    """The five arrays from the rounded sums a[n, 10], float32 operation by operation as the kernel writes them."""
    one, half = np.float32(1), np.float32(0.5)
    op, A, B, C = splats[:, 2], splats[:, 3], splats[:, 4], splats[:, 5]
    has = cnt > 0
    vx = np.where(has, A * a[:, 1] + B * a[:, 2], 0).astype(np.float32)
    vy = np.where(has, B * a[:, 1] + C * a[:, 2], 0).astype(np.float32)
    vop = -a[:, 0] / op
    if flags & LOGIT:
        vop = vop * (op * (one - op))
    vop = np.where(has, vop, 0).astype(np.float32)
    conic = np.stack([half * a[:, 3], a[:, 4], half * a[:, 5]], 1)
    colors = a[:, 6:6 + channels].copy()
    if color_mask is not None:
        for c in range(3):
            colors[has & ((color_mask >> c) & 1 == 0), c] = 0
    return np.stack([vx, vy], 1), conic, colors, vop


def device_arrays(flags, rows, shift, gen):
    """row_flags and partials inside larger tensors: guard bytes of the current generation, guard rows of 1e30."""
    dev = torch.device("cuda:0")
    big_f = torch.full((GUARD + shift + len(flags) + GUARD + 16,), gen, dtype=torch.uint8, device=dev)
    assert big_f.data_ptr() % 16 == 0
    row_flags = big_f[GUARD + shift:GUARD + shift + len(flags)]
    row_flags.copy_(torch.from_numpy(flags))
    big_p = torch.full((GUARD + len(rows) + GUARD, 12), float(POISON), dtype=torch.float32, device=dev)
    partials = big_p[GUARD:GUARD + len(rows)]
    partials.copy_(torch.from_numpy(rows))
    return (big_f, big_p), row_flags, partials


def launch(cnt, cum, row_flags, partials, splats, flags, channels, depth=False, color_mask=None, rows_out=False):
    dev = torch.device("cuda:0")
    lib, n = _lib.load(), len(cnt)
    d_cnt, d_cum, d_sp = (torch.from_numpy(x).to(dev) for x in (cnt, cum, splats))
    nan = float("nan")
    if rows_out:
        out = torch.full((n, 12), nan, device=dev)
        _lib.check(lib.ts_reduce_partials_rows(n, channels, flags, _ptr(d_cnt), _ptr(d_cum), _ptr(partials), _ptr(row_flags),
                                               _ptr(d_sp), _ptr(out), _stream(dev)), "ts_reduce_partials_rows")
        torch.cuda.synchronize()
        return out.cpu().numpy()
    v_xy, v_conic, v_op = torch.full((n, 2), nan, device=dev), torch.full((n, 3), nan, device=dev), torch.full((n,), nan, device=dev)
    v_colors = torch.full((n, 3 if depth else channels), nan, device=dev)
    v_depth = torch.full((n,), nan, device=dev) if depth else None
    d_mask = torch.from_numpy(color_mask).to(dev) if color_mask is not None else None
    _lib.check(lib.ts_reduce_partials(n, channels, flags, _ptr(d_cnt), _ptr(d_cum), _ptr(partials), _ptr(row_flags), _ptr(d_sp),
                                      _ptr(v_xy), _ptr(v_conic), _ptr(v_colors), _ptr(v_op), _ptr(v_depth), _ptr(d_mask),
                                      _stream(dev)), "ts_reduce_partials")
    torch.cuda.synchronize()
    return [t.cpu().numpy() if t is not None else None for t in (v_xy, v_conic, v_colors, v_op, v_depth)]


def assert_bits(got, want, what):
    bad = np.nonzero(got.view(np.uint32) != want.view(np.uint32))
    assert len(bad[0]) == 0, f"{what}: {len(bad[0])} entries differ, first at {[int(b[0]) for b in bad]}: " \
                             f"{got[tuple(b[0] for b in bad)]} against {want[tuple(b[0] for b in bad)]}"


def assert_ulp(got, want, what, ulps=2):
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    tol = ulps * np.spacing(np.abs(want)).astype(np.float64)
    worst = float(np.max(err / np.maximum(np.spacing(np.abs(want)).astype(np.float64), 1e-300)))
    print(f"{what}: worst {worst:.2f} ulp")
    assert np.all(np.isfinite(got)) and np.all(err <= tol), f"{what}: worst {worst:.2f} ulp (bound {ulps})"


def flag_word(gen, extra=0):
    return extra | ((gen << 8) if gen != 1 else 0)          # generation 1 is also the legacy value of a zeroed array


@pytest.mark.parametrize("shift", [0, 5])
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("gen", [1, 200])
@pytest.mark.parametrize("name", ["residues", "waves"])
def test_flagged_rows_in_ascending_order(name, gen, pattern, shift):
    cnt, cum, flags, rows, splats, sums = scenario(name, gen, pattern, 1)
    assert cnt[0] > 0 and cnt[-1] > 0                       # the ends of row_flags belong to the first and last Gaussian
    keep, row_flags, partials = device_arrays(flags, rows, shift, gen)
    word = flag_word(gen, LOGIT)
    got = launch(cnt, cum, row_flags, partials, splats, word, 3)
    again = launch(cnt, cum, row_flags, partials, splats, word, 3)
    v_xy, v_conic, v_colors, v_op = expected(cnt, splats, sums, word, 3)
    assert_bits(got[1], v_conic, "v_conic")
    assert_bits(got[2], v_colors, "v_colors")
    assert_ulp(got[0], v_xy, "v_xy")
    assert_ulp(got[3], v_op, "v_opacity")
    for a, b in zip(got[:4], again[:4]):
        assert a.tobytes() == b.tobytes(), "two calls differ"


@pytest.mark.parametrize("gen", [1, 200])
@pytest.mark.parametrize("variant", ["ch3_linear_opacity", "ch4", "ch4_depth", "ch3_color_mask", "ch4_depth_color_mask",
                                     "ch3_rows", "ch4_rows"])
def test_other_outputs(variant, gen):
    cnt, cum, flags, rows, splats, sums = scenario("residues", gen, "alternating", 1)
    keep, row_flags, partials = device_arrays(flags, rows, 3, gen)
    channels = 4 if variant.startswith("ch4") else 3
    word = flag_word(gen, 0 if variant == "ch3_linear_opacity" else LOGIT)
    mask = np.random.default_rng(5).integers(0, 8, len(cnt)).astype(np.uint8) if "color_mask" in variant else None
    v_xy, v_conic, v_colors, v_op = expected(cnt, splats, sums, word, channels, mask)
    if variant.endswith("rows"):
        got = launch(cnt, cum, row_flags, partials, splats, word, channels, rows_out=True)
        assert_ulp(got[:, 0:2], v_xy, "grad_rows v_xy")
        assert_bits(got[:, 2:5], v_conic, "grad_rows v_conic")
        assert_bits(got[:, 5:8], v_colors[:, :3], "grad_rows v_colors")
        depth = v_colors[:, 3] if channels == 4 else np.zeros(len(cnt), dtype=np.float32)
        assert_bits(got[:, 8], depth, "grad_rows depth")
        assert_ulp(got[:, 9], v_op, "grad_rows v_opacity")
        assert_bits(got[:, 10:12], np.zeros((len(cnt), 2), dtype=np.float32), "grad_rows padding")
        return
    depth = "depth" in variant
    got = launch(cnt, cum, row_flags, partials, splats, word, channels, depth=depth, color_mask=mask)
    assert_bits(got[1], v_conic, "v_conic")
    assert_bits(got[2], v_colors[:, :3] if depth else v_colors, "v_colors")
    if depth:
        assert_bits(got[4], v_colors[:, 3], "v_depth")
    assert_ulp(got[0], v_xy, "v_xy")
    assert_ulp(got[3], v_op, "v_opacity")


@pytest.mark.parametrize("gen", [1, 200])
@pytest.mark.parametrize("channels", [3, 4])
def test_split_blocks_flag_words(channels, gen):
    """TS_RASTER_SPLIT_BLOCKS: slot s owns the flag word and the rows 4 s .. 4 s + 3, of which 1 - 4 are flagged."""
    cnt, cum, flags, rows, splats, sums = scenario("residues", gen, "alternating", 4)
    keep, row_flags, partials = device_arrays(flags, rows, 0, gen)
    word = flag_word(gen, LOGIT | SPLIT)
    got = launch(cnt, cum, row_flags, partials, splats, word, channels)
    again = launch(cnt, cum, row_flags, partials, splats, word, channels)
    v_xy, v_conic, v_colors, v_op = expected(cnt, splats, sums, word, channels)
    assert_bits(got[1], v_conic, "v_conic")
    assert_bits(got[2], v_colors, "v_colors")
    assert_ulp(got[0], v_xy, "v_xy")
    assert_ulp(got[3], v_op, "v_opacity")
    for a, b in zip(got[:4], again[:4]):
        assert a.tobytes() == b.tobytes(), "two calls differ"
