"""What ``extract.py`` and ``mesh.py`` (sections 6g and 6h) share on the Python side of the
packed-record density (csrc/density_field.h): the packed model, its neighbour search, normals and colours, and a chunk's
workspace."""
from dataclasses import dataclass

import torch
from torch import Tensor

from . import _lib
from .ops import _call, _f32c, _need_hip, _ptr, _stream

EXTRACT_K = 16                  # knn_points(..., K=16) (model_gaussian.py:260, :425)
RECORD = 10                     # TS_EXTRACT_RECORD


@dataclass
class PackedModel:
    """``ts_extract_pack`` of a model: ``records`` float32 [N,10], ``p_std`` float32 [N], and the contiguous means
    the neighbour searches run on."""
    means: Tensor
    records: Tensor
    p_std: Tensor


@torch.no_grad()
def pack_model(model) -> PackedModel:
    """Once per extraction: per Gaussian {mean, the Cholesky factor of Sigma^-1, sigmoid(opacity)} and
    ``|exp(scales)|``.  Needs at least 16 Gaussians with finite means (the reference's k-NN would fail)."""
    means, scales, quats, opac = (_f32c(t.detach()) for t in (model.means, model.scales, model.quats, model.opacities))
    dev = _need_hip(means, scales, quats, opac)
    n = means.shape[0]
    if n < EXTRACT_K:
        raise ValueError(f"the level-set extraction needs at least {EXTRACT_K} Gaussians, got {n}")
    if not bool(torch.isfinite(means).all()):
        raise ValueError("the means must be finite")
    lib = _lib.load()
    records = torch.empty((n, RECORD), dtype=torch.float32, device=dev)
    p_std = torch.empty((n,), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _call("ts_extract_pack", lib.ts_extract_pack, n, _ptr(means), _ptr(scales), _ptr(quats), _ptr(opac),
              _ptr(records), _ptr(p_std), _stream(dev))
    return PackedModel(means, records, p_std)


def align256(b: int) -> int:
    """As csrc/host_util.h: every part of a carved workspace starts on 256 bytes."""
    return (b + 255) // 256 * 256


class Workspace:
    """One ``uint8`` tensor of ``total`` bytes handed out as typed, shaped, 256-aligned views, in the order of the
    ``ts_*_chunk_bytes`` entry that gave ``total``; ``done`` asserts that the two agree."""

    def __init__(self, total: int, dev):
        self.buf = torch.empty((total,), dtype=torch.uint8, device=dev)
        self.at = 0

    def take(self, dtype, *shape) -> Tensor:
        nbytes = torch.Size(shape).numel() * dtype.itemsize
        view = self.buf[self.at:self.at + nbytes].view(dtype).view(shape)
        self.at += align256(nbytes)
        return view

    def done(self):
        assert self.at == self.buf.shape[0], (self.at, self.buf.shape[0])


def largest(fits, limit: int) -> int:
    """The largest count in 1..limit that ``fits`` (monotone), 0 if none."""
    if fits(limit):
        return limit
    lo, hi = 0, limit                       # fits(lo), not fits(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if fits(mid):
            lo = mid
        else:
            hi = mid
    return lo


def knn(lib, pk: PackedModel, queries, m: int, k: int, dist, idx, ws, stats, stream):
    """``ts_knn``: the ``k`` nearest means of the first ``m`` rows of ``queries``; ``stats`` int32 [2] or None."""
    _call("ts_knn", lib.ts_knn, pk.means.shape[0], _ptr(pk.means), m, _ptr(queries), k, _ptr(dist), _ptr(idx),
          _ptr(ws), _ptr(stats), stream)


def normals_at(lib, pk: PackedModel, points, p: int, out, dist, idx, ws, stream):
    """``-grad d / |grad d|`` at the first ``p`` rows of ``points``, over each point's own 16 neighbours."""
    knn(lib, pk, points, p, EXTRACT_K, dist, idx, ws, None, stream)
    _call("ts_extract_normals", lib.ts_extract_normals, pk.means.shape[0], p, _ptr(points), _ptr(idx),
          _ptr(pk.records), _ptr(out), stream)


def colors_at(lib, pk: PackedModel, colors_dc, colors_rest, points, normals, p: int, degree: int, out, dist, idx, ws,
              stream, search: bool = True):
    """``ts_field_colors`` at the first ``p`` rows of ``points``: the SH colour seen along ``-normals`` (None: band 0
    only), weighed over each point's own 16 neighbours.  ``search=False``: ``idx`` already holds these points'
    neighbours (``normals_at`` on the same rows just ran) and is not searched for again."""
    if search:
        knn(lib, pk, points, p, EXTRACT_K, dist, idx, ws, None, stream)
    _call("ts_field_colors", lib.ts_field_colors, pk.means.shape[0], p, _ptr(points), _ptr(normals), _ptr(idx),
          _ptr(pk.records), _ptr(colors_dc), _ptr(colors_rest), colors_rest.shape[1], degree, _ptr(out), stream)


def cat(parts, shape, dtype, dev) -> Tensor:
    """The parts in order, or an empty tensor of ``shape`` where there are none."""
    return torch.cat(parts) if parts else torch.empty(shape, dtype=dtype, device=dev)
