"""The per-Gaussian row state and the one place that rebuilds it (DESIGN.md sections 6b, 6r).

One row per Gaussian lives in the six parameter tensors, in Adam's two moments of each (``optim``: training.Adam or any
holder of its ``params`` / ``exp_avg`` / ``exp_avg_sq`` dictionaries) and in whatever column a caller keeps beside them.
Whoever drops, permutes, copies or appends rows - densify.Densifier, mcmc.McmcDensifier, the surface regulariser's prune -
plans with ``plan``, copies with ``rebuild`` / ``gather`` (ts_gather_rows, never PyTorch indexing), rebinds with ``install``.
"""
from __future__ import annotations

import ctypes
import math

import torch
from torch import Tensor

from . import _lib
from .ops import _call, _f32c, _need_hip, _ptr, _stream

FIELDS = ("means", "colors_dc", "colors_rest", "scales", "quats", "opacities")


def row_floats(t: Tensor) -> int:
    return math.prod(t.shape[1:])


def hold(model, who: str) -> None:
    """Marks a model as having per-row state kept elsewhere (Adam moments, gradient accumulator, neighbour indices): the
    in-place reorder of a FRESH model, SplatModel.spatial_sort_, refuses such a model."""
    held = getattr(model, "held_by", None)
    if held is None:
        held = set()
        try:
            model.held_by = held
        except AttributeError:          # a foreign model class with __slots__: nothing to mark
            return
    held.add(who)


def fields_of(model):
    """-> (the six tensors by name, the names of those whose rows are not empty, N, their device)"""
    old = {f: getattr(model, f) for f in FIELDS}
    dev = _need_hip(*old.values())
    n = old["means"].shape[0]
    for f, t in old.items():
        if not t.is_contiguous() or t.dtype != torch.float32 or t.shape[0] != n:
            raise ValueError(f"{f} must be contiguous float32 with {n} rows")
    return old, [f for f in FIELDS if row_floats(old[f]) > 0], n, dev


def tables(*lists):
    """Lists of as many tensors each -> the ctypes pointer table of every list, then the row widths of the first."""
    k = len(lists[0])
    return [(ctypes.c_void_p * k)(*[t.data_ptr() for t in ts]) for ts in lists] + \
        [(ctypes.c_int32 * k)(*[row_floats(t) for t in lists[0]])]


def plan(flags: Tensor, n: int, dev):
    """ts_densify_plan over the policy bits ``flags`` (uint8 [n]) -> ((kept, cloned, split, n2), src_of): row ``r < n2`` of
    the rebuilt tensors copies row ``src_of[r]`` (int32), laid out kept | cloned | split samples.  The counts come back
    in the one host read of a rebuild: they size the tensors."""
    lib = _lib.load()
    with torch.cuda.device(dev):
        ws = torch.empty((int(lib.ts_densify_ws_ints(n)),), dtype=torch.int32, device=dev)
        counts = torch.empty((4,), dtype=torch.int32, device=dev)
        src_of = torch.empty((max(2 * n, 1),), dtype=torch.int32, device=dev)
        _call("ts_densify_plan", lib.ts_densify_plan, n, _ptr(flags), _ptr(ws), _ptr(counts), _ptr(src_of), _stream(dev))
    return tuple(int(v) for v in counts.tolist()), src_of


def gather(src, dst, dst_rows: int, copy_rows: int, src_of: Tensor, dev) -> None:
    """One ts_gather_rows launch over the tensor pairs: ``dst[i][r] = src[i][src_of[r]]`` for ``r < copy_rows``, zero for
    the rows from there to ``dst_rows``."""
    sp, dp, widths = tables(src, dst)
    with torch.cuda.device(dev):
        _call("ts_gather_rows", _lib.load().ts_gather_rows, len(src), sp, dp, widths, int(dst_rows), int(copy_rows),
              _ptr(src_of), _stream(dev))


def rebuild(old, live, optim, src_of: Tensor, rows: int, copy_params: int, copy_moments: int):
    """``old, live`` of ``fields_of`` -> (new, new_m, new_v): fresh parameter, exp_avg and exp_avg_sq tensors of ``rows``
    rows by field name, the first ``copy_params`` / ``copy_moments`` rows gathered through ``src_of`` and the others
    zero.  Nothing is installed: the caller may still write the rows it makes itself."""
    dev, out = src_of.device, []
    for src, copy_rows in ((old, copy_params), (optim.exp_avg, copy_moments), (optim.exp_avg_sq, copy_moments)):
        dst = {f: torch.empty((rows,) + tuple(old[f].shape[1:]), dtype=torch.float32, device=dev) for f in FIELDS}
        gather([src[f] for f in live], [dst[f] for f in live], rows, copy_rows, src_of, dev)
        out.append(dst)
    return out


def install(model, optim, new, new_m, new_v) -> None:
    """Rebinds the model's six tensors and the optimiser's three dictionaries to rebuilt ones (never a swap through
    ``.data``: identity keyed caches must see new tensors); ``requires_grad`` is carried over."""
    for f in FIELDS:
        p = new[f].requires_grad_(getattr(model, f).requires_grad)
        setattr(model, f, p)
        optim.params[f] = p
        optim.exp_avg[f] = new_m[f]
        optim.exp_avg_sq[f] = new_v[f]


@torch.no_grad()
def compact(model, optim, mask: Tensor, append=None):
    """model_gaussian.py:197-242: drops the rows where ``mask`` is True and appends the caller's rows -> (kept, src_of).
    Layout kept | appended, exactly the reference's ``cat((param[~mask], tensors[name]))``; Adam moments of appended rows
    are zero.  ``append`` may name any subset of the six fields; missing ones append nothing, and all given ones must
    append the same number of rows (the reference would build ragged parameters otherwise).  With nothing to drop or
    append the tensors stay the same objects.  A column of the caller's own survives as its rows ``src_of[:kept]``."""
    old, live, n, dev = fields_of(model)
    if mask.dtype != torch.bool or mask.shape != (n,):
        raise ValueError("mask must be bool [N]")
    made = {}
    for f, t in (append or {}).items():
        if f not in FIELDS:
            raise KeyError(f"unknown parameter {f!r}")
        want = tuple(old[f].shape[1:])
        if tuple(t.shape[1:]) != want:
            raise ValueError(f"{f}: rows must have shape {want}")
        made[f] = _f32c(t.detach().to(dev))
    counts = {f: made[f].shape[0] for f in live if f in made}
    extra = max(counts.values(), default=0)
    if extra > 0 and (set(counts) != set(live) or set(counts.values()) != {extra}):
        raise ValueError("every parameter must append the same number of rows")
    (kept, _, _, _), src_of = plan(mask.to(device=dev, dtype=torch.uint8) * 4, n, dev)         # TS_DENSIFY_PRUNE
    if kept < n or extra > 0:
        new, new_m, new_v = rebuild(old, live, optim, src_of, kept + extra, kept, kept)
        if extra > 0:
            for f in live:
                new[f][kept:].copy_(made[f])
        install(model, optim, new, new_m, new_v)
    return kept, src_of
