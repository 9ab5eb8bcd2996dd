"""Brute-force float64 k-nearest-neighbour oracle (CPU, chunked torch) for tinysplat_amd.knn_points.

Distances are sqrt(dx*dx + dy*dy + dz*dz) in float64 from the float32 coordinates (the kernel's formula,
and what sklearn's NearestNeighbors returns); rows are ordered by (float64 distance, index)."""
import torch


def knn_oracle(queries, points, k):
    """-> (dist float64 [m,k], idx int64 [m,k])."""
    P = torch.as_tensor(points).to(torch.float64)
    Q = torch.as_tensor(queries).to(torch.float64)
    n, m = P.shape[0], Q.shape[0]
    chunk = max(1, (1 << 22) // n)
    out_d, out_i = [], []
    ar = torch.arange(n)
    for a in range(0, m, chunk):
        q = Q[a:a + chunk]
        dx = q[:, None, 0] - P[None, :, 0]
        dy = q[:, None, 1] - P[None, :, 1]
        dz = q[:, None, 2] - P[None, :, 2]
        d = torch.sqrt(dx * dx + dy * dy + dz * dz)
        t = torch.topk(d, k, dim=1, largest=False, sorted=True).values[:, k - 1:k]       # the k-th distance
        # entries below it (fewer than k), ordered by (distance, index) ...
        below = d < t
        v, i = torch.topk(torch.where(below, d, torch.inf), k, dim=1, largest=False, sorted=True)
        o1 = torch.argsort(i, dim=1, stable=True)
        v, i = v.gather(1, o1), i.gather(1, o1)
        o2 = torch.argsort(v, dim=1, stable=True)
        v, i = v.gather(1, o2), i.gather(1, o2)
        # ... then the smallest indices at exactly the k-th distance
        at_t = torch.topk(torch.where(d == t, ar.to(torch.float64), torch.inf), k, dim=1, largest=False,
                          sorted=True).values
        nb = below.sum(dim=1, keepdim=True)
        pos = torch.arange(k)[None, :]
        take = pos < nb
        ri = torch.where(take, i, at_t.gather(1, (pos - nb).clamp(min=0)).to(torch.int64))
        rd = torch.where(take, v, t.expand(-1, k))
        out_d.append(rd)
        out_i.append(ri)
    return torch.cat(out_d), torch.cat(out_i)
