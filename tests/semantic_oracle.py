"""The label-vote contract of DESIGN.md section 6q restated in numpy, for tests/test_semantic_cpu.py and
tests/test_gpu_semantic.py.

The weight.  For a camera, a pixel p and a Gaussian g on the pixel's 16x16 tile list, vis_g(p) is the float32 weight
with which the forward compositing kernel blends g into p (`vis` of fwd_chunk in csrc/raster.hip: |T_old| - |T_new|; 0
for a Gaussian below 1/255, for the stopping Gaussian and for finished pixels).  The tests take it from the forward
itself: one-hot colours give out_img[p, j] = vis_{4k+j}(p) exactly (one non-zero term per channel).

The votes.  votes[g, c] = sum over views, sum over the pixels p with col_v(p) = c, of rint(2^24 vis_g(p)); int64 [N, C];
2^24 vis is exact in float32, rint is round-half-to-even, vis < 1.  col_v(p) = class_map[label_v(p)] with label_v the
view's uint8 [H, W] map and class_map uint8 [256] sending a label to a column 0 .. C-1 or to 255 (the pixel does not
vote); 1 <= C <= 255; without a map every pixel of the image is column 0.

Labels from votes.  top[g] = the largest column of row g, ties to the smaller column; total[g] = the row sum;
label[g] = argmax if total > 0 and double(top) >= min_share * double(total), else 255;
confidence[g] = float32(double(top) / double(total)), 0 where total = 0.
"""
import numpy as np

NONE = 255
SCALE = float(1 << 24)


def quantise(weights):
    """float32 weights -> int64 rint(2^24 w) (numpy's rint rounds half to even; the product is exact in float64)."""
    w = np.asarray(weights)
    assert w.dtype == np.float32
    return np.rint(w.astype(np.float64) * SCALE).astype(np.int64)


def columns(label_map, class_map, num_classes):
    """uint8 [H, W] labels -> the pixels' columns (255: no vote)."""
    col = np.asarray(class_map, dtype=np.uint8)[np.asarray(label_map, dtype=np.uint8)].astype(np.int64)
    col[col >= num_classes] = NONE
    return col


def votes_from_table(table, col, num_classes):
    """table float32 [N, H, W] of weights, col int [H, W] (255: no vote; None: all column 0) -> int64 [N, C]."""
    q = quantise(table)
    n = q.shape[0]
    votes = np.zeros((n, num_classes), dtype=np.int64)
    if col is None:
        votes[:, 0] = q.reshape(n, -1).sum(axis=1)
        return votes
    for c in np.unique(col):
        if c != NONE:
            votes[:, int(c)] = q[:, col == c].sum(axis=1)
    return votes


def labels_from_votes(votes, min_share=0.0):
    """int64 [N, C] -> (labels uint8 [N], confidence float32 [N], top int64 [N], total int64 [N])."""
    votes = np.asarray(votes, dtype=np.int64)
    arg = votes.argmax(axis=1)                               # numpy's argmax is the first maximum
    top = votes[np.arange(votes.shape[0]), arg]
    total = votes.sum(axis=1)
    ok = (total > 0) & (top.astype(np.float64) >= np.float64(min_share) * total.astype(np.float64))
    labels = np.where(ok, arg, NONE).astype(np.uint8)
    with np.errstate(divide="ignore", invalid="ignore"):
        conf = np.where(total > 0, top.astype(np.float64) / np.maximum(total, 1).astype(np.float64), 0.0)
    return labels, conf.astype(np.float32), top, total


def class_sums(table, labels, num_classes):
    """float64 [num_classes, H, W]: per pixel the summed weights of the Gaussians carrying each label."""
    t = np.asarray(table, dtype=np.float64)
    out = np.zeros((num_classes,) + t.shape[1:], dtype=np.float64)
    for c in range(num_classes):
        sel = np.asarray(labels) == c
        if sel.any():
            out[c] = t[sel].sum(axis=0)
    return out


def rendered_labels(sums):
    """-> (uint8 [H, W]: first largest class, 255 where no class has weight; float64 [H, W]: top minus runner-up)."""
    arg = sums.argmax(axis=0)
    ordered = np.sort(sums, axis=0)
    top = ordered[-1]
    second = ordered[-2] if sums.shape[0] > 1 else np.zeros_like(top)
    return np.where(top > 0, arg, NONE).astype(np.uint8), top - second


def iou(pred, target, num_classes, ignore=255):
    """-> (float64 [num_classes] with NaN where the union is empty, mean over the classes that occur in target)."""
    pred, target = np.asarray(pred).reshape(-1), np.asarray(target).reshape(-1)
    valid = target != ignore
    pred, target = pred[valid], target[valid]
    out = np.full(num_classes, np.nan)
    occurs = []
    for c in range(num_classes):
        inter = int(((pred == c) & (target == c)).sum())
        union = int(((pred == c) | (target == c)).sum())
        if union:
            out[c] = inter / union
        if (target == c).any():
            occurs.append(c)
    return out, (float(np.mean(out[occurs])) if occurs else float("nan"))
