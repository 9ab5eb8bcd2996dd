#!/usr/bin/env python
"""Evaluates a saved scene on the views of a COLMAP dataset: PSNR, SSIM and L1 per view and their means.

    python tools/eval.py scene.ply --dataset-dir datasets/train --holdout 8

``SCENE`` is a 3DGS PLY (``.ply``), a checkpoint (``.pth`` / ``.pt``) or a ``.splat`` file, told apart by its extension.
``--holdout N`` evaluates every N-th camera by image name - the views ``tools/train.py --eval-holdout N`` kept out of
training; ``--holdout 0`` evaluates all views.  Every view is rendered on a black background and compared with its
(undistorted) image; ``--max-image-dimension`` and ``--principal-point`` must be those the scene was trained with.  SSIM
is the training loss's (pytorch_msssim: valid filtering), not the zero-padded SSIM of the 3DGS papers' tables.
``--semantic-dir D`` additionally lifts the label maps ``D/<image name>.npy`` of the TRAINING views onto the Gaussians
(``semantic.lift_labels``), renders the labels at the evaluated views and prints their mean IoU against those views'
maps.  ``--color-correct`` first maps every render to its target by a least-squares affine colour fit (3x4, per view) and
measures the result: the numbers to quote for a scene trained with ``tools/train.py --appearance``, whose held-out views
have no colour transform of their own.  ``--refine-poses K`` first aligns every evaluated view to its image by K pose steps with
the Gaussians frozen (``pose.refine_pose``): the numbers to quote for a scene trained with ``tools/train.py --optimize-poses``,
which has drifted against the held-out cameras.  ``--masks-dir D`` (one mask per photo below ``--dataset-dir``, nonzero keeps)
and ``--mask-classes a,b`` (classes of the label maps of ``--semantic-dir`` to ignore, grown by ``--mask-dilate`` pixels) measure
every view over its kept pixels only, as ``tools/train.py`` takes them; a view whose mask keeps nothing is left out of the
means.  ``--poses poses.pth`` puts the corrections that run saved onto the cameras
they were trained on (all cameras, or those ``--holdout`` leaves for training) before anything is rendered from them.  Needs
a GPU: there is no CPU path.
"""
import argparse
import csv
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))

READERS = {".ply": "load_ply", ".pth": "load_checkpoint", ".pt": "load_checkpoint", ".splat": "load_splat"}
HEADER = ("view", "psnr", "ssim", "l1", "mse")


def parse(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("scene", type=str, help="scene.ply, scene.pth or scene.splat")
    ap.add_argument("--device", type=str, default="cuda:0")
    ap.add_argument("--dataset-dir", type=str, required=True)
    ap.add_argument("--colmap-path", type=str, default="colmap/sparse/0", help="below --dataset-dir")
    ap.add_argument("--images-path", type=str, default="images", help="below --dataset-dir")
    ap.add_argument("--max-image-dimension", type=int, default=None,
                    help="downscale the targets so that their longer side is at most this many pixels")
    ap.add_argument("--principal-point", choices=("reference", "center"), default="reference")
    ap.add_argument("--holdout", type=int, default=8, help="evaluate every N-th camera by image name; 0: all of them")
    ap.add_argument("--csv", type=str, default=None, help="write the per-view table and the means to this CSV file")
    ap.add_argument("--color-correct", action="store_true",
                    help="measure every render after its least-squares affine colour fit to the target")
    ap.add_argument("--refine-poses", type=int, default=0, metavar="K",
                    help="align every evaluated view to its image by K pose steps before it is measured")
    ap.add_argument("--poses", type=str, default=None, help="pose corrections saved by tools/train.py --poses-out")
    ap.add_argument("--semantic-dir", type=str, default=None,
                    help="label maps <image name>.npy: also print the mIoU of the rendered labels on the evaluated views")
    ap.add_argument("--semantic-classes", type=int, default=150, help="labels of the maps: 0 .. this - 1, 255 ignored")
    ap.add_argument("--min-share", type=float, default=0.0, help="least share of a Gaussian's votes its class must have")
    ap.add_argument("--antialiased", action="store_true",
                    help="render in the antialiased mode (opacity compensation for the 2D low-pass), whatever the file says")
    from train import add_mask_arguments, mask_classes
    add_mask_arguments(ap, semantic=False)
    args = ap.parse_args(argv)
    args.classes = mask_classes(args, ap.error)
    if not 1 <= args.semantic_classes <= 255 or not 0.0 <= args.min_share <= 1.0:
        ap.error("--semantic-classes must be in 1..255 and --min-share in [0, 1]")
    if Path(args.scene).suffix.lower() not in READERS:
        ap.error(f"SCENE must end in one of {', '.join(READERS)}")
    if args.holdout < 0 or (args.max_image_dimension is not None and args.max_image_dimension < 1):
        ap.error("--holdout must not be negative and --max-image-dimension must be at least 1")
    if args.refine_poses < 0:
        ap.error("--refine-poses must not be negative")
    return args


def table_rows(result):
    """(view, psnr, ssim, l1, mse) per view, then the means."""
    rows = [(name, float(r[3]), float(r[2]), float(r[1]), float(r[0])) for name, r in zip(result.names, result.table)]
    return rows + [("mean", result.psnr, result.ssim, result.l1, result.mse)]


def semantic_line(model, cameras, train, views, args):
    """Lifts the TRAINING views' label maps onto the Gaussians, renders the labels at the evaluated views and compares
    them with those views' maps -> the line to print."""
    import torch
    from tinysplat_amd.semantic import SemanticMaps, label_iou, lift_labels, render_labels
    used = sorted(set(train) | set(views))
    maps = SemanticMaps([cameras[i] for i in used], args.semantic_dir, num_classes=args.semantic_classes,
                        device=args.device)
    at = {i: k for k, i in enumerate(used)}
    lifted = lift_labels(model, [cameras[i] for i in train], maps, min_share=args.min_share)
    pred = torch.cat([render_labels(model, cameras[i], lifted.labels, args.semantic_classes).reshape(-1) for i in views])
    target = torch.cat([maps.maps[at[i]].reshape(-1) for i in views])
    iou, mean = label_iou(pred, target, args.semantic_classes)
    present = int((~torch.isnan(iou)).sum())
    return (f"semantic: mIoU {mean:.5f} over the classes of {len(views)} views' maps ({present} classes with pixels), "
            f"labels lifted from {len(train)} training views")


def apply_poses(cameras, train, path):
    """Replaces the cameras the corrections at ``path`` were trained on by their refined copies -> how many."""
    import torch
    from tinysplat_amd.pose import PoseModel
    views = int(torch.load(str(path), map_location="cpu")["quats"].shape[0])
    on = train if views == len(train) else list(range(len(cameras))) if views == len(cameras) else None
    if on is None:
        raise SystemExit(f"{path} holds {views} corrections; the dataset has {len(cameras)} cameras, {len(train)} for training")
    try:
        refined = PoseModel.load(path, [cameras[i] for i in on]).cameras()
    except ValueError as e:
        raise SystemExit(f"{path}: {e}")
    for i, camera in zip(on, refined):
        cameras[i] = camera
    return views


def main(argv=None):
    args = parse(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: tinysplat_amd has no CPU path")
    from tinysplat_amd import Dataset, evaluate, formats, holdout_split
    from tinysplat_amd.dataset import Targets
    base = Path(args.dataset_dir)
    dataset = Dataset(base / args.colmap_path, base / args.images_path, max_image_dimension=args.max_image_dimension,
                      device=args.device, principal_point=args.principal_point)
    model = getattr(formats, READERS[Path(args.scene).suffix.lower()])(args.scene, args.device)
    if args.antialiased:                 # overrides what the file says (a .pth or .splat says nothing)
        model.rasterize_mode = "antialiased"
    train, test = holdout_split([c.name for c in dataset.cameras], args.holdout)
    views = test if args.holdout else train
    if args.poses:
        print(f"{apply_poses(dataset.cameras, train, args.poses)} pose corrections from {args.poses}")
    if not views:
        raise SystemExit(f"--holdout {args.holdout} selects none of the {len(dataset.cameras)} cameras")
    masked = {}
    if args.masks_dir is not None or args.classes:
        from tinysplat_amd.masks import dataset_masks
        # (--semantic-dir is taken as given here, as the label maps of the mIoU line are)
        masks = dataset_masks(dataset, None if args.masks_dir is None else base / args.masks_dir, args.semantic_dir,
                              args.classes, args.mask_dilate, args.semantic_classes, args.device)
        masked = {"masks": [masks[i] for i in views]}
    result = evaluate(model, [dataset.cameras[i] for i in views], Targets([dataset.targets.images_u8[i] for i in views]),
                      args.device, **masked, **({"color_correct": True} if args.color_correct else {}),
                      **({"refine_poses": args.refine_poses} if args.refine_poses else {}))
    rows = table_rows(result)
    width = max(len(r[0]) for r in rows)
    print(f"{'view':<{width}}  {'PSNR':>9}  {'SSIM':>8}  {'L1':>8}")
    for name, psnr, ssim, l1, _mse in rows:
        print(f"{name:<{width}}  {psnr:9.4f}  {ssim:8.5f}  {l1:8.5f}")
    print(f"{len(views)} views, {model.num_points} Gaussians" + (", colour-corrected" if args.color_correct else "")
          + (f", poses aligned by {args.refine_poses} steps" if args.refine_poses else "")
          + (", over the masks' kept pixels" if masked else "")
          + (f"; nothing kept in: {', '.join(result.empty)}" if result.empty else ""))
    if args.semantic_dir:
        print(semantic_line(model, dataset.cameras, train, views, args))
    if args.csv:
        with open(args.csv, "w", newline="") as f:
            writer = csv.writer(f)
            writer.writerow(HEADER)
            writer.writerows([r[0], *(repr(v) for v in r[1:])] for r in rows)


if __name__ == "__main__":
    main()
