#!/usr/bin/env python
"""Trains a scene from a COLMAP reconstruction and saves it.

    python tools/train.py --dataset-dir datasets/train --max-iter 10000 --output scene.ply

The flow of the reference's scripts/train.py: ``Dataset`` reads
``<dataset-dir>/<colmap-path>`` (cameras.bin, images.bin, points3D.bin) and undistorts the images of
``<dataset-dir>/<images-path>`` on the GPU, ``from_pcd`` starts the model from the sparse points, ``fit`` trains it
with densification every ``len(cameras)`` steps (train.py:277), and the result is written as a 3DGS PLY (``.ply``), a
checkpoint (``.pth`` / ``.pt``) or a ``.splat`` file, told apart by the extension of ``--output``.  ``--viewer`` serves the
scene while it trains (``tinysplat_amd.Viewer``, the reference's websocket protocol; it is off unless asked for): a pending
request is rendered between two steps.  ``--eval-holdout N`` keeps every N-th camera (by image name) out of training and
prints the reference's metrics table for those views - PSNR, SSIM, L1 and the number of Gaussians - every
``--eval-interval`` steps (default: one epoch of the training cameras) and after the last step; ``--metrics-csv`` also
appends the rows to a file.  ``--regularize-depth`` adds the reference's depth term (train.py:65-69): the monocular depth
maps ``<dataset-dir>/<depths-path>/<image name>.npy``, made with any model, are scale-matched to the SfM points on the GPU
(``tinysplat_amd.DepthPriors``) and weigh in with ``--lambda-depth`` from step ``--regularize-depth-start`` to
``--regularize-depth-end``; a camera without a usable map trains without the term, held-out views get none, and
``--depth-fits-csv`` writes the table of fits.  Without the flag the run is what it was.  ``--strategy mcmc`` replaces the
reference's clone / split / prune with budgeted densification (``tinysplat_amd.McmcDensifier``): dead Gaussians are moved
onto live ones and the set grows to exactly ``--max-gaussians``; ``--means-lr-final`` decays the means' learning rate
log-linearly over the run (off unless given).  ``--appearance affine|grid`` trains a colour transform per training image
between the render and the loss (``tinysplat_amd.AppearanceModel``: a 3x4 exposure matrix, or a bilateral grid of
``--appearance-grid L H W`` of them) so that exposure and white balance that change from photo to photo do not end up in the
scene; ``--appearance-out`` saves the transforms, and with ``--eval-holdout`` the table is also printed (and written to
``<metrics-csv stem>_cc.csv``) for renders mapped to their targets by a least-squares affine colour fit, since held-out
views have no transform.  ``--optimize-poses`` refines every training camera's pose with the scene (``tinysplat_amd.PoseModel``:
an SE(3) correction per view, ``--pose-lr`` for both rates, ``--pose-reg`` its decay towards the identity), prints the table of
corrections at the end and saves them with ``--poses-out``; the saved scene then lives in the refined cameras' frame, so with
``--eval-holdout`` every held-out view is first aligned to its image by ``--eval-refine-poses K`` steps with the Gaussians
frozen (30 unless given; 0 and without ``--optimize-poses``: the cameras as they are).  ``--masks-dir D`` reads one mask per
photo from ``<dataset-dir>/D`` (``a.jpg.png``, COLMAP's ``mask_path`` convention, then ``a.png``, then ``a.jpg.npy``; nonzero
keeps the pixel; a mask of the photo's size is undistorted with it) and ``--mask-classes a,b`` with ``--semantic-dir D`` ignores
those classes of the label maps ``<dataset-dir>/D/<image name>.npy``, grown by ``--mask-dilate`` pixels (10, the SSIM
window's reach); both together combine.  Ignored pixels take no part in the loss (``tinysplat_amd.masks``), and with
``--eval-holdout`` the held-out views are measured over their kept pixels only.  Flags the reference's parser has keep
its names and defaults.  Needs a GPU: there is no CPU path.
"""
import argparse
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

WRITERS = {".ply": "export_ply", ".pth": "save_checkpoint", ".pt": "save_checkpoint", ".splat": "export_splat"}


def _depth_parser():
    ap = argparse.ArgumentParser(add_help=False, allow_abbrev=False)
    g = ap.add_argument_group("depth prior")
    g.add_argument("--regularize-depth", action="store_true", help="train with scale-matched monocular depth targets")
    g.add_argument("--depths-path", type=str, default="depths", help="below --dataset-dir: <image name>.npy per camera")
    g.add_argument("--lambda-depth", type=float, default=0.2)
    g.add_argument("--regularize-depth-start", type=int, default=1)
    g.add_argument("--regularize-depth-end", type=int, default=15000)
    g.add_argument("--depth-space", choices=("depth", "disparity"), default="depth",
                   help="what the stored maps hold; disparity: the target is 1 / (s D + t)")
    g.add_argument("--depth-fits-csv", type=str, default=None, help="write the per-camera fits to this CSV file")
    return ap


def parse_depth(argv=None):
    """The depth prior's options, a namespace of their own: ``parse`` keeps returning the options it always has."""
    ap = _depth_parser()
    args, _rest = ap.parse_known_args(argv)
    if args.lambda_depth < 0 or args.regularize_depth_start < 1 or args.regularize_depth_end < args.regularize_depth_start:
        ap.error("--lambda-depth must not be negative, and 1 <= --regularize-depth-start <= --regularize-depth-end")
    if args.depth_fits_csv is not None and not args.regularize_depth:
        ap.error("--depth-fits-csv needs --regularize-depth")
    return args


def _strategy_parser():
    ap = argparse.ArgumentParser(add_help=False, allow_abbrev=False)
    g = ap.add_argument_group("densification strategy")
    g.add_argument("--strategy", choices=("reference", "mcmc"), default="reference",
                   help="reference: the reference's clone / split / prune; mcmc: relocation and growth to --max-gaussians")
    g.add_argument("--max-gaussians", type=int, default=1_000_000, help="the cap of --strategy mcmc (cap_max)")
    g.add_argument("--means-lr-final", type=float, default=None,
                   help="decay the means' learning rate log-linearly to this value over --max-iter steps")
    return ap


def parse_strategy(argv=None):
    """The densification strategy's options, a namespace of their own like the depth prior's."""
    ap = _strategy_parser()
    args, _rest = ap.parse_known_args(argv)
    if args.max_gaussians < 1 or (args.means_lr_final is not None and not args.means_lr_final > 0):
        ap.error("--max-gaussians must be at least 1 and --means-lr-final positive")
    return args


def _appearance_parser():
    ap = argparse.ArgumentParser(add_help=False, allow_abbrev=False)
    g = ap.add_argument_group("per-view appearance")
    g.add_argument("--appearance", choices=("none", "affine", "grid"), default="none",
                   help="a colour transform per training image: affine, one 3x4 matrix; grid, a bilateral grid of them")
    g.add_argument("--appearance-grid", type=int, nargs=3, default=None, metavar=("L", "H", "W"),
                   help="luminance levels, rows and columns of --appearance grid (default 8 16 16)")
    g.add_argument("--appearance-lr", type=float, default=2e-3)
    g.add_argument("--appearance-tv", type=float, default=10.0, help="weight of the grids' total variation")
    g.add_argument("--appearance-out", type=str, default=None, help="save the trained transforms to this file")
    return ap


def parse_appearance(argv=None):
    """The appearance model's options, a namespace of their own like the depth prior's."""
    ap = _appearance_parser()
    args, _rest = ap.parse_known_args(argv)
    if args.appearance_grid is not None and args.appearance != "grid":
        ap.error("--appearance-grid needs --appearance grid")
    if args.appearance_grid is None:
        args.appearance_grid = [8, 16, 16]
    if min(args.appearance_grid) < 1 or args.appearance_lr < 0 or args.appearance_tv < 0:
        ap.error("--appearance-grid needs sizes of at least 1; --appearance-lr and --appearance-tv must not be negative")
    if args.appearance_out is not None and args.appearance == "none":
        ap.error("--appearance-out needs --appearance affine or grid")
    return args


def appearance_config(args):
    """The ``AppearanceConfig`` of the parsed options; None for ``--appearance none``."""
    if args.appearance == "none":
        return None
    from tinysplat_amd.appearance import AppearanceConfig
    grid = (1, 1, 1) if args.appearance == "affine" else tuple(args.appearance_grid)
    return AppearanceConfig(grid=grid, lr=args.appearance_lr, tv_weight=args.appearance_tv)


def _pose_parser():
    ap = argparse.ArgumentParser(add_help=False, allow_abbrev=False)
    g = ap.add_argument_group("camera pose refinement")
    g.add_argument("--optimize-poses", action="store_true", help="refine the training cameras' poses with the scene")
    g.add_argument("--pose-lr", type=float, default=1e-5, help="Adam rate of a pose's translation and rotation")
    g.add_argument("--pose-reg", type=float, default=1e-6, help="decay of a correction towards the identity")
    g.add_argument("--poses-out", type=str, default=None, help="save the trained corrections to this file")
    g.add_argument("--eval-refine-poses", type=int, default=None, metavar="K",
                   help="align every held-out view by K pose steps before it is measured (30 with --optimize-poses, else 0)")
    return ap


EVAL_REFINE_STEPS = 30           # --eval-refine-poses where --optimize-poses and --eval-holdout are both given


def parse_pose(argv=None):
    """The pose refinement's options, a namespace of their own like the depth prior's."""
    ap = _pose_parser()
    args, _rest = ap.parse_known_args(argv)
    if args.pose_lr < 0 or args.pose_reg < 0 or (args.eval_refine_poses is not None and args.eval_refine_poses < 0):
        ap.error("--pose-lr, --pose-reg and --eval-refine-poses must not be negative")
    if args.poses_out is not None and not args.optimize_poses:
        ap.error("--poses-out needs --optimize-poses")
    if args.eval_refine_poses is None:
        args.eval_refine_poses = EVAL_REFINE_STEPS if args.optimize_poses else 0
    return args


def print_corrections(poses, cameras) -> None:
    """The table of the trained corrections: per view its rotation angle and the length of its translation."""
    import numpy as np
    table = poses.corrections()
    print(f"{'camera':<32} {'steps':>7} {'rotation (deg)':>15} {'translation':>12}")
    for i, (angle, shift) in enumerate(table):
        print(f"{str(getattr(cameras[i], 'name', i)):<32} {poses.steps[i]:>7} {np.degrees(angle):>15.5f} {shift:>12.6f}")
    print(f"{'mean':<32} {'':>7} {np.degrees(table[:, 0].mean()):>15.5f} {table[:, 1].mean():>12.6f}")


def _mask_parser():
    ap = argparse.ArgumentParser(add_help=False, allow_abbrev=False)
    add_mask_arguments(ap.add_argument_group("masks"))
    return ap


def add_mask_arguments(g, semantic: bool = True):
    """The mask options tools/train.py and tools/eval.py share."""
    g.add_argument("--masks-dir", type=str, default=None, help="below --dataset-dir: one mask per photo, nonzero keeps")
    g.add_argument("--mask-classes", type=str, default=None, metavar="a,b",
                   help="ignore these classes of the label maps of --semantic-dir")
    g.add_argument("--mask-dilate", type=int, default=10, help="grow what --mask-classes ignores by this many pixels")
    if semantic:
        g.add_argument("--semantic-dir", type=str, default=None, help="below --dataset-dir: <image name>.npy label maps")
        g.add_argument("--semantic-classes", type=int, default=150, help="labels of the maps: 0 .. this - 1, 255 ignored")


def mask_classes(args, error):
    """--mask-classes as a list of labels, checked -> [] where not given."""
    if args.mask_classes is None:
        return []
    try:
        classes = [int(v) for v in args.mask_classes.split(",") if v.strip()]
    except ValueError:
        error("--mask-classes must be a comma-separated list of labels")
    if not classes or args.semantic_dir is None:
        error("--mask-classes needs at least one label and --semantic-dir")
    if args.mask_dilate < 0 or not 1 <= args.semantic_classes <= 255 or any(not 0 <= c < args.semantic_classes for c in classes):
        error("--mask-dilate must not be negative and the labels of --mask-classes must lie in [0, --semantic-classes)")
    return classes


def parse_masks(argv=None):
    """The mask options, a namespace of its own like the depth prior's; ``classes`` holds the labels to drop."""
    ap = _mask_parser()
    args = ap.parse_known_args(argv)[0]
    args.classes = mask_classes(args, ap.error)
    return args


def _frame_parser():
    ap = argparse.ArgumentParser(add_help=False, allow_abbrev=False)
    g = ap.add_argument_group("scene frame")
    g.add_argument("--normalize-scene", action="store_true",
                   help="train in a frame with z up, the cameras centred and the farthest one at distance 1 "
                        "(edit.orient_from_cameras); the transform is printed as a 4x4 matrix")
    return ap


def parse_frame(argv=None):
    """The scene frame's option, a namespace of its own like the depth prior's."""
    return _frame_parser().parse_known_args(argv)[0]


def _render_parser():
    ap = argparse.ArgumentParser(add_help=False, allow_abbrev=False)
    g = ap.add_argument_group("rendering")
    g.add_argument("--antialiased", action="store_true",
                   help="train and evaluate in the antialiased mode: every opacity is scaled by sqrt(det(cov2d) / "
                        "det(cov2d + 0.3 I)), so that the 2D low-pass spreads a Gaussian's energy and adds none; a .ply "
                        "output records the mode")
    return ap


def parse_render(argv=None):
    """The rasterize mode's option, a namespace of its own like the depth prior's."""
    return _render_parser().parse_known_args(argv)[0]


def parse(argv=None):
    depth_ap, strategy_ap, appearance_ap = _depth_parser(), _strategy_parser(), _appearance_parser()
    parse_depth(argv)                                          # checks the depth prior's options
    parse_strategy(argv)
    parse_appearance(argv)
    _depth, argv = depth_ap.parse_known_args(argv)
    _strategy, argv = strategy_ap.parse_known_args(argv)
    _appearance, argv = appearance_ap.parse_known_args(argv)
    _frame, argv = _frame_parser().parse_known_args(argv)
    _render, argv = _render_parser().parse_known_args(argv)
    parse_masks(argv)
    _masks, argv = _mask_parser().parse_known_args(argv)
    parse_pose(argv)
    pose_ap = _pose_parser()
    _pose, argv = pose_ap.parse_known_args(argv)
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter,
                                 epilog=depth_ap.format_help().split("\n\n", 1)[-1] + "\n" +
                                 strategy_ap.format_help().split("\n\n", 1)[-1] + "\n" +
                                 appearance_ap.format_help().split("\n\n", 1)[-1] + "\n" +
                                 _frame_parser().format_help().split("\n\n", 1)[-1] + "\n" +
                                 _render_parser().format_help().split("\n\n", 1)[-1] + "\n" +
                                 _mask_parser().format_help().split("\n\n", 1)[-1] + "\n" +
                                 pose_ap.format_help().split("\n\n", 1)[-1])
    ap.add_argument("--device", type=str, default="cuda:0")
    ap.add_argument("--sh-degree", type=int, default=3)
    ap.add_argument("--max-iter", type=int, default=10_000)
    ap.add_argument("--dataset-dir", type=str, default="datasets/train")
    ap.add_argument("--colmap-path", type=str, default="colmap/sparse/0", help="below --dataset-dir")
    ap.add_argument("--images-path", type=str, default="images", help="below --dataset-dir")
    ap.add_argument("--max-image-dimension", type=int, default=None,
                    help="downscale the targets so that their longer side is at most this many pixels")
    ap.add_argument("--principal-point", choices=("reference", "center"), default="reference",
                    help="reference: the reference's camera matrices; center: recentre the images on the principal point")
    ap.add_argument("--output", type=str, default="scene.ply", help="scene.ply, scene.pth or scene.splat")
    ap.add_argument("--viewer", action="store_true", help="serve the scene to a websocket viewer while it trains")
    ap.add_argument("--viewer-ip", type=str, default="127.0.0.1")
    ap.add_argument("--viewer-port", type=int, default=8765)
    ap.add_argument("--eval-holdout", type=int, default=0,
                    help="hold every N-th camera (sorted by image name) out of training and evaluate on them; 0: none")
    ap.add_argument("--eval-interval", type=int, default=None,
                    help="steps between two evaluations (default: the number of training cameras, one epoch)")
    ap.add_argument("--metrics-csv", type=str, default=None, help="append the evaluation rows to this CSV file")
    args = ap.parse_args(argv)
    if Path(args.output).suffix.lower() not in WRITERS:
        ap.error(f"--output must end in one of {', '.join(WRITERS)}")
    if args.max_iter < 0 or (args.max_image_dimension is not None and args.max_image_dimension < 1):
        ap.error("--max-iter must not be negative and --max-image-dimension must be at least 1")
    if args.eval_holdout < 0 or (args.eval_interval is not None and args.eval_interval < 1):
        ap.error("--eval-holdout must not be negative and --eval-interval must be at least 1")
    if args.eval_holdout == 0 and (args.eval_interval is not None or args.metrics_csv is not None):
        ap.error("--eval-interval and --metrics-csv need --eval-holdout")
    return args


def normalize_scene(dataset):
    """Moves the dataset's cameras and point cloud into the frame of ``orient_from_cameras`` and prints the transform."""
    from tinysplat_amd.edit import orient_from_cameras, transform_cameras, transform_points
    t = orient_from_cameras(dataset.cameras)
    dataset.cameras = transform_cameras(dataset.cameras, t)
    dataset.pcd.xyz = transform_points(dataset.pcd.xyz, t)
    dataset.spatial_extent *= t.scale
    print("scene transform:\n" + "\n".join(" ".join(f"{v: .9g}" for v in row) for row in t.matrix()))
    return t


def main(argv=None):
    args, depth, strategy, look = parse(argv), parse_depth(argv), parse_strategy(argv), parse_appearance(argv)
    posing, masking = parse_pose(argv), parse_masks(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: tinysplat_amd has no CPU path")
    from tinysplat_amd import Dataset, formats, from_pcd
    from tinysplat_amd.densify import DensifyConfig, Densifier
    from tinysplat_amd.training import fit
    base = Path(args.dataset_dir)
    dataset = Dataset(base / args.colmap_path, base / args.images_path, max_image_dimension=args.max_image_dimension,
                      device=args.device, principal_point=args.principal_point)
    print(f"{len(dataset.cameras)} cameras ({sum(dataset.resampled)} resampled), {dataset.pcd.xyz.shape[0]} points, "
          f"extent {dataset.spatial_extent:.3f}")
    if parse_frame(argv).normalize_scene:
        normalize_scene(dataset)
    model = from_pcd(dataset.pcd, sh_degree=args.sh_degree, device=args.device)
    if parse_render(argv).antialiased:
        model.rasterize_mode = "antialiased"
    cameras, targets, evaluator, corrected = dataset.cameras, dataset.targets, None, None
    masks = held_masks = None
    if masking.masks_dir is not None or masking.classes:
        from tinysplat_amd.masks import dataset_masks, mask_coverage
        masks = dataset_masks(dataset, None if masking.masks_dir is None else base / masking.masks_dir,
                              None if masking.semantic_dir is None else base / masking.semantic_dir, masking.classes,
                              masking.mask_dilate, masking.semantic_classes, args.device)
        shares = [mask_coverage(m) for m in masks]
        print(f"masks for {len(masks)} cameras: {100.0 * sum(shares) / len(shares):.1f} % of the pixels kept "
              f"(least {100.0 * min(shares):.1f} %)")
    depth_targets = depth_schedule = None
    if depth.regularize_depth:
        from tinysplat_amd import DepthPriors
        from tinysplat_amd.training import Scheduler
        priors = DepthPriors(dataset, dataset.pcd, base / depth.depths_path, space=depth.depth_space)
        depth_targets = priors.targets
        depth_schedule = Scheduler(True, depth.regularize_depth_start, depth.regularize_depth_end)
        print(f"depth priors for {sum(t is not None for t in depth_targets)} of {len(cameras)} cameras")
        if depth.depth_fits_csv:
            priors.write_csv(depth.depth_fits_csv)
    if args.eval_holdout:
        from tinysplat_amd import Evaluator, holdout_split
        from tinysplat_amd.dataset import Targets
        train, test = holdout_split([c.name for c in cameras], args.eval_holdout)
        if not train or not test:
            raise SystemExit(f"--eval-holdout {args.eval_holdout} leaves {len(train)} training and {len(test)} held-out cameras")
        held = ([cameras[i] for i in test], Targets([targets.images_u8[i] for i in test]))
        cameras, targets = [cameras[i] for i in train], Targets([targets.images_u8[i] for i in train])
        depth_targets = None if depth_targets is None else [depth_targets[i] for i in train]
        if masks is not None:
            masks, held_masks = [masks[i] for i in train], [masks[i] for i in test]
        masked = {} if held_masks is None else {"masks": held_masks}
        evaluator = Evaluator(model, *held, args.device, args.eval_interval or len(cameras),
                              on_result=lambda row, _result: print(Evaluator.format(row), flush=True),
                              csv_path=args.metrics_csv, refine_poses=posing.eval_refine_poses, **masked)
        if look.appearance != "none":                         # held-out views have no transform: also measure them colour-corrected
            cc_csv = None if args.metrics_csv is None else \
                str(Path(args.metrics_csv).with_name(Path(args.metrics_csv).stem + "_cc" + Path(args.metrics_csv).suffix))
            corrected = Evaluator(model, *held, args.device, args.eval_interval or len(cameras), csv_path=cc_csv,
                                  on_result=lambda row, _result: print("colour-corrected | " + Evaluator.format(row), flush=True),
                                  color_correct=True, refine_poses=posing.eval_refine_poses, **masked)
        print(f"{len(cameras)} training cameras, {len(test)} held out")
    if strategy.strategy == "mcmc":
        from tinysplat_amd.mcmc import McmcConfig, McmcDensifier
        densifier = McmcDensifier(model, McmcConfig(cap_max=strategy.max_gaussians))
    else:
        densifier = Densifier(model, DensifyConfig(interval_densify=len(cameras)))      # train.py:277
    lr_schedule = None
    if strategy.means_lr_final is not None:
        from tinysplat_amd.mcmc import ExponentialLr
        from tinysplat_amd.training import DEFAULT_LRS
        lr_schedule = ExponentialLr(DEFAULT_LRS["means"], strategy.means_lr_final, max(args.max_iter, 1))
    viewer = None
    if args.viewer:
        from tinysplat_amd import Viewer
        from tinysplat_amd.viewer import ViewRenderer
        viewer = Viewer(ViewRenderer(model, dataset.cameras[0], args.device), args.viewer_ip, args.viewer_port)
        print(f"viewer on ws://{args.viewer_ip}:{viewer.port}")
    callbacks = [f for f in (evaluator, corrected, viewer.service if viewer else None) if f is not None]
    appearance = None
    if look.appearance != "none":
        from tinysplat_amd.appearance import AppearanceModel
        appearance = AppearanceModel(len(cameras), appearance_config(look), args.device)
        print(f"appearance: {len(cameras)} grids of {'x'.join(map(str, appearance.config.grid))} colour matrices")
    poses = None
    if posing.optimize_poses:
        from tinysplat_amd.pose import PoseConfig, PoseModel
        poses = PoseModel(cameras, PoseConfig(lr_translation=posing.pose_lr, lr_rotation=posing.pose_lr,
                                              weight_decay=posing.pose_reg))
        print(f"poses: {poses.num_views} corrections, rate {posing.pose_lr:g}, decay {posing.pose_reg:g}")

    def on_step(step, out):
        for f in callbacks:
            f(step, out)
    try:
        extra = {} if depth_targets is None else dict(depth_targets=depth_targets, lambda_depth=depth.lambda_depth,
                                                      depth_schedule=depth_schedule)
        if appearance is not None:
            extra["appearance"] = appearance
        if poses is not None:
            extra["poses"] = poses
        if masks is not None:
            extra["masks"] = masks
        out = fit(model, cameras, targets, args.device, args.max_iter, max_sh_degree=args.sh_degree,
                  densifier=densifier, on_step=on_step if callbacks else None, lr_schedule=lr_schedule, **extra)
    finally:
        if viewer:
            viewer.stop()
    if evaluator is not None:
        evaluator.final(args.max_iter)
    if corrected is not None:
        corrected.final(args.max_iter)
    if appearance is not None and look.appearance_out:
        appearance.save(look.appearance_out)
        print(f"wrote {look.appearance_out}: {appearance.num_views} appearance grids")
    if poses is not None:
        print_corrections(poses, cameras)
        if posing.poses_out:
            poses.save(posing.poses_out)
            print(f"wrote {posing.poses_out}: {poses.num_views} pose corrections")
    if out is not None:
        print(f"step {args.max_iter}: loss {float(out['loss']):.6f}")
        if depth_targets is not None and "depth_l1" in out:
            print(f"step {args.max_iter}: depth l1 {float(out['depth_l1']):.6f}")
    getattr(formats, WRITERS[Path(args.output).suffix.lower()])(model, args.output)
    print(f"wrote {args.output}: {Path(args.output).stat().st_size} bytes from {model.num_points} Gaussians")


if __name__ == "__main__":
    main()
