#!/usr/bin/env python
"""Exports a trained scene to a file other tools read.

    python tools/export.py input_file output_file --filetype PLY|SPLAT|OBJ|MESH_PLY [options]
    python tools/export.py scene.ply mesh.ply --filetype MESH_PLY --mesher tsdf --dataset-dir DATASET

``input_file``: a checkpoint (``.pth`` / ``.pt``, what training saves) or a 3DGS PLY (``.ply``), told apart by the
extension.  File types:

  PLY       the 3DGS point file (``formats.export_ply``): every tensor, 4 (17 + 3 (K - 1)) bytes per Gaussian
  SPLAT     the 32-byte-per-Gaussian file the WebGL viewers stream (``formats.export_splat``): view-independent colour
            only, most important Gaussians first; ``--limit N`` keeps the N most important
  OBJ       the iso-surface mesh (``extract_mesh``) as a Wavefront OBJ
  MESH_PLY  the same mesh as a binary PLY

The mesh types take ``--resolution`` (cells along the longest axis), ``--target-faces`` (simplify to a budget) and
``--colors`` (vertex colours from the spherical harmonics).  ``--mesher density`` (the default) meshes the SuGaR density,
a surface only for a scene trained with ``--regularize-density``; ``--mesher tsdf`` fuses the depth renders of the
cameras of ``--dataset-dir`` (its COLMAP reconstruction below ``--colmap-path``) into a truncated signed distance volume
and meshes that (``extract_mesh_tsdf``: any scene that renders good depth; no vertex colours).

``--semantic-dir D`` (with ``--dataset-dir``) cuts the scene by class before any of this: the label maps
``D/<image name>.npy`` (``semantic.SemanticMaps``) of the dataset's cameras are lifted onto the Gaussians
(``lift_labels``, all ``--semantic-classes`` classes voting) and only the Gaussians whose class is one of
``--keep-classes a,b,...`` - or all but those of ``--drop-classes a,b,...``, unlabelled ones included - are exported; ``--min-share S`` leaves a Gaussian unlabelled whose top class has less than
that share of its votes.

``--rotate w,x,y,z``, ``--translate x,y,z`` and ``--scale s`` together form one similarity ``x' = s R x + t`` that moves
the scene (``edit.transform_gaussians``: means, scales, rotations and the spherical harmonics of every band);
``--orient-cameras`` (with ``--dataset-dir``) first turns the cameras' mean up direction to +z, centres them and scales
the farthest one to distance 1 (``edit.orient_from_cameras``), and the manual similarity is applied after it.
``--crop-box cx,cy,cz,hx,hy,hz`` keeps the Gaussians whose mean is inside the axis-aligned box of that centre and those
half extents in the NEW frame.  Order: class cut, transform, crop, export; ``--mesher tsdf`` renders from the cameras moved
with the scene.  Needs a GPU: there is no CPU path.
"""
import argparse
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

FILETYPES = ("PLY", "SPLAT", "OBJ", "MESH_PLY")


def parse(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("input_file", help="checkpoint (.pth, .pt) or 3DGS PLY (.ply)")
    ap.add_argument("output_file")
    ap.add_argument("--filetype", choices=FILETYPES, required=True)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--limit", type=int, default=None, help="SPLAT: keep the N most important Gaussians")
    ap.add_argument("--resolution", type=int, default=None, help="OBJ, MESH_PLY: cells along the longest axis")
    ap.add_argument("--target-faces", type=int, default=None, help="OBJ, MESH_PLY: simplify to at most this many faces")
    ap.add_argument("--colors", action="store_true", help="OBJ, MESH_PLY: vertex colours")
    ap.add_argument("--mesher", choices=("density", "tsdf"), default="density",
                    help="OBJ, MESH_PLY: the density's level set, or the fusion of the cameras' depth renders")
    ap.add_argument("--dataset-dir", type=str, default=None, help="--mesher tsdf, --semantic-dir: the reconstruction whose cameras render")
    ap.add_argument("--colmap-path", type=str, default="colmap/sparse/0", help="below --dataset-dir")
    ap.add_argument("--semantic-dir", type=str, default=None, help="label maps <image name>.npy; needs --dataset-dir")
    ap.add_argument("--semantic-classes", type=int, default=150, help="labels of the maps: 0 .. this - 1, 255 ignored")
    ap.add_argument("--keep-classes", type=class_list, default=None, help="a,b,...: export the Gaussians of these classes")
    ap.add_argument("--drop-classes", type=class_list, default=None, help="a,b,...: export all but these classes")
    ap.add_argument("--min-share", type=float, default=0.0, help="least share of a Gaussian's votes its class must have")
    ap.add_argument("--rotate", type=float_list(4), default=None, help="w,x,y,z: rotate the scene by this quaternion")
    ap.add_argument("--translate", type=float_list(3), default=None, help="x,y,z: move the scene (after rotation and scale)")
    ap.add_argument("--scale", type=float, default=None, help="scale the scene about the origin")
    ap.add_argument("--orient-cameras", action="store_true",
                    help="z up, centred and unit-sized by the cameras of --dataset-dir, before the manual transform")
    ap.add_argument("--crop-box", type=float_list(6), default=None,
                    help="cx,cy,cz,hx,hy,hz: keep the Gaussians inside this axis-aligned box of the new frame")
    ap.add_argument("--antialiased", action="store_true",
                    help="treat the input as a model of the antialiased mode (opacity compensation for the 2D low-pass), "
                         "whatever the file says: the depth renders of --mesher tsdf and the votes of --semantic-dir "
                         "follow it, and a PLY output records it")
    args = ap.parse_args(argv)
    mesh = args.filetype in ("OBJ", "MESH_PLY")
    if args.limit is not None and args.filetype != "SPLAT":
        ap.error("--limit goes with --filetype SPLAT")
    if args.limit is not None and args.limit < 0:
        ap.error("--limit must not be negative")
    if not mesh and (args.resolution is not None or args.target_faces is not None or args.colors):
        ap.error("--resolution, --target-faces and --colors go with --filetype OBJ or MESH_PLY")
    if args.mesher == "tsdf" and not mesh:
        ap.error("--mesher goes with --filetype OBJ or MESH_PLY")
    if args.semantic_dir is not None and args.dataset_dir is None:
        ap.error("--semantic-dir needs --dataset-dir")
    if args.keep_classes is not None and args.drop_classes is not None:
        ap.error("--keep-classes and --drop-classes exclude each other")
    if (args.semantic_dir is not None) != (args.keep_classes is not None or args.drop_classes is not None):
        ap.error("--semantic-dir goes with --keep-classes or --drop-classes")
    if args.semantic_dir is None and args.min_share != 0.0:
        ap.error("--min-share goes with --semantic-dir")
    if not 0.0 <= args.min_share <= 1.0 or not 1 <= args.semantic_classes <= 255:
        ap.error("--min-share must be in [0, 1] and --semantic-classes in 1..255")
    for c in (args.keep_classes or []) + (args.drop_classes or []):
        if not 0 <= c < args.semantic_classes:
            ap.error(f"class {c} is outside [0, {args.semantic_classes})")
    if args.orient_cameras and args.dataset_dir is None:
        ap.error("--orient-cameras needs --dataset-dir")
    if (args.mesher == "tsdf" or args.semantic_dir is not None or args.orient_cameras) != (args.dataset_dir is not None):
        ap.error("--dataset-dir goes with --mesher tsdf or --semantic-dir")
    if args.scale is not None and not (args.scale > 0 and args.scale < float("inf")):
        ap.error("--scale must be positive and finite")
    if args.rotate is not None and not sum(v * v for v in args.rotate) > 0:
        ap.error("--rotate needs a quaternion that is not zero")
    if args.crop_box is not None and not all(h > 0 for h in args.crop_box[3:]):
        ap.error("--crop-box needs half extents > 0")
    if args.mesher == "tsdf" and args.colors:
        ap.error("--colors goes with --mesher density")
    return args


def class_list(text):
    """'a,b,...' -> [a, b, ...], distinct."""
    try:
        ids = [int(t) for t in text.split(",")]
    except ValueError:
        raise argparse.ArgumentTypeError(f"{text!r}: a comma-separated list of class numbers expected")
    if len(set(ids)) != len(ids):
        raise argparse.ArgumentTypeError(f"{text!r}: a class is named twice")
    return ids


def float_list(count):
    """'a,b,...' -> [a, b, ...], exactly ``count`` finite numbers."""
    def parse_list(text):
        try:
            values = [float(t) for t in text.split(",")]
        except ValueError:
            raise argparse.ArgumentTypeError(f"{text!r}: {count} comma-separated numbers expected")
        if len(values) != count or not all(v == v and abs(v) != float("inf") for v in values):
            raise argparse.ArgumentTypeError(f"{text!r}: {count} comma-separated finite numbers expected")
        return values
    return parse_list


def scene_transform(args, cameras=None):
    """The similarity of --orient-cameras (first) and --rotate / --translate / --scale (after it), or None."""
    from tinysplat_amd.edit import Sim3, orient_from_cameras
    manual = args.rotate is not None or args.translate is not None or args.scale is not None
    if not manual and not args.orient_cameras:
        return None
    t = Sim3.identity()
    if args.orient_cameras:
        t = orient_from_cameras(cameras)
    if manual:
        t = Sim3.from_quat(args.rotate or (1.0, 0.0, 0.0, 0.0), args.translate or (0.0, 0.0, 0.0),
                           1.0 if args.scale is None else args.scale) @ t
    return t


def cut_by_class(model, cameras, args):
    """The Gaussians of --keep-classes, or all but those of --drop-classes, by the lifted labels."""
    import torch
    from tinysplat_amd.semantic import SemanticMaps, lift_labels, select_gaussians
    named = args.keep_classes if args.keep_classes is not None else args.drop_classes
    # every class votes (a Gaussian belongs to a named class only if that class beats all the others): column = label
    maps = SemanticMaps(cameras, args.semantic_dir, num_classes=args.semantic_classes, device=args.device)
    lifted = lift_labels(model, None, maps, min_share=args.min_share)
    of_named = torch.isin(lifted.labels, torch.tensor(named, dtype=torch.uint8, device=lifted.labels.device))
    mask = of_named if args.keep_classes is not None else ~of_named
    print(f"{int(of_named.sum())} of {model.num_points} Gaussians carry one of the classes {named}; keeping {int(mask.sum())}")
    return select_gaussians(model, mask)


def dataset_cameras(dataset_dir, colmap_path):
    """One camera per image of the reconstruction, in the order of images.bin; no image is read."""
    from tinysplat_amd.colmap import read_reconstruction
    from tinysplat_amd.dataset import camera_from_colmap
    rec = read_reconstruction(Path(dataset_dir) / colmap_path)
    cameras = []
    for image in rec.images.values():
        cam = rec.cameras[image.camera_id]
        cameras.append(camera_from_colmap(cam, image, (cam.width, cam.height)).camera)
    return cameras


def load_model(path, device):
    from tinysplat_amd import formats
    ext = Path(path).suffix.lower()
    if ext == ".ply":
        return formats.load_ply(path, device)
    if ext in (".pth", ".pt"):
        return formats.load_checkpoint(path, device)
    raise SystemExit(f"{path}: a checkpoint (.pth, .pt) or a 3DGS PLY (.ply) expected")


def main(argv=None):
    args = parse(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: tinysplat_amd has no CPU path")
    from tinysplat_amd import MeshConfig, extract_mesh, formats
    model = load_model(args.input_file, args.device)
    if args.antialiased:
        model.rasterize_mode = "antialiased"
    cameras = dataset_cameras(args.dataset_dir, args.colmap_path) if args.dataset_dir is not None else None
    if args.semantic_dir is not None:
        model = cut_by_class(model, cameras, args)
    transform = scene_transform(args, cameras)
    if transform is not None:
        from tinysplat_amd.edit import transform_cameras, transform_gaussians
        model = transform_gaussians(model, transform)
        cameras = transform_cameras(cameras, transform) if cameras is not None else None
        print("scene transform:\n" + "\n".join(" ".join(f"{v: .9g}" for v in row) for row in transform.matrix()))
    if args.crop_box is not None:
        from tinysplat_amd.edit import crop_gaussians
        before = model.num_points
        model = crop_gaussians(model, args.crop_box[:3], args.crop_box[3:])
        print(f"--crop-box keeps {model.num_points} of {before} Gaussians")
    if args.filetype == "PLY":
        formats.export_ply(model, args.output_file)
    elif args.filetype == "SPLAT":
        formats.export_splat(model, args.output_file, limit=args.limit)
    else:
        res = {} if args.resolution is None else {"resolution": args.resolution}
        if args.mesher == "tsdf":
            from tinysplat_amd import FusionConfig, extract_mesh_tsdf
            mesh = extract_mesh_tsdf(model, cameras, FusionConfig(target_faces=args.target_faces, **res), args.device)
        else:
            mesh = extract_mesh(model, MeshConfig(colors=args.colors, target_faces=args.target_faces, **res))
        write = formats.export_mesh_obj if args.filetype == "OBJ" else formats.export_mesh_ply
        write(mesh, args.output_file)
        print(f"{int(mesh.vertices.shape[0])} vertices, {int(mesh.faces.shape[0])} faces")
    print(f"wrote {args.output_file}: {Path(args.output_file).stat().st_size} bytes from {model.num_points} Gaussians")


if __name__ == "__main__":
    main()
