#!/usr/bin/env python
"""Serves a saved scene to a websocket viewer.

    python tools/view.py scene.ply --dataset-dir datasets/train
    python tools/view.py scene.splat --width 1920 --height 1080 --fov-x 60

The scene is a 3DGS PLY (``.ply``), a checkpoint (``.pth`` / ``.pt``) or a ``.splat`` file.  The camera every client starts
from is the first image's camera in ``--dataset-dir``'s COLMAP reconstruction (at the size cameras.bin records), or a pinhole camera of ``--width`` x ``--height``
pixels and ``--fov-x`` degrees at the origin.  The server speaks the reference's protocol (``tinysplat_amd.Viewer``): JSON
text frames, ``renderRequest`` answered with a base64 JPEG that the GPU encodes.  The browser client is not part of this
project.  Needs a GPU: there is no CPU path.
"""
import argparse
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

READERS = {".ply": "load_ply", ".pth": "load_checkpoint", ".pt": "load_checkpoint", ".splat": "load_splat"}


def parse(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("scene", type=str, help="scene.ply, scene.pth or scene.splat")
    ap.add_argument("--device", type=str, default="cuda:0")
    ap.add_argument("--dataset-dir", type=str, default=None, help="take the template camera from this reconstruction")
    ap.add_argument("--colmap-path", type=str, default="colmap/sparse/0", help="below --dataset-dir")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--fov-x", type=float, default=60.0, help="degrees")
    ap.add_argument("--quality", type=int, default=90)
    ap.add_argument("--subsampling", choices=("420", "444"), default="420")
    ap.add_argument("--viewer-ip", type=str, default="127.0.0.1")
    ap.add_argument("--viewer-port", type=int, default=8765)
    ap.add_argument("--antialiased", action="store_true",
                    help="render in the antialiased mode (opacity compensation for the 2D low-pass), whatever the file says")
    args = ap.parse_args(argv)
    if Path(args.scene).suffix.lower() not in READERS:
        ap.error(f"the scene must end in one of {', '.join(READERS)}")
    if not 1 <= args.quality <= 100 or args.width < 1 or args.height < 1 or not 0 < args.fov_x < 180:
        ap.error("--quality is 1..100, --width and --height at least 1, --fov-x between 0 and 180")
    return args


def main(argv=None):
    args = parse(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: tinysplat_amd has no CPU path")
    from tinysplat_amd import Viewer, formats
    from tinysplat_amd.viewer import ViewRenderer
    model = getattr(formats, READERS[Path(args.scene).suffix.lower()])(args.scene, args.device)
    if args.antialiased:                 # overrides what the file says (a .pth or .splat says nothing)
        model.rasterize_mode = "antialiased"
    if args.dataset_dir is not None:
        from tinysplat_amd.colmap import read_reconstruction
        from tinysplat_amd.dataset import camera_from_colmap
        rec = read_reconstruction(Path(args.dataset_dir) / args.colmap_path)
        image = next(iter(rec.images.values()))
        cam = rec.cameras[image.camera_id]
        camera = camera_from_colmap(cam, image, (cam.width, cam.height)).camera
    else:
        from tinysplat_amd.synthetic import PinholeCamera
        camera = PinholeCamera.look_at_origin_plus_z(args.width, args.height, args.fov_x, position=(0.0, 0.0, 0.0))
    viewer = Viewer(ViewRenderer(model, camera, args.device), args.viewer_ip, args.viewer_port, args.quality,
                    args.subsampling)
    print(f"{model.num_points} Gaussians at {camera.width} x {camera.height} on ws://{args.viewer_ip}:{viewer.port}")
    try:
        viewer.run_forever()
    finally:
        viewer.stop()
        print(f"{viewer.rendered} requests rendered")


if __name__ == "__main__":
    main()
