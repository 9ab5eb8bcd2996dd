"""Builds libtinysplat_hip.so (gfx950) in-tree with hipcc.  Used by __graft_entry__.build()."""
from __future__ import annotations

import os
import shutil
import subprocess
from pathlib import Path

CSRC = Path(__file__).resolve().parent / "csrc"
LIB_PATH = CSRC / "libtinysplat_hip.so"

# (source, extra flags).  project.hip must not contract a*b+c into fma: its float32 results are
# checked bit-for-bit against the oracle (radii / num_tiles_hit drive bit-exact binning checks).
SOURCES = [
    ("project.hip", ["-ffp-contract=off"]),
    ("binning.hip", ["-ffp-contract=off"]),
    # raster.hip: the SLP vectoriser pairs unrelated scalar accumulators into v_pk_* ops and pays for
    # it with register shuffles (v_mov) that cost more VALU issue slots than the packing saves
    # (measured: raster_bwd 0.87 -> 0.67 ms with it off)
    ("raster.hip", ["-fno-slp-vectorize"]),
    ("train.hip", []),
    ("densify.hip", ["-ffp-contract=off"]),
    ("formats.hip", []),
    ("frame.hip", []),
    ("shard.hip", ["-ffp-contract=off"]),
    # knn.hip: neighbour distances are compared bit-for-bit with a float64 oracle (sqrt of dx*dx + dy*dy + dz*dz)
    ("knn.hip", ["-ffp-contract=off"]),
    # surface.hip: every multiply and add of the entropy and its gradient is rounded on its own, as torch rounds the
    # expression's separate operations (the gradient's factors come in another order than autograd's: a few ulps)
    ("surface.hip", ["-ffp-contract=off"]),
    # density.hip: the density term and its gradient are compared with a float32 restatement of the reference
    ("density.hip", ["-ffp-contract=off"]),
    # extract.hip: sample positions, densities and crossings are compared with a float64 restatement of the reference
    ("extract.hip", ["-ffp-contract=off"]),
    # mesh.hip: corner positions and interpolated vertices must come out bit-identical in every cell sharing an edge,
    # and equal to the host build of mesh_cells.h; densities are compared with the same float64 restatement
    ("mesh.hip", ["-ffp-contract=off"]),
    # field_color.hip: the neighbours' weights are density_field.h's term, whose bits extract.hip and mesh.hip pin, and the
    # colours are compared with a float64 restatement whose float32 run rounds every product and sum on its own
    ("field_color.hip", ["-ffp-contract=off"]),
    # simplify.hip: a vertex's cell comes from a float32 difference and quotient that the host build of simplify_math.h
    # and the oracle round separately, and the double sums and solves are compared with a float64 restatement
    ("simplify.hip", ["-ffp-contract=off"]),
    # clean.hip: a face's weight ranks the faces at an edge and must be numpy's double, product by product
    ("clean.hip", ["-ffp-contract=off"]),
    # splatfile.hip: a record's bytes are truncations of float32 (and, for the rotation, double) expressions that the host
    # build of splat_record.h and the float64 oracle round operation by operation; an fma would move values across integers
    ("splatfile.hip", ["-ffp-contract=off"]),
    # undistort.hip: source coordinates and bilinear sums are compared with a float64 restatement whose float32 run, like
    # the host build of undistort_math.h, rounds every product and sum on its own
    ("undistort.hip", ["-ffp-contract=off"]),
    # jpeg.hip: a quantised coefficient is rint of a float32 quotient of sums of eight products; the host build of
    # jpeg_math.h must round every product and sum as the kernel does, or a coefficient near a half differs and with it
    # the file
    ("jpeg.hip", ["-ffp-contract=off"]),
    # metrics.hip: a uint8 target and the float target of the same values go through two instantiations of one kernel
    # and must give the same 32 bytes; with no contraction left to the compiler (the filters' fmas are written out) the
    # two cannot round a sum differently
    ("metrics.hip", ["-ffp-contract=off"]),
    # depth_prior.hip: a point's pixel is rint of a float32 expression that the host build of depth_prior_math.h and the
    # oracle round operation by operation, and a target is one float32 rounding of a double product and sum; the fit's
    # residuals are written as fmas on purpose
    ("depth_prior.hip", ["-ffp-contract=off"]),
    # tsdf.hip: a corner's pixel is rint of a float32 expression and its observation a float32 difference and quotient
    # that the host build of tsdf_math.h rounds operation by operation; an fma would move a corner across a pixel border
    # in one brick and not in its neighbour's host restatement, and the corner positions are mesh.hip's, bit for bit
    ("tsdf.hip", ["-ffp-contract=off"]),
    # votes.hip: its staging culls are raster.hip's and are compiled as raster.hip compiles them (no file-wide contraction
    # switch); the per-pixel body that must give the forward's bits turns contraction off itself, as fwd_chunk does
    ("votes.hip", []),
    # mcmc.hip: the noise's Sigma z and the normals' Box-Muller are compared with the host build of mcmc_math.h, which
    # rounds every product and sum on its own, and the double series of the relocation is compared with a float64
    # restatement term by term; an fma in either would make the device and the host build two different functions
    ("mcmc.hip", ["-ffp-contract=off"]),
    # appearance.hip: the forward and the image gradient must be the bits of the host build of appearance_math.h, which
    # rounds every product and sum of the nested lerps on its own (an fma would also break "a constant grid returns its
    # constant"), and the double sums of the total variation and the fit are compared with the host build bit for bit
    ("appearance.hip", ["-ffp-contract=off"]),
    # transform.hip: a transformed mean, quaternion and SH coefficient are defined as the bits of the host build of
    # transform_math.h, sums of separately rounded products in a fixed order; an fma would also keep an identity transform
    # from returning its input
    ("transform.hip", ["-ffp-contract=off"]),
    # pose.hip: a row's six terms and the sums over the rows are defined as the bits of the host build of pose_math.h,
    # double products and sums each rounded on its own in a fixed order; an fma would make the two builds two functions
    ("pose.hip", ["-ffp-contract=off"]),
    # antialias.hip: comp, the compensated opacity and the gradient rows are defined as the bits of the host build of
    # antialias_math.h, float32 products and sums each rounded on its own; its exponential is written out in that header
    ("antialias.hip", ["-ffp-contract=off"]),
]
COMMON = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wall", "-Wno-unused-function"]


def _hipcc() -> str:
    exe = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(exe):
        raise RuntimeError("hipcc not found; the HIP library cannot be built")
    return exe


def _stale(target: Path, deps) -> bool:
    if not target.exists():
        return True
    t = target.stat().st_mtime
    return any(Path(d).stat().st_mtime > t for d in deps)


def _stamp_path(obj: Path) -> Path:
    return obj.with_suffix(obj.suffix + ".flags")


def _flags_match(obj: Path, cmd) -> bool:
    """An object is only as good as the command line that produced it: ablation builds
    (TS_EXTRA_HIPCC_FLAGS, e.g. -DTS_ABLATE=3 which makes results WRONG) leave objects that are newer
    than the sources, so the exact flag list is recorded next to each object and compared."""
    sp = _stamp_path(obj)
    return sp.exists() and sp.read_text() == " ".join(cmd[1:])


def build_variant(out_dir, flags, jobs: int = 8) -> Path:
    """A second build of the library with extra -D flags into ``out_dir`` (objects and .so; the in-tree build is not
    touched), sources compiled in parallel -> path of the .so.  Load it in a process of its own with TS_LIB_PATH=<path>
    TS_ALLOW_VARIANT_LIB=1 (tests/test_gpu_variants.py: the other settings of SURVEY App. C's switches)."""
    from concurrent.futures import ThreadPoolExecutor
    hipcc = _hipcc()
    out_dir = Path(out_dir)
    out_dir.mkdir(parents=True, exist_ok=True)
    flags = list(flags)

    def one(item):
        src, extra = item
        o = out_dir / (Path(src).stem + ".o")
        subprocess.run([hipcc, *COMMON, *extra, *flags, "-c", str(CSRC / src), "-o", str(o)], check=True)
        return str(o)
    with ThreadPoolExecutor(max_workers=max(1, jobs)) as ex:
        objs = list(ex.map(one, SOURCES))
    rocm = Path(hipcc).resolve().parent.parent
    have_roctx = any((r / "include" / "rocprofiler-sdk-roctx" / "roctx.h").exists() for r in (rocm, Path("/opt/rocm")))
    lib = out_dir / "libtinysplat_hip.so"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", *objs,
                    *(["-lrocprofiler-sdk-roctx"] if have_roctx else []), "-o", str(lib)], check=True)
    _stamp_path(lib).write_text(" ".join([*COMMON, *flags]))
    return lib


def build_library(force: bool = False, verbose: bool = False) -> Path:
    hipcc = _hipcc()
    # developer knob for ablation runs (tools/time_raster.py): extra -D flags, implies a rebuild
    extra_env = os.environ.get("TS_EXTRA_HIPCC_FLAGS", "").split()
    headers = [*sorted(CSRC.glob("*.h")), CSRC.parent.parent / "include" / "tinysplat_hip.h",
               Path(__file__)]          # every header of csrc/ (splat_math.h, pack.h, ...); the flags live in this file
    objs = []
    relink = False
    for src, extra in SOURCES:
        s = CSRC / src
        o = CSRC / (Path(src).stem + ".o")
        cmd = [hipcc, *COMMON, *extra, *extra_env, "-c", str(s), "-o", str(o)]
        if force or _stale(o, [s, *headers]) or not _flags_match(o, cmd):
            if verbose:
                print(" ".join(cmd), flush=True)
            _stamp_path(o).unlink(missing_ok=True)
            subprocess.run(cmd, check=True)
            _stamp_path(o).write_text(" ".join(cmd[1:]))
            relink = True
        objs.append(str(o))
    # roctx ranges (csrc/frame.hip) are optional: link the marker library only where the header it is guarded by exists
    rocm = Path(hipcc).resolve().parent.parent
    have_roctx = any((r / "include" / "rocprofiler-sdk-roctx" / "roctx.h").exists() for r in (rocm, Path("/opt/rocm")))
    cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", *objs,
           *(["-lrocprofiler-sdk-roctx"] if have_roctx else []), "-o", str(LIB_PATH)]
    # the library records the flag sets of all its objects: a variant library is relinked by the
    # next default build even though it is newer than every source
    want = "\n".join(_stamp_path(Path(o)).read_text() for o in objs)
    lib_stamp = _stamp_path(LIB_PATH)
    if force or relink or _stale(LIB_PATH, objs) or not lib_stamp.exists() or lib_stamp.read_text() != want:
        if verbose:
            print(" ".join(cmd), flush=True)
        lib_stamp.unlink(missing_ok=True)
        subprocess.run(cmd, check=True)
        lib_stamp.write_text(want)
    return LIB_PATH


def library_is_default_build() -> bool:
    """True if the library on disk was built without developer -D overrides (tests/test_abi.py)."""
    sp = _stamp_path(LIB_PATH)
    return sp.exists() and "-DTS_" not in sp.read_text()


if __name__ == "__main__":
    print(build_library(verbose=True))
