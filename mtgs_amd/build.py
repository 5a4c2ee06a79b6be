"""Builds mtgs_amd/libmtgs_rast.so (gfx950) from mtgs_amd/csrc/*.hip with hipcc, in-tree.

hipcc cross-compiles without a GPU, so this runs in the build container; the resulting .so is
git-ignored but travels with the tree to the GPU box.
"""
from __future__ import annotations

import os
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

PKG = Path(__file__).resolve().parent
CSRC = PKG / "csrc"
OBJ = CSRC / "_obj"
LIB = PKG / "libmtgs_rast.so"
ARCH = "gfx950"

# -fno-slp-vectorize: on gfx950 v_pk_{fma,mul,add}_f32 issue in two passes (no throughput gain for
# fp32) but the SLP vectoriser pays v_mov shuffles to pair their operands -- measured -19 % time on
# the compositing backward without it.
COMMON_FLAGS = [
    f"--offload-arch={ARCH}", "-O3", "-std=c++17", "-fPIC", "-munsafe-fp-atomics", "-fno-slp-vectorize",
    "-Wall", "-Wno-unused-function", f"-I{PKG.parent / 'include'}",
]
# The projection forward must round after every operation (bit-exact tile binning inputs); the metrics and the
# geometric and depth losses round as the reference's per-operation PyTorch kernels do, and so do the neighbour distances, the seeding
# and the point-cloud filters (whose fp64 sums and voxel indices are compared bit for bit with a NumPy transcription); the crop box
# decides a row by three fp32 dot products that the host evaluates operation by operation in torch and NumPy;
# the colormaps of a presented frame are nerfstudio's chain of element-wise fp32 kernels, one rounding per operation.
# lpips.hip (the LPIPS metric) takes the common flags: its convolutions are fma chains on the MFMA unit whatever the flag, and its
# tail is compared with an fp64 restatement within a derived bound, not bit for bit.  dino.hip (the DINOv2 similarity) likewise: its
# preprocessing is integer arithmetic and single correctly rounded fp32 operations that no contraction can join.
# jpeg.hip (the JPEG encoder) is integer arithmetic; its one fp32 conversion uses __fmul_rn / __fadd_rn, which never fuse.
# lidar.hip (the lidar depth image, the cloud's colours and labels) is fp64 whose products and sums round separately: its discrete
# outputs (pixels, field of view, labels) are compared bit for bit with a NumPy restatement.
# frame.hip (Pillow's resize of a training frame) adds (double)float * double products in double, tap by tap, as Pillow's C does: a
# fused multiply-add would skip the product's rounding and change bits of the float32 depth.
# stack.hip (lidar sweeps split by the boxes and stacked) is fp64 like lidar.hip: the owner of a point is decided by <= on sums of
# products, and its box-frame and global coordinates are compared bit for bit with a NumPy restatement.
# icp.hip (lidar registration) is fp64 in a stated order: voxel indices, the map's accept / refuse rule, the nearest neighbour and the
# 27 sums of an iteration are compared bit for bit with a NumPy restatement.
# undistort.hip (the lens undistortion of a frame) evaluates its map in fp64, one rounding per operation, before the rounding to
# float32 and to five fractional bits: the map and every sampled byte are compared bit for bit with a NumPy restatement.
# brightness.hip (the V factors and the HSV adjust) converts HSV to RGB in fp32 with one rounding per operation -- a fused
# vf * (1 - sf * f) would change bytes -- and shares lidar.hip's fp64 sample, whose truncated V is compared bit for bit with the reference.
# redistort.hip (a rendered frame bent back into the raw camera) iterates the inverse lens model in fp64, one rounding per operation:
# its map and every sampled byte are compared bit for bit with a NumPy restatement, as undistort.hip's are.
# png.hip (the indexed PNG codec) is integer arithmetic; the two depth rules fused into it are single fp32 operations written with
# __fmul_rn / __fadd_rn / __fdiv_rn, and the flag keeps anything added beside them from fusing: the bytes are compared with NumPy.
PER_FILE_FLAGS = {"png.hip": ["-ffp-contract=off"], "project.hip": ["-ffp-contract=off"], "front.hip": ["-ffp-contract=off"], "metrics.hip": ["-ffp-contract=off"],
                  "geomloss.hip": ["-ffp-contract=off"], "depthloss.hip": ["-ffp-contract=off"], "seed.hip": ["-ffp-contract=off"], "cloud.hip": ["-ffp-contract=off"],
                  "crop.hip": ["-ffp-contract=off"], "present.hip": ["-ffp-contract=off"], "lidar.hip": ["-ffp-contract=off"],
                  "frame.hip": ["-ffp-contract=off"], "stack.hip": ["-ffp-contract=off"], "icp.hip": ["-ffp-contract=off"],
                  "undistort.hip": ["-ffp-contract=off"], "brightness.hip": ["-ffp-contract=off"], "redistort.hip": ["-ffp-contract=off"]}


class HipccNotFound(RuntimeError):
    """No hipcc on this machine (a GPU box running the prebuilt in-tree .so): the only build error callers may ignore."""


def _hipcc() -> str:
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and Path(cand).exists():
            return cand
    raise HipccNotFound("hipcc not found (set HIPCC or add /opt/rocm/bin to PATH)")


def sources():
    return sorted(CSRC.glob("*.hip"))


def _stale(out: Path, deps) -> bool:
    if not out.exists():
        return True
    t = out.stat().st_mtime
    return any(Path(d).stat().st_mtime > t for d in deps)


def stale_sources():
    """csrc files (and headers) newer than the built library -- empty when the .so is up to date."""
    if not LIB.exists():
        return sources()
    t = LIB.stat().st_mtime
    deps = sources() + list(CSRC.glob("*.hpp")) + sorted((PKG.parent / "include").glob("*.h"))
    return [d for d in deps if d.stat().st_mtime > t]


def build(force: bool = False, verbose: bool = False) -> Path:
    hipcc = _hipcc()
    OBJ.mkdir(exist_ok=True)
    live = {s.stem for s in sources()}
    for stale in OBJ.glob("*.o"):          # objects of sources that no longer exist (bin2.o after round 2)
        if stale.stem not in live:
            stale.unlink()
    headers = list(CSRC.glob("*.hpp")) + sorted((PKG.parent / "include").glob("*.h")) + [Path(__file__)]
    jobs = []
    for src in sources():
        obj = OBJ / (src.stem + ".o")
        if force or _stale(obj, [src] + headers):
            cmd = [hipcc, "-c", str(src), "-o", str(obj)] + COMMON_FLAGS + PER_FILE_FLAGS.get(src.name, [])
            jobs.append(cmd)

    def run(cmd):
        if verbose:
            print(" ".join(cmd), file=sys.stderr)
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"hipcc failed: {' '.join(cmd)}\n{r.stdout}\n{r.stderr}")
        return r.stderr

    if jobs:
        # at most 16 compilers at once: a shared machine reports every CPU it has, not the few a process may use
        with ThreadPoolExecutor(max_workers=min(len(jobs), os.cpu_count() or 4, 16)) as ex:
            for warn in ex.map(run, jobs):
                if verbose and warn:
                    print(warn, file=sys.stderr)
    objs = [OBJ / (s.stem + ".o") for s in sources()]
    if force or jobs or _stale(LIB, objs):
        run([hipcc, "-shared", "-fPIC", f"--offload-arch={ARCH}", "-o", str(LIB)] + [str(o) for o in objs])
    return LIB


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
