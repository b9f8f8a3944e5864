"""Build the native libraries of _libraries.LIBRARIES in-tree for gfx950 (hipcc cross-compiles without a GPU).

    python -m pixelsynth_amd.build [--force]

One object per translation unit of csrc/, linked into the library the table names for it: libpixelsynth_hip.so and, beside it,
libpixelsynth_percsim.so, libpixelsynth_consistency.so, libpixelsynth_fid.so, libpixelsynth_scene.so (scene.hip and splat.hip share
the splat's kernels through the header splat_pipeline.h), libpixelsynth_plan.so, libpixelsynth_rank.so, libpixelsynth_rank_groups.so, libpixelsynth_nll.so, libpixelsynth_lmconv_bwd.so, libpixelsynth_splat_bwd.so, libpixelsynth_vq_train.so, libpixelsynth_conv_bwd.so, libpixelsynth_norm_train.so, libpixelsynth_block_train.so, libpixelsynth_content.so, libpixelsynth_thin_train.so, libpixelsynth_gan_train.so, libpixelsynth_disc_conv.so, libpixelsynth_pixelcnn_train.so, libpixelsynth_train_glue.so, libpixelsynth_spectral_train.so, libpixelsynth_unet_train.so and libpixelsynth_vq_conv_train.so.  The HIP units are built with -ffp-contract=off: the splat family
(splat.hip, zbuffer.hip, scene.hip, splat_bwd.hip, which share splat_math.h) because its index paths must be bit-exact against the
oracle, the lmconv*.hip units (lmconv_plan.hip, the planning of the whole-grid pass, with them: it shares their headers) so that the post ops inlined into different kernels (whole-grid vs column step) round identically, the
metric units because their fp32 steps restate the reference's in its order; the matrix products are explicit MFMA intrinsics and are
not affected.  With PS_HIP_LIB set (tuning builds, with PS_OBJ_SUFFIX and PS_EXTRA_HIPCC_FLAGS) only the main library is built, there.
"""
import glob
import os
import subprocess
import sys

from ._libraries import LIBRARIES, MAIN, path

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
ARCH = "gfx950"

COMMON = ["-O3", "-std=c++17", "-fPIC", f"--offload-arch={ARCH}", "-Wall", "-Wno-unused-function"]
EXTRA = os.environ.get("PS_EXTRA_HIPCC_FLAGS", "").split()  # tuning builds, e.g. -DPS_TUNING_BUILD -DPS_CHAIN_TRACE_BUILD
COMMON += EXTRA
if EXTRA:   # ps_build_info() (csrc/host_order.cpp) names them: a number measured through such a library carries its provenance
    COMMON += ['-DPS_BUILD_EXTRA_FLAGS="%s"' % " ".join(EXTRA).replace('"', "'")]


def _deps():
    """What every unit is rebuilt after: the headers of csrc/ and include/"""
    return glob.glob(os.path.join(CSRC, "*.h")) + glob.glob(os.path.join(os.path.dirname(HERE), "include", "*.h"))


def build(force=False, verbose=True):
    """-> the path of libpixelsynth_hip.so; the other libraries of the table are built beside it."""
    for entry in LIBRARIES if not os.environ.get("PS_HIP_LIB") else (MAIN,):
        _build(entry.units, path(entry), force, verbose)
    return path(MAIN)


def _build(units, lib, force, verbose):
    objs, todo = [], []
    dep_m = max(os.path.getmtime(d) for d in _deps())
    for src, flags in units:
        sp = os.path.join(CSRC, src)
        if not os.path.exists(sp):
            continue
        obj = os.path.join(CSRC, os.path.splitext(src)[0] + os.environ.get("PS_OBJ_SUFFIX", "") + ".o")
        if force or not os.path.exists(obj) or os.path.getmtime(obj) < max(os.path.getmtime(sp), dep_m):
            todo.append([HIPCC, "-x", "hip", "-c", sp, "-o", obj] + COMMON + flags)
        objs.append(obj)
    if todo:   # the units are independent: compiled side by side (a full build is the longest unit, not the sum)
        from concurrent.futures import ThreadPoolExecutor

        def run(cmd):
            if verbose:
                print(" ".join(cmd), flush=True)
            subprocess.check_call(cmd)
        with ThreadPoolExecutor(max_workers=min(len(todo), max(1, (os.cpu_count() or 2) // 2))) as pool:
            list(pool.map(run, todo))
    if force or not os.path.exists(lib) or any(os.path.getmtime(o) > os.path.getmtime(lib) for o in objs):
        cmd = [HIPCC, "-shared", "-fPIC", f"--offload-arch={ARCH}", "-o", lib] + objs
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd)
    return lib


if __name__ == "__main__":
    print(build(force="--force" in sys.argv))
