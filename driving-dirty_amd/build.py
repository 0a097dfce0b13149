"""Build the C-ABI shared library (``csrc/libdd_hotpath.so``) and its extension libraries (``csrc/libdd_augment.so``, ``csrc/libdd_tta.so``, ``csrc/libdd_ema.so``, ``csrc/libdd_rm_loss.so``) with hipcc for gfx950.

    python -m driving_dirty_amd.build          # or __graft_entry__.build()

hipcc cross-compiles without a GPU.  The library is built IN-TREE so that it travels with the
repository snapshot to the GPU box (a JIT cache under ~/.cache would not).  Each source is compiled
to its own object (in parallel, re-done only when the source or a header is newer) and the objects
are linked into the one library.  The extension libraries (``include/dd_augment.h``: the train-time augmentation; ``include/dd_tta.h``:
mirror test-time averaging; ``include/dd_ema.h``: the moving average of the parameters; ``include/dd_rm_loss.h``: the road-map loss on logits) are built the same way, with the same flags, each from its own sources, and link against the main library,
whose ``dd_fail`` / ``dd_last_error`` they use.
"""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc")
LIB = os.path.join(CSRC, "libdd_hotpath.so")
OBJ = os.path.join(CSRC, "build")
SOURCES = ["runtime.hip", "conv3x3.hip", "layout_pool.hip", "dense.hip", "linear.hip", "gconv.hip", "dconv.hip", "dconv_t.hip", "dconv_m.hip", "dconv_split.hip", "conv1ch.hip", "ssconv.hip", "bn2d.hip", "raster.hip",
           "conv3x3_bf16.hip", "decoder_bf16.hip", "mlp_tail.hip", "adam_rankb.hip", "strip6.hip", "boxeval.hip", "tshist.hip", "gradnorm.hip", "box_loss.hip"]
FLAGS = ["-O3", "--offload-arch=gfx950", "-std=c++17", "-fPIC", "-Wall", "-Wno-unused-function"]
# per-file additions.  adam_rankb.hip: MFMA accumulators in ordinary vector registers (the kernel's whole budget is 72 registers, and the
# default form keeps a second copy of the accumulators in the accumulation registers)
EXTRA_FLAGS = {"adam_rankb.hip": ["-mllvm", "-amdgpu-mfma-vgpr-form"]}
HEADER = os.path.join(os.path.dirname(os.path.dirname(CSRC)), "include", "dd_hotpath.h")      # the C ABI; _lib.py derives its ctypes table from it
HEADERS = [os.path.join(CSRC, "dd_common.h"), os.path.join(CSRC, "dd_device.h"), os.path.join(CSRC, "dd_adam.h"), os.path.join(CSRC, "adam_rankb_kernels.inc"), HEADER]
# the extension library: launch functions that are not part of include/dd_hotpath.h (its set of functions is pinned); augment.py binds it
AUG_LIB = os.path.join(CSRC, "libdd_augment.so")
AUG_SOURCES = ["augment.hip"]
AUG_HEADER = os.path.join(os.path.dirname(HEADER), "dd_augment.h")
AUG_HEADERS = [os.path.join(CSRC, "dd_common.h"), os.path.join(CSRC, "dd_device.h"), HEADER, AUG_HEADER]
# ... and the second one: mirror test-time averaging (the sets of functions of both headers above are pinned); tta.py binds it
TTA_LIB = os.path.join(CSRC, "libdd_tta.so")
TTA_SOURCES = ["tta.hip"]
TTA_HEADER = os.path.join(os.path.dirname(HEADER), "dd_tta.h")
TTA_HEADERS = [os.path.join(CSRC, "dd_common.h"), os.path.join(CSRC, "dd_device.h"), HEADER, TTA_HEADER]
# ... and the third: the exponential moving average of the parameters and the exchange with it (the three headers above are pinned); ema.py binds it
EMA_LIB = os.path.join(CSRC, "libdd_ema.so")
EMA_SOURCES = ["ema.hip"]
EMA_HEADER = os.path.join(os.path.dirname(HEADER), "dd_ema.h")
EMA_HEADERS = [os.path.join(CSRC, "dd_common.h"), os.path.join(CSRC, "dd_device.h"), HEADER, EMA_HEADER]
# ... and the fourth: weighted BCE-with-logits + soft threat score on the road-map head's logits (the four headers above are pinned); rm_loss.py binds it
RM_LOSS_LIB = os.path.join(CSRC, "libdd_rm_loss.so")
RM_LOSS_SOURCES = ["rm_loss.hip"]
RM_LOSS_HEADER = os.path.join(os.path.dirname(HEADER), "dd_rm_loss.h")
RM_LOSS_HEADERS = [os.path.join(CSRC, "dd_common.h"), os.path.join(CSRC, "dd_device.h"), HEADER, RM_LOSS_HEADER]


def _obj(src):
    return os.path.join(OBJ, os.path.splitext(src)[0] + ".o")


def _stale(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def _main_needs_build():
    return _stale(LIB, [os.path.join(CSRC, s) for s in SOURCES] + HEADERS)


def _augment_needs_build():
    return _stale(AUG_LIB, [os.path.join(CSRC, s) for s in AUG_SOURCES] + AUG_HEADERS)


def _tta_needs_build():
    return _stale(TTA_LIB, [os.path.join(CSRC, s) for s in TTA_SOURCES] + TTA_HEADERS)


def _ema_needs_build():
    return _stale(EMA_LIB, [os.path.join(CSRC, s) for s in EMA_SOURCES] + EMA_HEADERS)


def _rm_loss_needs_build():
    return _stale(RM_LOSS_LIB, [os.path.join(CSRC, s) for s in RM_LOSS_SOURCES] + RM_LOSS_HEADERS)


def needs_build():
    return _main_needs_build() or _augment_needs_build() or _tta_needs_build() or _ema_needs_build() or _rm_loss_needs_build()


def build_diag(verbose=True):
    """``csrc/libdd_hotpath_diag.so``: the same library compiled with -DDD_TIMING_DIAG (timing ablations of single kernels whose
    results are then WRONG: DD_DCONV_REPEAT, DD_SPLIT_ABL).  Never loaded unless DD_HOTPATH_LIB points at it; not built by build()."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    out = os.path.join(CSRC, "build_diag")
    os.makedirs(out, exist_ok=True)

    def one(src):
        obj = os.path.join(out, os.path.splitext(src)[0] + ".o")
        if _stale(obj, [os.path.join(CSRC, src)] + HEADERS):
            cmd = [hipcc] + FLAGS + EXTRA_FLAGS.get(src, []) + ["-DDD_TIMING_DIAG", "-c", os.path.join(CSRC, src), "-o", obj]
            if verbose:
                print(" ".join(cmd), flush=True)
            subprocess.check_call(cmd)
        return obj
    with ThreadPoolExecutor(max_workers=8) as pool:
        objs = list(pool.map(one, SOURCES))
    lib = os.path.join(CSRC, "libdd_hotpath_diag.so")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", lib] + objs)
    return lib


def _run(cmd, verbose):
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.check_call(cmd)


def _build_extension(lib, sources, headers, force, verbose):
    """An extension library from its own sources: the main library's flags; linked against ``libdd_hotpath.so`` (found beside it at load
    time, $ORIGIN), which therefore has to exist."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    os.makedirs(OBJ, exist_ok=True)
    for src in sources:
        if force or _stale(_obj(src), [os.path.join(CSRC, src)] + headers):
            _run([hipcc] + FLAGS + ["-c", os.path.join(CSRC, src), "-o", _obj(src)], verbose)
    _run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", lib] + [_obj(s) for s in sources]
         + ["-L" + CSRC, "-l:" + os.path.basename(LIB), "-Wl,-rpath,$ORIGIN"], verbose)
    return lib


def build_augment(force=False, verbose=True):
    """``csrc/libdd_augment.so`` from AUG_SOURCES, when it is stale."""
    if not force and not _augment_needs_build():
        return AUG_LIB
    return _build_extension(AUG_LIB, AUG_SOURCES, AUG_HEADERS, force, verbose)


def build_tta(force=False, verbose=True):
    """``csrc/libdd_tta.so`` from TTA_SOURCES, when it is stale."""
    if not force and not _tta_needs_build():
        return TTA_LIB
    return _build_extension(TTA_LIB, TTA_SOURCES, TTA_HEADERS, force, verbose)


def build_ema(force=False, verbose=True):
    """``csrc/libdd_ema.so`` from EMA_SOURCES, when it is stale."""
    if not force and not _ema_needs_build():
        return EMA_LIB
    return _build_extension(EMA_LIB, EMA_SOURCES, EMA_HEADERS, force, verbose)


def build_rm_loss(force=False, verbose=True):
    """``csrc/libdd_rm_loss.so`` from RM_LOSS_SOURCES, when it is stale."""
    if not force and not _rm_loss_needs_build():
        return RM_LOSS_LIB
    return _build_extension(RM_LOSS_LIB, RM_LOSS_SOURCES, RM_LOSS_HEADERS, force, verbose)


def build(force=False, verbose=True):
    """The five libraries, each only when it is stale; returns the main library's path."""
    if force or _main_needs_build():
        _build_main(force, verbose)
    build_augment(force, verbose)
    build_tta(force, verbose)
    build_ema(force, verbose)
    build_rm_loss(force, verbose)
    return LIB


def _build_main(force, verbose):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    os.makedirs(OBJ, exist_ok=True)
    todo = [s for s in SOURCES if force or _stale(_obj(s), [os.path.join(CSRC, s)] + HEADERS)]

    def compile_one(src):
        cmd = [hipcc] + FLAGS + EXTRA_FLAGS.get(src, []) + ["-c", os.path.join(CSRC, src), "-o", _obj(src)]
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd)

    with ThreadPoolExecutor(max_workers=min(8, max(1, len(todo)))) as pool:
        list(pool.map(compile_one, todo))
    cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB] + [_obj(s) for s in SOURCES]
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.check_call(cmd)
    return LIB


if __name__ == "__main__":
    if "--diag" in sys.argv:
        print(build_diag())
    else:
        build(force="--force" in sys.argv)
