"""Build the C-ABI shared library (``csrc/libdd_hotpath.so``) and the extension libraries of ``EXTENSIONS`` (``csrc/libdd_<name>.so``)
with hipcc for gfx950.

    python -m driving_dirty_amd.build          # or __graft_entry__.build()

hipcc cross-compiles without a GPU.  The libraries are built IN-TREE so that they travel with the repository snapshot to the GPU box
(a JIT cache under ~/.cache would not).  Each source is compiled to its own object (in parallel, re-done only when the source or a
header is newer) and the objects are linked into their library.  An extension library holds launch functions that are not part of
``include/dd_hotpath.h`` (its set of functions is pinned): a header and sources of its own, the main library's flags, linked against
the main library, whose ``dd_fail`` / ``dd_last_error`` it uses.  It is declared ONCE, as an entry of ``EXTENSIONS``, or -- a library of
the optimizer -- of ``OPTIMIZER_EXTENSIONS``, or -- a library of the prediction path -- of ``PREDICTION_EXTENSIONS``, or -- a library of a
training loss that is off by default -- of ``TRAINING_EXTENSIONS``, or -- the bootstrapped road-map loss -- of ``BOOTSTRAP_EXTENSIONS``, or --
the sampled head's uncertainty -- of ``UNCERTAINTY_EXTENSIONS``; the module that binds it holds a ``_lib.Extension`` of that entry.
``extensions()`` is the first two tables as one mapping, ``libraries()`` the first three, ``every_library()`` the first four,
``all_libraries()`` the first five, ``built_libraries()`` all six: what is built, and what every function here that takes an extension's
name looks it up in.
"""
import os
import subprocess
import sys
from collections import namedtuple
from concurrent.futures import ThreadPoolExecutor

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc")
INCLUDE = os.path.join(os.path.dirname(os.path.dirname(CSRC)), "include")
LIB = os.path.join(CSRC, "libdd_hotpath.so")
OBJ = os.path.join(CSRC, "build")
SOURCES = ["runtime.hip", "conv3x3.hip", "camera_gather.hip", "layout_pool.hip", "dense.hip", "linear.hip", "gconv.hip", "dconv.hip", "dconv_t.hip", "dconv_m.hip", "dconv_split.hip", "conv1ch.hip", "ssconv.hip", "bn2d.hip", "raster.hip",
           "conv3x3_bf16.hip", "decoder_bf16.hip", "mlp_tail.hip", "adam.hip", "adam_rankb.hip", "strip6.hip", "boxeval.hip", "tshist.hip", "gradnorm.hip", "box_loss.hip"]
FLAGS = ["-O3", "--offload-arch=gfx950", "-std=c++17", "-fPIC", "-Wall", "-Wno-unused-function"]
# per-file additions.  adam_rankb.hip: MFMA accumulators in ordinary vector registers (the kernel's whole budget is 72 registers, and the
# default form keeps a second copy of the accumulators in the accumulation registers)
EXTRA_FLAGS = {"adam_rankb.hip": ["-mllvm", "-amdgpu-mfma-vgpr-form"]}
HEADER = os.path.join(INCLUDE, "dd_hotpath.h")      # the C ABI; _lib.py derives its ctypes table from it
_COMMON = [os.path.join(CSRC, "dd_common.h"), os.path.join(CSRC, "dd_device.h")]
_LOSS_STATS = os.path.join(CSRC, "dd_loss_stats.h")      # the device code box_loss.hip, rm_loss.hip, consistency.hip and topk_loss.hip share
HEADERS = _COMMON + [os.path.join(CSRC, "dd_adam.h"), os.path.join(CSRC, "dd_conv_strip.h"), os.path.join(CSRC, "conv_wino.inc"), os.path.join(CSRC, "conv_wino2.inc"), os.path.join(CSRC, "adam_rankb_kernels.inc"), _LOSS_STATS, HEADER]

# An extension library.  ``lib``: the .so; ``sources``: under csrc/; ``header``: its public header, from which the binder derives its
# ctypes table; ``headers``: what its objects depend on; ``what``: the noun of the binder's missing-library message.
Extension = namedtuple("Extension", "name lib sources header headers what")


def _extension(name, sources, what, internal=()):
    header = os.path.join(INCLUDE, f"dd_{name}.h")
    return Extension(name, os.path.join(CSRC, f"libdd_{name}.so"), sources, header, _COMMON + list(internal) + [HEADER, header], what)


# To add an extension: a header, a source, one entry in one of the six tables below, a module that holds a ``_lib.Extension`` of the entry.
EXTENSIONS = {e.name: e for e in (
    _extension("augment", ["augment.hip"], "the augmentation"),                      # augment.py: the train-time augmentation
    _extension("tta", ["tta.hip"], "mirror test-time averaging"),                    # tta.py
    _extension("ema", ["ema.hip"], "the weight average"),                            # ema.py: the moving average of the parameters
    _extension("rm_loss", ["rm_loss.hip"], "the road-map loss", [_LOSS_STATS]),      # rm_loss.py: weighted BCE + soft threat score on logits
)}
# The optimizer's extension libraries: the same kind of entry, the same rules, a table of their own.
OPTIMIZER_EXTENSIONS = {e.name: e for e in (
    _extension("adamw", ["adamw.hip"], "decoupled weight decay", [os.path.join(CSRC, "dd_adam.h")]),      # adamw.py: AdamW passes, the rank-B pre-scale
)}


# The prediction path's extension libraries: the same kind of entry, the same rules, a table of their own.
PREDICTION_EXTENSIONS = {e.name: e for e in (
    _extension("head_mean", ["head_mean.hip"], "the sampled road-map head"),      # mc.py: the head's mean over S dropout draws
)}


# The libraries of the training losses that are off by default: the same kind of entry, the same rules, a table of their own.
TRAINING_EXTENSIONS = {e.name: e for e in (
    _extension("consistency", ["consistency.hip"], "the consistency loss", [_LOSS_STATS]),      # consistency.py: the mirror consistency loss on pairs of logit maps
)}


# The library of the bootstrapped road-map loss, off by default: the same kind of entry, the same rules, a table of its own.
BOOTSTRAP_EXTENSIONS = {e.name: e for e in (
    _extension("topk_loss", ["topk_loss.hip"], "the bootstrapped road-map loss", [_LOSS_STATS]),      # topk_loss.py: BCE over each sample's K hardest pixels
)}


# The library of the sampled head's uncertainty, off by default: the same kind of entry, the same rules, a table of its own.
UNCERTAINTY_EXTENSIONS = {e.name: e for e in (
    _extension("head_uncert", ["head_uncert.hip"], "the sampled head's uncertainty"),      # uncertainty.py: entropy, mutual information and variance of the S draws
)}


def extensions():
    """``EXTENSIONS`` and then ``OPTIMIZER_EXTENSIONS`` by name."""
    return {**EXTENSIONS, **OPTIMIZER_EXTENSIONS}


def libraries():
    """Every extension library by name: ``extensions()`` and then ``PREDICTION_EXTENSIONS``."""
    return {**extensions(), **PREDICTION_EXTENSIONS}


def every_library():
    """Every extension library by name: ``libraries()`` and then ``TRAINING_EXTENSIONS``."""
    return {**libraries(), **TRAINING_EXTENSIONS}


def all_libraries():
    """Every extension library by name: ``every_library()`` and then ``BOOTSTRAP_EXTENSIONS``."""
    return {**every_library(), **BOOTSTRAP_EXTENSIONS}


def built_libraries():
    """Every extension library by name: ``all_libraries()`` and then ``UNCERTAINTY_EXTENSIONS``."""
    return {**all_libraries(), **UNCERTAINTY_EXTENSIONS}


def _stale(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def _library_stale(lib, sources, headers):
    return _stale(lib, [os.path.join(CSRC, s) for s in sources] + headers)


def extension_needs_build(name):
    e = built_libraries()[name]
    return _library_stale(e.lib, e.sources, e.headers)


def needs_build():
    return _library_stale(LIB, SOURCES, HEADERS) or any(extension_needs_build(name) for name in built_libraries())


def _run(cmd, verbose):
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.check_call(cmd)


def _hipcc():
    return os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def _compile(src, obj, deps, extra_flags, force, verbose):
    """``csrc/<src>`` to the object ``obj``, when forced or when the source or one of ``deps`` is newer; returns ``obj``."""
    path = os.path.join(CSRC, src)
    if force or _stale(obj, [path] + deps):
        _run([_hipcc()] + FLAGS + EXTRA_FLAGS.get(src, []) + extra_flags + ["-c", path, "-o", obj], verbose)
    return obj


def _library(lib, sources, objdir, deps, extra_flags, link_flags, force, verbose):
    """``lib`` from ``sources``: the stale objects compiled by at most 8 workers, then one link."""
    os.makedirs(objdir, exist_ok=True)
    with ThreadPoolExecutor(max_workers=8) as pool:
        objs = list(pool.map(lambda s: _compile(s, os.path.join(objdir, os.path.splitext(s)[0] + ".o"), deps, extra_flags, force, verbose), sources))
    _run([_hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC", "-o", lib] + objs + link_flags, verbose)
    return lib


def _build_main(force, verbose=True):
    return _library(LIB, SOURCES, OBJ, HEADERS, [], [], force, verbose)


def build_diag(verbose=True):
    """``csrc/libdd_hotpath_diag.so``: the same library compiled with -DDD_TIMING_DIAG (timing ablations of single kernels whose
    results are then WRONG: DD_DCONV_REPEAT, DD_SPLIT_ABL).  Never loaded unless DD_HOTPATH_LIB points at it; not built by build()."""
    return _library(os.path.join(CSRC, "libdd_hotpath_diag.so"), SOURCES, os.path.join(CSRC, "build_diag"), HEADERS, ["-DDD_TIMING_DIAG"], [], False,
                    verbose)


def build_extension(name, force=False, verbose=True):
    """``built_libraries()[name].lib`` from its sources, when it is stale: the main library's flags; linked against ``libdd_hotpath.so`` (found
    beside it at load time, $ORIGIN), which therefore has to exist."""
    e = built_libraries()[name]
    if not force and not extension_needs_build(name):
        return e.lib
    return _library(e.lib, e.sources, OBJ, e.headers, [], ["-L" + CSRC, "-l:" + os.path.basename(LIB), "-Wl,-rpath,$ORIGIN"], force, verbose)


def build(force=False, verbose=True):
    """The main library and every extension library, each only when it is stale; returns the main library's path."""
    if force or _library_stale(LIB, SOURCES, HEADERS):
        _build_main(force, verbose)
    for name in built_libraries():
        build_extension(name, force, verbose)
    return LIB


if __name__ == "__main__":
    if "--diag" in sys.argv:
        print(build_diag())
    else:
        build(force="--force" in sys.argv)
