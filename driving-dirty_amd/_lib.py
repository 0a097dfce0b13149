"""ctypes binding of ``csrc/libdd_hotpath.so``, derived from its C ABI ``include/dd_hotpath.h``.

There is no fallback: if the library is missing or a call fails, an exception is raised.

``SIGNATURES`` {name: (restype, argtypes)} is parsed from the header at import (``parse_header``); nothing is declared twice.
``call(name, *operands)`` is the one way the package enters a status-returning entry point, ``size(name, *args)`` the one way it
asks a ``*_bytes`` / ``*_floats`` / ``*_elems`` query that answers a negative number for "refused".

The boundary is also patched from OUTSIDE: bench.py's ``AbiTimer`` replaces entry points on the ``CDLL`` object by Python wrappers
(``setattr(lib(), symbol, timed)``) whose predicates read the arguments, and its ``KernelTimer`` rebinds functions of ``ops``.
What they rely on, and what ``call`` therefore keeps by construction:

  * an entry point is looked up on the ``CDLL`` object at EVERY call, ``getattr(lib(), name)``; a function object is never cached
    (a cached one would bypass the timers without a sound, and bench.py's roofline line would be computed from nothing);
  * arguments reach the function positionally, in header order;
  * descriptors go as ``ctypes.byref(struct)`` (the predicates read ``x[5]._obj.cin``);
  * scalars go as plain Python numbers (the predicates compute ``x[4] >= 100_000_000`` and ``x[6] * x[7]``);
  * ``ops.conv_fwd_bits``, ``ops.conv_wino_fwd_bits``, ``ops.conv_wino2_fwd_bits`` (``(x, packed, bias, desc)``) and
    ``ops.conv_wino2_dgrad_w1`` stay module-level functions of ``ops`` that ``EncoderConvStack`` reaches through the module's
    globals at call time; ``ops.WINOGRAD`` and ``ops.WINOGRAD_2D`` stay module attributes read at call time.
"""
import ctypes as C
import os
import re

import torch  # noqa: F401  -- FIRST: the library must bind to the HIP runtime torch has loaded (same soname
#                              libamdhip64.so.7); loading ours first would put a second runtime in the process

from . import ddp as _ddp
from .build import HEADER, LIB

if os.environ.get("DD_HOTPATH_LIB"):      # another BUILD of the same library (tools/: A/B of two builds on one box); must exist, same ABI
    LIB = os.environ["DD_HOTPATH_LIB"]

_i32, _i64, _f32, _p = C.c_int32, C.c_int64, C.c_float, C.c_void_p


class HotpathError(RuntimeError):
    pass


class ConvDesc(C.Structure):
    """struct dd_conv_desc"""
    _fields_ = [(n, _i32) for n in ("batch", "height", "width", "cin_real", "cin_store", "cout",
                                    "ksize", "stride", "pad", "rows_per_task")]


class GConvDesc(C.Structure):
    """struct dd_gconv_desc"""
    _fields_ = [(n, _i32) for n in ("batch", "in_h", "in_w", "in_cstore", "in_coff", "cin", "out_h", "out_w",
                                    "omem_h", "omem_w", "out_cstore", "out_coff", "cout", "kh", "kw", "stride_h",
                                    "stride_w", "dil_h", "dil_w", "pad_h", "pad_w", "div_h", "div_w", "ostride_h",
                                    "ostride_w", "ooff_h", "ooff_w", "mask_pass_lo", "mask_pass_hi")]


class AdamTensor(C.Structure):
    """struct dd_adam_tensor"""
    _fields_ = [("p", _p), ("g", _p), ("m", _p), ("v", _p), ("n", _i64)]


# ---- the header is the single source of the signatures ------------------------------------------------------------------------
_SCALARS = {"int": _i32, "int32_t": _i32, "int64_t": _i64, "float": _f32}
_STRUCTS = {"dd_conv_desc": ConvDesc, "dd_gconv_desc": GConvDesc, "dd_adam_tensor": AdamTensor}
_POINTEES = {"void", "char", "unsigned char", "float", "double", "uint8_t", "uint16_t", "uint32_t", "uint64_t", "int32_t", "int64_t"}
_RETURNS = {"int": _i32, "int32_t": _i32, "int64_t": _i64, "const char *": C.c_char_p}
# what the header holds besides declarations: the extern "C" brackets, struct and enum definitions, preprocessor lines
_NOT_DECLARATIONS = (r"#ifdef __cplusplus.*?#endif", r"typedef\s+struct\s+\w+\s*\{.*?\}\s*\w+\s*;", r"enum\s*\{.*?\}\s*;", r"#[^\n]*")


def _ctype(spelling, decl):
    """One parameter type of the header's vocabulary -> ctypes.  Scalars by name; ``const <struct>*`` -> POINTER of its Structure; a
    pointer (or ``T* const*`` table) to a plain C type -> c_void_p.  Anything else is refused."""
    t = " ".join(spelling.replace("*", " * ").split())
    if t in _SCALARS:
        return _SCALARS[t]
    m = re.fullmatch(r"(const )?(\w+(?: \w+)?) \*( const \*)?", t)
    if m and m.group(2) in _STRUCTS and m.group(1) and not m.group(3):
        return C.POINTER(_STRUCTS[m.group(2)])
    if m and m.group(2) in _POINTEES:
        return _p
    raise HotpathError(f"include/dd_hotpath.h: no ctypes mapping for the type '{spelling.strip()}' in: {decl}")


def parse_header(text):
    """Text of the header -> ({name: (restype, argtypes)}, frozenset of the names whose last parameter is called ``stream``).
    Every statement that is left after comments, preprocessor lines, the struct and enum definitions are taken out must read
    ``ret dd_name(params);`` in the types above: a declaration this cannot map raises HotpathError naming it."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    for pattern in _NOT_DECLARATIONS:
        text = re.sub(pattern, " ", text, flags=re.S)
    signatures, streamed = {}, set()
    for decl in (" ".join(s.split()) for s in text.split(";")):
        if not decl:
            continue
        m = re.fullmatch(r"(int|int32_t|int64_t|const char ?\*) ?(dd_\w+) ?\((.*)\)", decl)
        if not m:
            raise HotpathError(f"include/dd_hotpath.h: not a 'ret dd_name(params);' declaration: {decl}")
        ret, name, params = " ".join(m.group(1).replace("*", " *").split()), m.group(2), m.group(3).strip()
        if name in signatures:
            raise HotpathError(f"include/dd_hotpath.h: {name} is declared twice")
        argtypes, last = [], None
        for param in ([] if params == "void" else params.split(",")):
            pm = re.fullmatch(r"\s*(.*?[\s*])(\w+)\s*", param)
            if not pm:
                raise HotpathError(f"include/dd_hotpath.h: parameter '{param.strip()}' has no name in: {decl}")
            argtypes.append(_ctype(pm.group(1), decl))
            last = pm.group(2)
        signatures[name] = (_RETURNS[ret], argtypes)
        if last == "stream":
            if argtypes[-1] is not _p or _RETURNS[ret] is not _i32:
                raise HotpathError(f"include/dd_hotpath.h: a launch function returns int and ends in 'void* stream': {decl}")
            streamed.add(name)
    return signatures, frozenset(streamed)


with open(HEADER) as _f:
    SIGNATURES, STREAMED = parse_header(_f.read())
# operands a caller supplies: to call() for the launch functions (the stream is appended) and the dd_set_* settings, to size() for the
# int64 queries.  The yes/no queries and the getters are neither: their non-zero answer is no error code.
CALL_OPERANDS = {name: len(args) - (name in STREAMED) for name, (res, args) in SIGNATURES.items()
                 if name in STREAMED or (res is _i32 and name.startswith("dd_set_"))}
SIZE_OPERANDS = {name: len(args) for name, (res, args) in SIGNATURES.items() if res is _i64}

ABI_VERSION = 4      # include/dd_hotpath.h: DD_ABI_VERSION
_lib = None


def lib():
    """Load the shared library once; raise (never fall back) when it is absent."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB):
            raise HotpathError(
                f"{LIB} is missing: build the HIP extension first (python -m driving_dirty_amd.build "
                "or __graft_entry__.build()). There is no CPU / eager fallback for the hot path.")
        handle = C.CDLL(LIB)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(handle, name)          # AttributeError if the .so lacks a declared symbol
            fn.restype, fn.argtypes = res, args
        if handle.dd_abi_version() != ABI_VERSION:
            raise HotpathError("libdd_hotpath.so ABI version mismatch")
        _lib = handle
    return _lib


def check(rc, what):
    if rc != 0:
        raise HotpathError(f"{what} failed (code {rc}): {lib().dd_last_error().decode()}")


# ---- operands --------------------------------------------------------------------------------------------------------------
def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t):
    """Device pointer of a kernel operand.  A parameter whose all-gather (sharded optimizer, ddp.GradSync) is still in flight
    is waited for -- on the current stream -- the first time it is handed to a kernel.  For callers that build pointer tables or call
    lib() themselves; call() does the same per tensor operand inside its own loop."""
    if t is None:
        return None
    p = t.data_ptr()
    if _ddp.PARAM_WAITS:
        wait = _ddp.PARAM_WAITS.pop(p, None)
        if wait is not None:
            wait()
    return C.c_void_p(p)


_DTYPE_NAMES = {torch.float32: "fp32", torch.bfloat16: "bf16"}


def dev(t, name, shape=None, dtype=torch.float32):
    """Validate a kernel operand on the HOST before any launch (a faulting kernel can reset the GPU)."""
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == dtype and t.is_contiguous()):
        raise HotpathError(f"{name}: expected a contiguous {_DTYPE_NAMES.get(dtype, dtype)} device tensor, got "
                           f"{getattr(t, 'dtype', type(t))} on {getattr(t, 'device', '?')} "
                           f"contiguous={getattr(t, 'is_contiguous', lambda: '?')()}")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise HotpathError(f"{name}: shape {tuple(t.shape)} != expected {tuple(shape)}")
    return t


# The loop in call() is the host cost of every launch.  Measured against the idiom it replaces (check(lib().dd_x(_p(a), ...,
# _stream()), "dd_x")): operands told by their class first, ``ptr`` inlined and the names below bound once keep it level with it;
# through a helper and with attribute lookups per operand it cost 1.5 us more per call.
_PLAIN = frozenset((int, float, bool, type(None)))      # operands that pass as they are
_Tensor, _Structure, _byref, _void_p, _WAITS = torch.Tensor, C.Structure, C.byref, C.c_void_p, _ddp.PARAM_WAITS


def _refuse(name, operands, declared):
    if name not in declared:
        raise HotpathError(f"{name}: not an entry point that " + ("call() serves (a launch function or a dd_set_* setting)"
                                                                   if declared is CALL_OPERANDS else "size() serves (an int64_t query)"))
    raise HotpathError(f"{name}: {len(operands)} operands given, the header declares {declared[name]}"
                       + (" in front of the stream, which call() appends itself" if name in STREAMED else ""))


def call(name, *operands):
    """Enter a launch function (last parameter ``stream``: the current torch stream is appended) or a ``dd_set_*`` setting with
    ``operands`` in header order: a tensor goes as its device pointer (as ``ptr`` gives it), a Structure as byref; None, numbers,
    ctypes arrays and pointers as they are.  Another operand count than the header's, or any other function, is refused.  Raises
    HotpathError with the name, the code and dd_last_error() on a non-zero return.  The function is looked up on the CDLL object NOW
    (see the module docstring: never cache it)."""
    if len(operands) != CALL_OPERANDS.get(name):
        _refuse(name, operands, CALL_OPERANDS)
    args = []
    for a in operands:
        if a.__class__ in _PLAIN:
            args.append(a)
        elif isinstance(a, _Tensor):
            p = a.data_ptr()
            if _WAITS:
                wait = _WAITS.pop(p, None)
                if wait is not None:
                    wait()
            args.append(_void_p(p))
        else:
            args.append(_byref(a) if isinstance(a, _Structure) else a)
    if name in STREAMED:
        args.append(stream())
    rc = getattr(lib(), name)(*args)
    if rc != 0:
        check(rc, name)


def size(name, *args):
    """An ``int64_t`` query (``*_bytes`` / ``*_floats`` / ``*_elems``; descriptors go as they go to call()): its value, or HotpathError
    with dd_last_error() when it answers a negative one."""
    if len(args) != SIZE_OPERANDS.get(name):
        _refuse(name, args, SIZE_OPERANDS)
    n = getattr(lib(), name)(*[_byref(a) if isinstance(a, _Structure) else a for a in args])
    if n < 0:
        raise HotpathError(f"{name} refused (returned {n}): {lib().dd_last_error().decode()}")
    return n


# ---- extension libraries --------------------------------------------------------------------------------------------------------
class Extension:
    """The binder of an extension library, from its entry in ``build.EXTENSIONS``: launch functions that are not part of
    include/dd_hotpath.h (its set of functions is pinned), declared in a header of their own and built into a library of their own that
    links against ``libdd_hotpath.so`` for ``dd_fail`` / ``dd_last_error()`` (build.py).  The module of each extension holds one and
    publishes its parts as module-level names.  The ctypes table comes from the header through ``parse_header`` -- the one parser -- and
    ``launch(name, *operands)`` enters a function the way ``call`` does: looked up on the ``CDLL`` at every call, operands in header
    order, the current torch stream appended, ``HotpathError`` with the library's message on a non-zero return."""

    def __init__(self, entry):
        self.header, self.library, self.what = entry.header, entry.lib, entry.what      # ``what``: the missing-library message's noun
        with open(self.header) as f:
            self.text = f.read()
        self.signatures, self.streamed = parse_header(self.text)
        # every function ends in the stream, which launch() appends
        self.operands = {name: len(args) - 1 for name, (res, args) in self.signatures.items()}
        self._handle = None

    def constant(self, name, cast=int):
        """The number a ``#define`` of the header gives ``name``, brackets and a float's ``f`` taken off: ``(-1.0f)`` is -1.0 to float."""
        return cast(re.search(rf"^#define {name} \(?(-?[\d.]+)f?\)?", self.text, re.M).group(1))

    def lib(self):
        """Load the library once, after the main library (it links against it: ``dd_fail``); raise when it is absent."""
        if self._handle is None:
            lib()
            if not os.path.exists(self.library):
                raise HotpathError(f"{self.library} is missing: build the HIP extensions first (python -m driving_dirty_amd.build or "
                                   f"__graft_entry__.build()). There is no CPU / eager fallback for {self.what}.")
            handle = C.CDLL(self.library)
            for name, (res, args) in self.signatures.items():
                fn = getattr(handle, name)          # AttributeError if the .so lacks a declared symbol
                fn.restype, fn.argtypes = res, args
            self._handle = handle
        return self._handle

    def last_error(self):
        """The message of the calling thread's last failure: ``dd_last_error()`` of the ``libdd_hotpath.so`` this library is linked
        against (the one beside it; DD_HOTPATH_LIB may have sent ``lib()`` to another build)."""
        from . import build as _build
        hot = lib() if LIB == _build.LIB else C.CDLL(_build.LIB)
        fn = hot.dd_last_error
        fn.restype = C.c_char_p
        return fn().decode()

    def launch(self, name, *operands):
        """Enter a launch function of the header with ``operands`` in header order; a tensor goes as its device pointer, ctypes
        arrays, numbers and None as they are; the current torch stream is appended.  Raises HotpathError on another operand count
        than the header's and on a non-zero return.  The function is looked up on the CDLL object NOW."""
        if len(operands) != self.operands.get(name):
            where = "include/" + os.path.basename(self.header)
            raise HotpathError(f"{name}: " + (f"not a function of {where}" if name not in self.operands else
                                              f"{len(operands)} operands given, the header declares {self.operands[name]} in front of the stream"))
        args = [ptr(a) if isinstance(a, torch.Tensor) else a for a in operands]
        rc = getattr(self.lib(), name)(*args, stream())
        if rc != 0:
            raise HotpathError(f"{name} failed (code {rc}): {self.last_error()}")
