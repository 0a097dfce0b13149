"""CPU-side checks of the boundary: the C-ABI library loads without a GPU, exports every function include/dd_hotpath.h
declares, the ctypes table mirrors the header one to one, and the host-side validation refuses bad arguments before any
launch (no compute calls here)."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dd_hotpath.h")


def declared_functions():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(dd_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_declared_symbol():
    from driving_dirty_amd import _lib
    from driving_dirty_amd.build import LIB
    assert os.path.exists(LIB), "build the HIP library first (python __graft_entry__.py)"
    handle = ctypes.CDLL(LIB)
    names = declared_functions()
    assert len(names) >= 40
    for n in names:
        assert hasattr(handle, n), f"{n} is declared in include/dd_hotpath.h but not exported by the library"
    # the ctypes signature table binds exactly the declared set
    assert sorted(_lib.SIGNATURES) == names
    assert _lib.lib().dd_abi_version() == _lib.ABI_VERSION


def test_descriptor_structs_match_the_header():
    from driving_dirty_amd import _lib
    text = open(HEADER).read()
    for struct, cls in (("dd_conv_desc", _lib.ConvDesc), ("dd_gconv_desc", _lib.GConvDesc)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), text, flags=re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = [f.strip() for decl in re.findall(r"int32_t([^;]*);", body) for f in decl.split(",")]
        assert fields == [n for n, _ in cls._fields_], struct
        assert ctypes.sizeof(cls) == 4 * len(fields)


def test_host_side_validation_without_a_gpu():
    from driving_dirty_amd import _lib, ops
    lib = _lib.lib()
    d = _lib.ConvDesc(2, 16, 22, 32, 32, 32, 3, 1, 1, 0)
    assert lib.dd_conv_packed_floats(ctypes.byref(d), 0) == 36 * 64 * 4
    assert lib.dd_conv_wgrad_workspace_bytes(ctypes.byref(d)) > 0
    bad = _lib.ConvDesc(2, 16, 22, 32, 32, 32, 5, 1, 2, 0)
    assert lib.dd_conv_packed_floats(ctypes.byref(bad), 0) == -1
    assert b"k3 p1" in lib.dd_last_error()
    assert lib.dd_set_cu_budget(0) != 0 and lib.dd_set_cu_budget(256) == 0
    # NULL pointers / bad sizes are refused by the entry points themselves
    assert lib.dd_stitch6(None, None, None, None, 1, 4, 4, -1, None) == 2
    assert lib.dd_linear_fwd(None, None, None, None, 4, 8, 6, None, 0, None) != 0          # K % 4 != 0 -> unsupported first
    assert lib.dd_adam_step(None, None, None, None, 16, 1e-3, 0.9, 0.999, 1e-8, 1, 1.0, None) == 2
    assert lib.dd_adam_step_multi(None, 0, 1e-3, 0.9, 0.999, 1e-8, 1, 1.0, None) == 2
    # the Python shims refuse CPU tensors loudly: there is no CPU fallback
    with pytest.raises(_lib.HotpathError):
        ops.pool4_fwd(torch.zeros(1, 4, 4, 32))
    from driving_dirty_amd.components import Encoder
    with pytest.raises(RuntimeError):
        Encoder(16, 8, 3, 16, 22)(torch.zeros(2, 3, 16, 22))


def test_missing_library_fails_loudly(monkeypatch):
    from driving_dirty_amd import _lib
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB", "/nonexistent/libdd_hotpath.so")
    with pytest.raises(_lib.HotpathError):
        _lib.lib()


# ------------------------------------------------------------------------------------------------ the table is derived from the header
def _stripped_header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_derived_table_against_signatures_written_out_by_hand():
    from driving_dirty_amd import _lib
    P, I, L, F = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_float
    DP, GP, AP = ctypes.POINTER(_lib.ConvDesc), ctypes.POINTER(_lib.GConvDesc), ctypes.POINTER(_lib.AdamTensor)
    expected = {
        "dd_mlp_tail_fwd": (I, [P] * 25 + [I] * 4 + [F] * 6 + [I, P]),
        "dd_adam_step_multi": (I, [AP, I, F, F, F, F, I, F, P]),
        "dd_conv_wino2_wgrad": (I, [P, P, P, P, P, L, DP, P]),                  # the descriptor was a bare void* in the hand-written table
        "dd_dconv_fwd_colsum": (I, [P, P, P, P, P, GP, I, P, L, P]),            # likewise
        "dd_conv_bf16_pack": (I, [P, DP, I, P, P]),                             # likewise; the descriptor is the SECOND parameter here
        "dd_stitch6_ptrs": (I, [P, P, I, I, I, P]),                             # const float* const*
        "dd_strip6_fwd": (I, [P, I, P, P, P, P, I, I, I, P]),                   # const void* const*, const float* const*
        "dd_sqnorm": (I, [P, L, P, P, L, P]),                                   # int64_t in the middle, double*
        "dd_last_error": (ctypes.c_char_p, []),
        "dd_abi_version": (I, []),
        "dd_linear_workspace_bytes": (L, [I, I, I]),
        "dd_dconv_supported": (I, [GP]),                                        # int32_t return
        "dd_clip_scale": (I, [P, I, F, F, P, P]),
    }
    for name, sig in expected.items():
        assert _lib.SIGNATURES[name] == sig, name
    assert set(_lib.SIGNATURES) == set(_lib.parse_header(open(HEADER).read())[0])
    # the launch functions: exactly the declarations that end in `void* stream`
    decls = re.findall(r"\b(dd_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", _stripped_header())
    assert len(decls) == len(_lib.SIGNATURES)
    streamed = {n for n, params in decls if re.search(r"void\s*\*\s*stream\s*$", params)}
    assert _lib.STREAMED == streamed and streamed
    assert all(_lib.SIGNATURES[n][0] is I and _lib.SIGNATURES[n][1][-1] is P for n in streamed)
    # ... and a function that returns `int` without taking a stream is a setting, a version or a yes/no query known today
    plain_int = set(re.findall(r"^int\s+(dd_[a-z0-9_]+)\s*\(", _stripped_header(), flags=re.M)) - streamed
    assert plain_int == {"dd_abi_version", "dd_set_cu_budget", "dd_get_cu_budget", "dd_set_adam_blocks_per_cu", "dd_set_adam_spare_cus",
                         "dd_mlp_tail_supported"}
    # the library carries the derived types (lib() sets them on every function)
    assert _lib.lib().dd_conv_wino2_wgrad.argtypes == expected["dd_conv_wino2_wgrad"][1]


@pytest.mark.parametrize("text,names", [
    ("int dd_x(size_t n, void* stream);", ("size_t", "dd_x")),                         # a type outside the vocabulary
    ("int dd_w(const dd_other_desc* d, void* stream);", ("dd_other_desc", "dd_w")),    # a struct without a Structure: no silent void*
    ("int dd_u(dd_conv_desc* d);", ("dd_conv_desc*", "dd_u")),                         # descriptors are const
    ("float dd_y(void);", ("dd_y",)),                                                  # a return type outside the vocabulary
    ("int dd_z(int32_t);", ("int32_t", "dd_z")),                                       # a parameter without a name
    ("int dd_x(int32_t a", ("dd_x",)),                                                 # malformed
    ("int dd_x(int32_t a) { return 0; }", ("dd_x",)),
    ("int64_t dd_v(void* stream);", ("dd_v",)),                                        # a launch function returns int
    ("int dd_a(void); int dd_a(void);", ("dd_a", "twice")),
])
def test_header_parser_refuses_what_it_cannot_map(text, names):
    from driving_dirty_amd import _lib
    with pytest.raises(_lib.HotpathError) as e:
        _lib.parse_header(text)
    assert all(n in str(e.value) for n in names), str(e.value)


def test_header_parser_on_strings():
    from driving_dirty_amd import _lib
    sigs, streamed = _lib.parse_header("/* c */ #define X 1\nint dd_a(const float* const* t, int64_t n,\n  void* stream); // x\n"
                                       "const char* dd_b(void);\ntypedef struct dd_s { int32_t a; } dd_s;\nenum { A = 0 };\nint32_t dd_c(const dd_gconv_desc* d);")
    assert sigs == {"dd_a": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]), "dd_b": (ctypes.c_char_p, []),
                    "dd_c": (ctypes.c_int32, [ctypes.POINTER(_lib.GConvDesc)])}
    assert streamed == {"dd_a"}


# ------------------------------------------------------------------------------------------------ _lib.call / _lib.size without a GPU
ADAM_OPERANDS = (None, None, None, None, 16, 1e-3, 0.9, 0.999, 1e-8, 1, 1.0)


@pytest.fixture
def no_stream(monkeypatch):
    from driving_dirty_amd import _lib
    monkeypatch.setattr(_lib, "stream", lambda: None)      # torch.cuda.current_stream() needs a GPU; NULL = the default stream
    return _lib


class _Wrapped:
    """An entry point replaced on the CDLL object the way bench.py's AbiTimer does it."""

    def __init__(self, _lib, symbol):
        self.lib, self.symbol, self.seen = _lib.lib(), symbol, []

    def __enter__(self):
        self.inner = getattr(self.lib, self.symbol)

        def wrapper(*a):
            self.seen.append(a)
            return self.inner(*a)
        setattr(self.lib, self.symbol, wrapper)
        return self.seen

    def __exit__(self, *exc):
        setattr(self.lib, self.symbol, self.inner)


def test_call_raises_with_name_code_and_last_error(no_stream):
    _lib = no_stream
    with pytest.raises(_lib.HotpathError) as e:
        _lib.call("dd_adam_step", *ADAM_OPERANDS)
    assert "dd_adam_step" in str(e.value) and "code 2" in str(e.value) and "adam" in str(e.value).split(":", 1)[1]
    with pytest.raises(_lib.HotpathError, match="stream"):      # the stream is call()'s to append
        _lib.call("dd_adam_step", *ADAM_OPERANDS, None)
    with pytest.raises(_lib.HotpathError, match="operands"):
        _lib.call("dd_adam_step", *ADAM_OPERANDS[:-1])
    assert _lib.call("dd_set_cu_budget", 256) is None              # a status function without a stream: nothing appended
    with pytest.raises(_lib.HotpathError, match="dd_set_cu_budget"):
        _lib.call("dd_set_cu_budget", 0)
    # a yes/no query or a getter is not call()'s (its non-zero answer is no error), a status function not size()'s
    assert set(_lib.CALL_OPERANDS) == _lib.STREAMED | {"dd_set_cu_budget", "dd_set_adam_blocks_per_cu", "dd_set_adam_spare_cus"}
    for name, args in (("dd_mlp_tail_supported", (3, 16, 16, 8)), ("dd_get_cu_budget", ()), ("dd_no_such_function", ())):
        with pytest.raises(_lib.HotpathError, match="call\\(\\) serves"):
            _lib.call(name, *args)
    with pytest.raises(_lib.HotpathError, match="size\\(\\) serves"):
        _lib.size("dd_set_cu_budget", 256)


def test_call_goes_through_a_wrapper_installed_on_the_library(no_stream):
    _lib = no_stream
    original = _lib.lib().dd_adam_step
    with _Wrapped(_lib, "dd_adam_step") as seen:
        with pytest.raises(_lib.HotpathError):
            _lib.call("dd_adam_step", *ADAM_OPERANDS)
    assert len(seen) == 1 and len(seen[0]) == 12 and seen[0][:11] == ADAM_OPERANDS and seen[0][11] is None      # positional, header order, stream last
    assert all(type(x) in (int, float) for x in seen[0][4:11])                                                    # scalars as plain numbers
    assert _lib.lib().dd_adam_step is original
    with _Wrapped(_lib, "dd_adam_step") as seen:                   # installed AFTER a first call: nothing was cached
        with pytest.raises(_lib.HotpathError):
            _lib.call("dd_adam_step", *ADAM_OPERANDS)
    assert len(seen) == 1
    d = _lib.ConvDesc(2, 16, 22, 32, 32, 32, 3, 1, 1, 0)
    with _Wrapped(_lib, "dd_conv_pack") as seen:
        with pytest.raises(_lib.HotpathError, match="dd_conv_pack"):
            _lib.call("dd_conv_pack", None, None, d, 0)
    assert seen[0][2]._obj is d and seen[0][2]._obj.cin_real == 32 and seen[0][3] == 0      # what bench.py's predicates read
    with _Wrapped(_lib, "dd_conv_packed_floats") as seen:
        assert _lib.size("dd_conv_packed_floats", d, 0) == 36 * 64 * 4
    assert seen[0][0]._obj is d


def test_size_raises_on_refusal_and_passes_zero(no_stream):
    _lib = no_stream
    bad = _lib.ConvDesc(2, 16, 22, 32, 32, 32, 5, 1, 2, 0)
    with pytest.raises(_lib.HotpathError) as e:
        _lib.size("dd_conv_packed_floats", bad, 0)
    assert "dd_conv_packed_floats" in str(e.value) and "k3 p1" in str(e.value)
    assert _lib.size("dd_linear_workspace_bytes", 3, 8, 1056) == _lib.lib().dd_linear_workspace_bytes(3, 8, 1056) >= 0
    assert _lib.lib().dd_label_components_workspace_bytes(1, 8, 8) == 0      # a query whose answer for a supported shape IS zero ...
    assert _lib.size("dd_label_components_workspace_bytes", 1, 8, 8) == 0    # ... comes through unharmed
    with pytest.raises(_lib.HotpathError):
        _lib.size("dd_label_components_workspace_bytes", 1, 8, 1 << 20)


def test_typed_descriptor_pointers_refuse_the_wrong_struct():
    from driving_dirty_amd import _lib
    lib = _lib.lib()
    g = _lib.GConvDesc()
    with pytest.raises(ctypes.ArgumentError):
        lib.dd_conv_wino2_packed_floats(ctypes.byref(g))           # accepted as void* by the hand-written table
    assert lib.dd_conv_wino2_packed_floats(None) == -1
    assert lib.dd_conv_wino2_packed_floats(ctypes.byref(_lib.ConvDesc(2, 16, 22, 32, 32, 32, 3, 1, 1, 0))) > 0


def test_operand_check_and_retained_names():
    from driving_dirty_amd import _lib, gconv, ops
    assert ops._p is _lib.ptr is gconv._p and ops._stream is _lib.stream is gconv._stream and ops._dev is _lib.dev
    assert ops.check is _lib.check and ops._lib is _lib and ops.C is ctypes
    with pytest.raises(_lib.HotpathError, match="x: expected a contiguous fp32 device tensor, got torch.float32 on cpu"):
        _lib.dev(torch.zeros(2), "x")
    with pytest.raises(_lib.HotpathError, match="x: expected a contiguous bf16 device tensor, got torch.float32"):
        _lib.dev(torch.zeros(2), "x", dtype=torch.bfloat16)
    # ptr: the device pointer; a parameter's pending all-gather (ddp.PARAM_WAITS) is waited for once, at first use
    from driving_dirty_amd import ddp
    t, waited = torch.zeros(4), []
    assert _lib.ptr(None) is None and _lib.ptr(t).value == t.data_ptr()
    ddp.PARAM_WAITS[t.data_ptr()] = lambda: waited.append(1)
    try:
        assert _lib.ptr(t).value == t.data_ptr() and waited == [1] and t.data_ptr() not in ddp.PARAM_WAITS
        assert _lib.ptr(t).value == t.data_ptr() and waited == [1]
    finally:
        ddp.PARAM_WAITS.pop(t.data_ptr(), None)


def test_every_call_site_in_the_package_has_the_headers_operand_count():
    """Static: each ``call("dd_x", ...)`` / ``size("dd_x", ...)`` in the package names a declared function and passes as many operands as
    the header declares (in front of the stream), so a parameter dropped at a site fails here and not in a launch."""
    import ast
    import glob
    from driving_dirty_amd import _lib
    pkg = os.path.join(ROOT, "driving-dirty_amd")
    sites = 0
    for path in sorted(glob.glob(os.path.join(pkg, "*.py"))):
        for node in ast.walk(ast.parse(open(path).read())):
            fn = node.func if isinstance(node, ast.Call) else None
            name = fn.id if isinstance(fn, ast.Name) else fn.attr if isinstance(fn, ast.Attribute) else None
            if name not in ("call", "size") or not node.args or path.endswith("_lib.py"):
                continue
            where = f"{os.path.basename(path)}:{node.lineno}"
            first = node.args[0]
            if not (isinstance(first, ast.Constant) and isinstance(first.value, str)):
                continue                                            # a computed name (a kernel family, an entry passed in): checked when it runs
            assert first.value in _lib.SIGNATURES, f"{where}: {first.value} is not declared in the header"
            declared = _lib.CALL_OPERANDS if name == "call" else _lib.SIZE_OPERANDS
            assert first.value in declared, f"{where}: {name}() does not serve {first.value}"
            if not any(isinstance(a, ast.Starred) for a in node.args):
                assert len(node.args) - 1 == declared[first.value], f"{where}: {first.value} takes {declared[first.value]} operands"
            sites += 1
    assert sites


def test_call_waits_for_a_pending_parameter_gather_once(no_stream):
    """call() converts tensors in its own loop: the same pop-and-wait as ptr, on the one dict ddp owns (bound once by _lib)."""
    _lib = no_stream
    from driving_dirty_amd import ddp
    assert _lib._WAITS is ddp.PARAM_WAITS
    lib, t, waited, seen = _lib.lib(), torch.zeros(4), [], []
    inner = lib.dd_add
    setattr(lib, "dd_add", lambda *a: seen.append(a) or 0)      # a stub: host pointers must not reach a kernel
    ddp.PARAM_WAITS[t.data_ptr()] = lambda: waited.append(1)
    try:
        _lib.call("dd_add", t, t, t, 4)
        assert waited == [1] and t.data_ptr() not in ddp.PARAM_WAITS
        _lib.call("dd_add", t, None, t, 4)
        assert waited == [1]
    finally:
        ddp.PARAM_WAITS.pop(t.data_ptr(), None)
        setattr(lib, "dd_add", inner)
    assert [type(x) for x in seen[0]] == [ctypes.c_void_p] * 3 + [int, type(None)] and seen[0][0].value == t.data_ptr() and seen[1][1] is None
