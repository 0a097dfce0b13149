"""Guard-band arena for the C ABI's launch functions: the operands of ONE call laid out in one ``uint8`` allocation that is filled
with 0xFF (NaN as fp32 / bf16 / fp64, -1 as int32 / int64, 255 as a byte), every operand with a 64 KiB gap in front of it and
behind it, at the alignment include/dd_hotpath.h promises to accept and no more.

    arena = Arena(dev, "minimal")
    x = arena.put(x_cpu, 16, "x")                 # an input: copied in, must come back bit-identical
    y = arena.out((m, n), torch.float32, 16, "y") # an output: left 0xFF, must come back finite
    rm = arena.inout(rm_cpu, 16, "running_mean")  # read and written
    ws = arena.workspace(nbytes, 16, "workspace") # exactly the bytes the query answered, left 0xFF
    _lib.call("dd_...", x, y, rm, ws, ...)        # the tensors are views into the arena; call() takes data_ptr()
    outs = arena.verify()                         # {"y": ..., "running_mean": ...} on the CPU

Modes: ``natural`` puts every payload on a 256-byte boundary (what torch.empty gives the wrappers), ``minimal`` at an address
that is ``align`` modulo 256 -- aligned to what the header asks for that operand and to nothing larger.

What ``verify`` sees: a byte written outside an operand (front or behind, with the distance); an input that changed; an output
that holds a NaN / Inf -- which is what a read from a gap, from an unwritten workspace row or an accumulate onto a workspace
turns into once it reaches a result.  What it cannot see: an over-read whose value is discarded.
"""
import ctypes as C

import torch

GAP = 64 * 1024      # more than any tile row of the kernels (128 pixels x 32 channels x 4 B = 16 KiB)
FILL = 0xFF
MODES = ("natural", "minimal")
_FLOATS = (torch.float32, torch.float64, torch.bfloat16, torch.float16)


class GuardError(AssertionError):
    """``operand``: the name given at placement; ``what``: 'front' / 'behind' (a damaged gap), 'input' (an input changed),
    'nonfinite' (a float output holds NaN / Inf); ``offset``: bytes from the payload's edge (front: -1 is the byte just in front
    of it; behind: 0 is the byte just behind it) or the element index."""

    def __init__(self, operand, what, offset, text):
        super().__init__(f"{operand}: {text}")
        self.operand, self.what, self.offset = operand, what, offset


class _Operand:
    __slots__ = ("name", "kind", "start", "nbytes", "view", "saved", "check_finite")


class Arena:
    def __init__(self, dev, mode="natural", capacity=8 << 20):
        assert mode in MODES, mode
        self.mode, self.dev = mode, torch.device(dev)
        self.buf = torch.full((capacity + 256,), FILL, dtype=torch.uint8, device=self.dev)
        self._base = self.buf.data_ptr()
        self._origin = (-self._base) % 256          # first 256-byte boundary of the allocation
        self._end = self._origin                    # end of the last payload (the first gap starts at the origin)
        self.operands = []

    # ---- placement ----------------------------------------------------------------------------------------------------------
    def _place(self, kind, name, nbytes, dtype, shape, align):
        assert align in (2, 4, 8, 16, 32, 64, 128), align
        assert align % torch.empty((), dtype=dtype).element_size() == 0, (align, dtype)
        assert all(o.name != name for o in self.operands), f"two operands called {name}"
        start = self._end + GAP
        want = 0 if self.mode == "natural" else align      # address modulo 256
        start += (want - (self._base + start)) % 256
        if start + nbytes + GAP > self.buf.numel():
            raise ValueError(f"arena of {self.buf.numel()} bytes is too small for {name} ({nbytes} bytes): pass a larger capacity")
        op = _Operand()
        op.name, op.kind, op.start, op.nbytes, op.saved, op.check_finite = name, kind, start, nbytes, None, False
        op.view = self.buf[start:start + nbytes].view(dtype).view(shape)
        self._end = start + nbytes
        self.operands.append(op)
        return op

    def _name(self, name, kind):
        return name if name is not None else f"{kind}{len(self.operands)}"

    def put(self, tensor, align=16, name=None):
        """An input: copied in; ``verify`` wants it back bit for bit."""
        t = tensor.detach().contiguous()
        op = self._place("input", self._name(name, "input"), t.numel() * t.element_size(), t.dtype, tuple(t.shape), align)
        op.view.copy_(t)
        op.saved = self.buf[op.start:op.start + op.nbytes].clone()
        return op.view

    def out(self, shape, dtype=torch.float32, align=16, name=None, check_finite=True):
        """An output, left 0xFF.  ``check_finite=False`` for one the entry point is documented to write only in part."""
        shape = (shape,) if isinstance(shape, int) else tuple(shape)
        n = 1
        for s in shape:
            n *= s
        op = self._place("output", self._name(name, "output"), n * torch.empty((), dtype=dtype).element_size(), dtype, shape, align)
        op.check_finite = check_finite and dtype in _FLOATS
        return op.view

    def inout(self, tensor, align=16, name=None):
        """Read and written (running statistics, Adam's p / m / v): copied in, returned by ``verify``, must come back finite."""
        t = tensor.detach().contiguous()
        op = self._place("inout", self._name(name, "inout"), t.numel() * t.element_size(), t.dtype, tuple(t.shape), align)
        op.view.copy_(t)
        op.check_finite = t.dtype in _FLOATS
        return op.view

    def workspace(self, nbytes, align=16, name=None):
        """Exactly ``nbytes`` bytes (what the ``*_workspace_bytes`` query answered), left 0xFF."""
        return self._place("workspace", self._name(name, "workspace"), int(nbytes), torch.uint8, (int(nbytes),), align).view

    def address(self, name):
        return self._base + self._find(name).start

    def _find(self, name):
        for op in self.operands:
            if op.name == name:
                return op
        raise KeyError(name)

    def gaps(self, name):
        """(bytes of 0xFF in front of the operand, bytes behind it), up to the neighbouring payloads."""
        i = self.operands.index(self._find(name))
        op = self.operands[i]
        front = op.start - (self.operands[i - 1].start + self.operands[i - 1].nbytes if i else self._origin)
        behind = (self.operands[i + 1].start if i + 1 < len(self.operands) else op.start + op.nbytes + GAP) - (op.start + op.nbytes)
        return front, behind

    # ---- the check ----------------------------------------------------------------------------------------------------------
    def _damage(self, lo, hi):
        """Offsets (in the allocation) of the bytes of [lo, hi) that are no longer 0xFF."""
        return lo + torch.nonzero(self.buf[lo:hi] != FILL).flatten()

    def verify(self):
        """After the call: synchronises, then raises GuardError for the first of: a damaged gap byte (naming the nearer operand
        and the side), a changed input, a non-finite float output.  Returns {name: CPU copy} of the outputs and in-out operands."""
        if self.dev.type == "cuda":
            torch.cuda.synchronize(self.dev)
        ops = self.operands
        for i, op in enumerate(ops):
            prev_end = ops[i - 1].start + ops[i - 1].nbytes if i else self._origin
            mid = prev_end + (op.start - prev_end) // 2 if i else prev_end       # a shared gap: each half belongs to the nearer payload
            bad = self._damage(mid, op.start)
            if bad.numel():
                off = int(bad.max()) - op.start
                raise GuardError(op.name, "front", off, f"{bad.numel()} byte(s) written in FRONT of it, the nearest {-off} byte(s) "
                                 f"before its start (value 0x{int(self.buf[op.start + off]):02x})")
            end = op.start + op.nbytes
            nxt = ops[i + 1].start if i + 1 < len(ops) else end + GAP
            stop = end + (nxt - end) // 2 if i + 1 < len(ops) else nxt
            bad = self._damage(end, stop)
            if bad.numel():
                off = int(bad.min()) - end
                raise GuardError(op.name, "behind", off, f"{bad.numel()} byte(s) written BEHIND it, the first {off} byte(s) past "
                                 f"its end (value 0x{int(self.buf[end + off]):02x})")
        for op in ops:
            if op.kind == "input":
                now = self.buf[op.start:op.start + op.nbytes]
                if not torch.equal(now, op.saved):
                    byte = int(torch.nonzero(now != op.saved).flatten()[0])
                    elem = byte // op.view.element_size()
                    raise GuardError(op.name, "input", elem, f"an INPUT was changed by the call: element {elem} (byte {byte})")
        outs = {}
        for op in ops:
            if op.kind in ("output", "inout"):
                got = op.view.detach().cpu().clone()
                if op.check_finite:
                    fin = torch.isfinite(got.float() if got.dtype == torch.bfloat16 else got).flatten()
                    if not bool(fin.all()):
                        elem = int(torch.nonzero(~fin).flatten()[0])
                        raise GuardError(op.name, "nonfinite", elem, f"element {elem} of {fin.numel()} is NaN / Inf ({int((~fin).sum())} in all): "
                                         "left unwritten, or a value from outside an operand / from an unwritten or accumulated-onto "
                                         "workspace reached it")
                outs[op.name] = got
        return outs


# ---- pointer tables built from arena views ------------------------------------------------------------------------------------
def ptr_table(tensors):
    """HOST array of device pointers (the ``*_ptrs`` entry points, dd_strip6_*)."""
    return (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def adam_table(quads):
    """HOST array of dd_adam_tensor from (p, g, m, v) views (dd_adam_step_multi*, dd_sqnorm_multi)."""
    from driving_dirty_amd import _lib
    table = (_lib.AdamTensor * len(quads))()
    for e, (p, g, m, v) in zip(table, quads):
        e.p, e.g, e.m, e.v, e.n = p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel()
    return table


# ---- cases --------------------------------------------------------------------------------------------------------------------
class Check:
    """One compared result.  ``how``: 'peak' = max |got - ref| / max |ref| < tol (rel_err of tests/test_gpu_parity.py), 'scalar' =
    |got - ref| / |ref| < tol, 'abs' = max |got - ref| <= tol, 'exact' = equal as they are, 'asserted' = the case's fn compared it
    with ``ref`` by a criterion of its own before returning (the result is still compared across the two alignments)."""

    def __init__(self, label, got, ref, tol=None, how="peak", floor=1e-30):
        self.label, self.got, self.ref, self.tol, self.how, self.floor = label, got, ref, tol, how, floor

    def error(self):
        got, ref = self.got.detach().double().cpu(), torch.as_tensor(self.ref).detach().double().cpu()
        assert got.shape == ref.shape, (self.label, got.shape, ref.shape)
        if self.how == "asserted":      # fn has held it to its reference itself (a criterion of another test, such as bf16 ulps)
            return 0.0
        if self.how == "exact":
            return 0.0 if torch.equal(got, ref) else float("inf")
        err = float((got - ref).abs().max())
        if self.how == "peak":
            return err / max(float(ref.abs().max()), self.floor)
        if self.how == "scalar":
            return err / abs(float(ref))
        return err


class Case:
    """``entry``: the entry point(s) the case is about; ``fn(arena, mode) -> [Check]`` builds the operands in the arena, calls,
    runs ``arena.verify()`` and returns what to compare; ``picks_kernel_by_alignment``: the launcher chooses another kernel in
    minimal mode (then the two modes need not agree bit for bit, and fn proves that both kernels ran); ``crosses``: the same for
    a case that keeps the bit-for-bit comparison although the kernel differs; ``capacity``: arena bytes."""

    def __init__(self, name, entry, fn, picks_kernel_by_alignment=False, capacity=8 << 20, crosses=None):
        self.name, self.entry, self.fn = name, (entry,) if isinstance(entry, str) else tuple(entry), fn
        self.picks_kernel_by_alignment, self.capacity = picks_kernel_by_alignment, capacity
        # the alignment-picking launchers whose two kernels the two modes of this case run (the case asserts the launcher's predicate)
        self.crosses = tuple(crosses) if crosses is not None else (self.entry if picks_kernel_by_alignment else ())


def run_case(case, dev):
    """Both alignment modes: every result finite (verify), within its tolerance of the fp64 reference, the gaps and inputs
    intact; and the minimal-mode results bit-identical to the natural-mode ones unless the launcher picks its kernel by alignment."""
    results = {}
    for mode in MODES:
        arena = Arena(dev, mode, case.capacity)
        checks = case.fn(arena, mode)
        assert checks, case.name
        for c in checks:
            err = c.error()
            print(f"{case.name} [{mode}] {c.label}: {c.how} error {err:.3g} (bound {c.tol})")
            assert (err == 0.0) if c.how in ("exact", "asserted") else (err < c.tol if c.how != "abs" else err <= c.tol), (case.name, mode, c.label, err, c.tol)
        results[mode] = checks
    if not case.picks_kernel_by_alignment:
        assert len(results["natural"]) == len(results["minimal"]), f"{case.name}: the two modes return different lists of results"
        for a, b in zip(results["natural"], results["minimal"]):
            assert a.label == b.label
            ga, gb = a.got.detach().cpu().contiguous().reshape(-1), b.got.detach().cpu().contiguous().reshape(-1)
            assert ga.dtype == gb.dtype and torch.equal(ga.view(torch.uint8), gb.view(torch.uint8)), \
                f"{case.name}: {a.label} differs between the natural and the minimal alignment"
