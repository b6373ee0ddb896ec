"""Guard-band and NaN-poison buffers for kernel tests (CPU and GPU tensors).

A kernel test that takes its buffers from torch.empty cannot see a write outside the tensor (it
lands in allocator slack or in a neighbour nobody compares), a read outside the tensor whose
value reaches an output (it passes while the neighbouring memory holds finite numbers), or an
output documented as OVERWRITTEN that is only partly written (fresh memory is usually zero).

`Guarded` owns one allocation laid out as [guard | payload | guard]:
  - each guard is GUARD = 1 MiB (the size tools/guardalloc uses): larger than any tile a kernel
    here addresses, so an overrun of the kind the kernels' comments describe lands inside the
    test's own allocation;
  - the payload starts 256-byte aligned;
  - the whole allocation is first filled with one quiet-NaN bit pattern per dtype (PATTERN; byte
    0xFF for workspaces), then `data` is copied into the payload.  All checks compare the
    pattern as integers, never as floats.
A strided payload (pixel stride > C of a channels-last tensor, batch stride > N * row of an
attention buffer) is a view `.t` of given shape and strides into a flat payload of `span`
elements; the elements of the payload the view does not cover are the gaps.  They hold the
pattern too: NaN under an input, and they must stay bit-intact under an output.

assert_clean(outputs, inputs) is the check after a call: every output fully written, its guards
and gaps bit-intact; every input (guards, gaps and payload) bit-identical to its snapshot.
(fp32 arithmetic hands a NaN operand's payload on, so a pattern NaN read from an fp32 buffer that
leaks into an fp32 output can arrive there bit for bit and is then reported as "unwritten"; in
every other combination it fails the value check as a NaN.  Either way the call is red.)
"""
import torch

GUARD = 1 << 20
ALIGN = 256
# quiet NaNs (exponent all ones, top mantissa bit set) with a recognisable payload; as the signed
# integers the checks compare
PATTERN = {torch.float32: 0x7FC0DEAD, torch.bfloat16: 0x7FD5, torch.uint8: 0xFF}
_INT = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.uint8: torch.uint8}


class Guarded:
    def __init__(self, shape, dtype, device, data=None, strides=None, span=None, name="buffer"):
        """`shape` elements of `dtype`; `strides` (elements, default contiguous) and `span` (the
        payload's length in elements, default the view's extent) describe a layout with gaps.
        `data` (any dtype / device, broadcastable to `shape`) is copied into the view and the
        buffer is frozen as an input; without it the view holds the pattern."""
        self.name, self.dtype, self.shape = name, dtype, tuple(int(s) for s in shape)
        it = _INT[dtype]
        es = torch.empty(0, dtype=dtype).element_size()
        if strides is None:
            strides, acc = [], 1
            for s in reversed(self.shape):
                strides.insert(0, acc)
                acc *= s
        self.strides = tuple(int(s) for s in strides)
        numel = 1
        for s in self.shape:
            numel *= s
        extent = 0 if numel == 0 else 1 + sum((n - 1) * s for n, s in zip(self.shape, self.strides))
        self.span = extent if span is None else int(span)
        assert self.span >= extent, (self.span, extent)
        ge = GUARD // es
        slack = ALIGN // es
        self.raw = torch.full((ge + slack + self.span + ge,), PATTERN[dtype], dtype=it,
                              device=device)
        base = self.raw.data_ptr()
        assert base % es == 0
        self.off = ge + ((-(base + GUARD)) % ALIGN) // es       # payload start, in elements
        self.end = self.off + self.span
        self.ptr = base + self.off * es
        assert self.ptr % ALIGN == 0 and self.raw.numel() - self.end >= ge
        self._flat_int = self.raw[self.off:self.end]
        self._int = torch.as_strided(self.raw, self.shape, self.strides, self.off)
        self.t = torch.as_strided(self.raw.view(dtype), self.shape, self.strides, self.off)
        self._gap = None
        if self.span != numel:
            cover = torch.zeros(self.span, dtype=torch.bool, device=device)
            torch.as_strided(cover, self.shape, self.strides).fill_(True)
            assert int(cover.sum()) == numel, "overlapping strides"
            self._gap = ~cover
        self._snap = None
        if data is not None:
            self.t.copy_(data)
            self.freeze()

    # ------------------------------------------------------------------ layouts
    @classmethod
    def cl(cls, shape, dtype, device, data=None, cstride=0, name="buffer"):
        """Channels-last [B, C, *spatial] (the layout of vdiff.ops: .t is the logical tensor, C
        fastest in memory) with `cstride` elements between pixels (0 = C); the last pixel's gap
        lanes belong to the payload."""
        shape = [int(s) for s in shape]
        C, cs = shape[1], int(cstride) or shape[1]
        assert cs >= C
        phys = [shape[0]] + shape[2:]
        st, acc = [], cs
        for n in reversed(phys):
            st.insert(0, acc)
            acc *= n
        strides = [st[0], 1] + st[1:]
        return cls(shape, dtype, device, data, strides, acc, name)

    @classmethod
    def rows(cls, nb, n, row, dtype, device, data=None, pad_rows=0, name="buffer"):
        """[nb][n + pad_rows][row] with .t the [nb, n, row] view: every batch is followed by
        pad_rows gap rows (batch stride (n + pad_rows) * row)."""
        return cls((nb, n, row), dtype, device, data, ((n + pad_rows) * row, row, 1),
                   nb * (n + pad_rows) * row, name)

    @classmethod
    def workspace(cls, nbytes, device, name="workspace"):
        """Exactly nbytes of 0xFF (stale NaN in every float format) inside intact guards."""
        return cls((int(nbytes),), torch.uint8, device, name=name)

    # ------------------------------------------------------------------ checks
    def _pat(self):
        return PATTERN[self.dtype]

    def _first_guard_fault(self):
        """Offset, in elements relative to the payload, of the first changed guard element."""
        front = self.raw[:self.off] != self._pat()
        if bool(front.any()):
            return int(front.nonzero()[0]) - self.off
        back = self.raw[self.end:] != self._pat()
        if bool(back.any()):
            return int(back.nonzero()[0]) + self.span
        return None

    def guards_intact(self):
        return self._first_guard_fault() is None

    def unwritten(self):
        """Mask, in the shape of .t, of the elements that still hold the pattern."""
        return self._int == self._pat()

    def _first_gap_fault(self):
        if self._gap is None:
            return None
        bad = (self._flat_int != self._pat()) & self._gap
        return int(bad.nonzero()[0]) if bool(bad.any()) else None

    def gaps_intact(self):
        return self._first_gap_fault() is None

    def freeze(self):
        """Snapshot of the whole allocation: from now on the buffer is an input."""
        self._snap = self.raw.clone()
        return self

    def _first_change(self):
        assert self._snap is not None, f"{self.name}: freeze() an input before the call"
        bad = self.raw != self._snap
        return int(bad.nonzero()[0]) - self.off if bool(bad.any()) else None

    def unchanged(self):
        return self._first_change() is None

    def payload(self):
        """The view copied out to a contiguous CPU tensor of the buffer's dtype."""
        return self.t.detach().cpu().contiguous()


def assert_clean(outputs=(), inputs=(), scratch=(), what=""):
    """After a call (synchronizes when a buffer lives on a GPU).  Outputs: guards intact, gaps
    intact, nothing unwritten.  Inputs: guards, gaps and payload bit-identical to the snapshot.
    Scratch (workspaces, whose content is the kernel's own business): guards intact.
    The message names the buffer and the first offending offset, in elements from the start of
    the payload (negative: in the front guard)."""
    if any(g.raw.is_cuda for g in tuple(outputs) + tuple(inputs) + tuple(scratch)):
        torch.cuda.synchronize()
    for g in scratch:
        o = g._first_guard_fault()
        assert o is None, f"{what}: {g.name}: guard written at payload offset {o} " \
                          f"(payload is {g.span} elements)"
    for g in outputs:
        o = g._first_guard_fault()
        assert o is None, f"{what}: {g.name}: guard written at payload offset {o} " \
                          f"(payload is {g.span} elements)"
        o = g._first_gap_fault()
        assert o is None, f"{what}: {g.name}: gap written at payload offset {o}"
        u = g.unwritten()
        if bool(u.any()):
            idx = tuple(int(i) for i in u.nonzero()[0])
            o = sum(i * s for i, s in zip(idx, g.strides))
            raise AssertionError(f"{what}: {g.name}: {int(u.sum())} of {u.numel()} elements "
                                 f"unwritten, first at {idx} (payload offset {o})")
    for g in inputs:
        o = g._first_change()
        assert o is None, f"{what}: {g.name}: input modified at payload offset {o}"
