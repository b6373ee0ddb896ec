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

Guarded.ranges lays several ragged ranges out in one flat payload -- range i occupies [starts[i],
starts[i] + lengths[i]), everything between them is gap -- and exposes each range's pointer, so
that a device descriptor table (vd_adam_desc, vd_ema_desc, vd_grad_desc) can point into it.
Guarded.flat is one such range: a contiguous tensor that starts `off` elements into the payload,
for a pointer that is element-aligned but not 16-byte aligned.  assert_finite is the value check
by buffer and offset for operands the element-wise bounds do not cover.

assert_clean(outputs, inputs) is the check after a call: every output fully written, its guards
and gaps bit-intact; every input (guards, gaps and payload) bit-identical to its snapshot.  A
buffer that is both read and written (p, m, v, an EMA shadow, a clipped gradient, x0_hist, x_prev
aliased to xt) goes into `inouts`: its guards and gaps must be bit-identical to the snapshot
taken when it was frozen, and its payload is the value check's business.
(fp32 arithmetic hands a NaN operand's payload on, so a pattern NaN read from an fp32 buffer that
leaks into an fp32 output can arrive there bit for bit and is then reported as "unwritten"; in
every other combination it fails the value check as a NaN.  Either way the call is red.)
"""
import torch

GUARD = 1 << 20
ALIGN = 256
# quiet NaNs (exponent all ones, top mantissa bit set) with a recognisable payload; as the signed
# integers the checks compare
PATTERN = {torch.float32: 0x7FC0DEAD, torch.bfloat16: 0x7FD5, torch.uint8: 0xFF,
           # integer operands (timesteps, step counts, window tables): far outside every table
           torch.int32: 0x7FC0DEAD, torch.int64: 0x7FC0DEAD7FC0DEAD}
_INT = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.uint8: torch.uint8,
        torch.int32: torch.int32, torch.int64: torch.int64}


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
    def ranges(cls, lengths, starts, dtype, device, data=None, name="buffer", span=None):
        """A flat payload in which range i is [starts[i], starts[i] + lengths[i]) (elements, in
        ascending order, not overlapping); the rest of the payload is gap.  .t is the whole flat
        payload; .range(i) the view of range i, .range_ptr(i) its address.  `data`: one tensor per
        range (the buffer is then frozen as an input), or None for pattern-filled ranges."""
        lengths, starts = [int(n) for n in lengths], [int(s) for s in starts]
        assert len(lengths) == len(starts) and all(n > 0 for n in lengths)
        end = 0
        for s_, n in zip(starts, lengths):
            assert s_ >= end, "ranges overlap or are not ascending"
            end = s_ + n
        g = cls((end if span is None else int(span),), dtype, device, name=name)
        assert g.span >= end
        g.starts, g.lengths = starts, lengths
        cover = torch.zeros(g.span, dtype=torch.bool)
        for s_, n in zip(starts, lengths):
            cover[s_:s_ + n] = True
        g._cover = cover.to(device)
        g._gap = ~g._cover if not bool(cover.all()) else None
        if data is not None:
            assert len(data) == len(lengths)
            for i, d in enumerate(data):
                g.range(i).copy_(d.reshape(-1))
            g.freeze()
        return g

    @classmethod
    def flat(cls, shape, dtype, device, data=None, off=0, name="buffer"):
        """A contiguous tensor of `shape` that starts `off` elements into the payload (off = 1: a
        pointer that is element-aligned but not 16-byte aligned; the elements before it are gap).
        .p is its address and .value() its content, as fp32 on the CPU."""
        shape = tuple(int(s) for s in shape)
        n = 1
        for s_ in shape:
            n *= s_
        g = cls.ranges([n], [off], dtype, device, None if data is None else [data], name=name)
        g.p, g.logical = g.range_ptr(0), shape
        return g

    def value(self):
        v = self.range_payloads()[0]
        return (v.float() if v.is_floating_point() else v).reshape(self.logical)

    def range(self, i):
        return self.t[self.starts[i]:self.starts[i] + self.lengths[i]]

    def range_ptr(self, i):
        return self.ptr + self.starts[i] * self.t.element_size()

    def range_payloads(self):
        """Every range copied out to a CPU tensor."""
        flat = self.t.detach().cpu()
        return [flat[s_:s_ + n].clone() for s_, n in zip(self.starts, self.lengths)]

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
        """Mask, in the shape of .t, of the elements that still hold the pattern (of a ranges
        layout: the elements of the ranges; the gaps are the gap check's)."""
        u = self._int == self._pat()
        cover = getattr(self, "_cover", None)
        return u if cover is None else u & cover

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

    def _first_frame_change(self):
        """As _first_change, for a buffer read and written in place: guards and gaps only."""
        assert self._snap is not None, f"{self.name}: freeze() an in-place operand before the call"
        bad = self.raw != self._snap
        if self._gap is None:
            bad[self.off:self.end] = False
        else:
            bad[self.off:self.end] &= self._gap
        return int(bad.nonzero()[0]) - self.off if bool(bad.any()) else None

    def payload(self):
        """The view copied out to a contiguous CPU tensor of the buffer's dtype."""
        return self.t.detach().cpu().contiguous()


def assert_clean(outputs=(), inputs=(), scratch=(), what="", inouts=()):
    """After a call (synchronizes when a buffer lives on a GPU).  Outputs: guards intact, gaps
    intact, nothing unwritten.  Inputs: guards, gaps and payload bit-identical to the snapshot.
    Scratch (workspaces, whose content is the kernel's own business): guards intact.
    Inouts (read and written in place; frozen before the call): guards and gaps bit-identical to
    the snapshot, the payload left to the value check.
    The message names the buffer and the first offending offset, in elements from the start of
    the payload (negative: in the front guard)."""
    every = tuple(outputs) + tuple(inputs) + tuple(scratch) + tuple(inouts)
    if any(g.raw.is_cuda for g in every):
        torch.cuda.synchronize()
    for g in inouts:
        o = g._first_frame_change()
        if o is not None:
            where = "gap" if 0 <= o < g.span else "guard"
            raise AssertionError(f"{what}: {g.name}: {where} written at payload offset {o} "
                                 f"(payload is {g.span} elements)")
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


def assert_finite(buffers, what=""):
    """The value check every guarded test ends with, by buffer and offset: no element of a
    written buffer (of a ranges layout: of its ranges) is NaN or infinite.  A pattern NaN read
    from a guard, a gap or a stale workspace slot that reached the buffer through arithmetic is
    found here, whatever bits it arrived with."""
    for g in buffers:
        bad = ~torch.isfinite(g.t.float())
        cover = getattr(g, "_cover", None)
        if cover is not None:
            bad &= cover
        if bool(bad.any()):
            idx = tuple(int(i) for i in bad.nonzero()[0])
            o = sum(i * s for i, s in zip(idx, g.strides))
            raise AssertionError(f"{what}: {g.name}: {int(bad.sum())} non-finite elements, first "
                                 f"at {idx} (payload offset {o})")
