"""Small assembler-text toolkit for the hand-scheduled gfx950 kernels (attn_asm.s).

The hot loops of the head_dim-64 attention kernels are emitted as explicit instruction
streams: MFMAs in a fixed order, with the softmax VALU work and the LDS fragment reads
placed into the gaps between them by position (MI355X_MICROARCH.md: per
v_mfma_f32_32x32x16_bf16 gap one wave can hide about 24 cycles of vector issue).  This
module provides
  * `Regs`  -- named register ranges (VGPR / AGPR / SGPR);
  * `Stream` -- an instruction list that tracks the wait-state hazards gfx950 does not
    interlock and pads them with s_nop, and derives the counted lgkmcnt waits of every
    consumer of an LDS read;
  * the pieces every kernel's generator shares (tile swizzle and lane-table entries, prologue
    sequences, LDS-DMA issue, the cost-driven VALU gap scheduler `place`);
  * `kernel_text` -- the code object wrapper (.amdhsa_kernel descriptor + metadata).

Hazard distances (gfx950; measured from hipcc's own padding of the same instruction pairs, the
store-data rule from LLVM's hazard recognizer -- a VALU write of the data VGPRs of a VMEM store
wider than 64 bits needs 2 wait states between them on gfx940+):
MFMA 32x32x16 write -> VALU / VMEM / DS / MFMA-A/B read 12 wait states (16x16x32: 8); VALU write -> MFMA
read 2; transcendental write -> VALU read 2 (one instruction between); an MFMA reading its
own accumulator chain as srcC needs none.  Wait states are counted as issued instructions
(s_nop n = n + 1), which under-counts the cycles an MFMA occupies, so the padding is
conservative.
"""
from __future__ import annotations

import re


class Regs:
    """Named register ranges in one file ('v', 'a' or 's')."""

    def __init__(self, kind: str, start: int = 0):
        self.kind, self.next, self.names = kind, start, {}

    def alloc(self, name: str, n: int, align: int = 1) -> int:
        if self.next % align:
            self.next += align - self.next % align
        base = self.next
        self.names[name] = (base, n)
        self.next += n
        return base

    def __getitem__(self, name):
        return self.names[name][0]

    def r(self, name, off=0, n=1) -> str:
        b, size = self.names[name]
        assert off + n <= size, (name, off, n, size)
        return reg(self.kind, b + off, n)


def reg(kind: str, i: int, n: int = 1) -> str:
    return f"{kind}{i}" if n == 1 else f"{kind}[{i}:{i + n - 1}]"


_RANGE = re.compile(r"\b([vas])\[(\d+):(\d+)\]|\b([vas])(\d+)\b")


def regs_of(text: str) -> set:
    """Physical registers named in an operand string: {('v', 12), ('a', 3), ...}."""
    out = set()
    for m in _RANGE.finditer(text):
        if m.group(1):
            k, lo, hi = m.group(1), int(m.group(2)), int(m.group(3))
            out.update((k, i) for i in range(lo, hi + 1))
        else:
            out.add((m.group(4), int(m.group(5))))
    return out


def classify(op: str) -> str:
    if op.startswith("v_mfma"):
        return "mfma"
    if op in ("v_exp_f32", "v_log_f32", "v_rcp_f32", "v_rsq_f32", "v_sqrt_f32"):
        return "trans"
    if op.startswith("v_"):
        return "valu"
    if op.startswith("ds_"):
        return "ds"
    if op.startswith(("buffer_", "global_")):
        return "vmem"
    return "salu"


class Ins:
    __slots__ = ("text", "op", "kind", "defs", "uses", "srcc", "lds_id", "wait_lds", "sdata")

    def __init__(self, text, lds_id=None, wait_lds=()):
        self.text = text.strip()
        self.op = self.text.split()[0]
        self.kind = classify(self.op)
        ops = self.text[len(self.op):].split(",")
        ops = [o.strip() for o in ops]
        self.srcc = set()
        self.sdata = set()   # data VGPRs of a store wider than 64 bits
        if self.kind in ("mfma", "trans", "valu"):
            self.defs = regs_of(ops[0]) if ops and ops[0] else set()
            self.uses = set().union(*[regs_of(o) for o in ops[1:]]) if len(ops) > 1 else set()
            if self.kind == "mfma" and len(ops) >= 4:
                self.srcc = regs_of(ops[3])
        elif self.kind == "ds":
            if self.op.startswith("ds_read"):
                self.defs, self.uses = regs_of(ops[0]), regs_of(ops[1].split()[0])
            else:
                self.defs, self.uses = set(), set().union(*[regs_of(o.split()[0]) for o in ops])
        elif self.kind == "vmem":
            if "lds" in self.text.split() or self.op.startswith(("buffer_store", "global_store")):
                self.defs, self.uses = set(), set().union(*[regs_of(o.split()[0]) for o in ops])
                if self.op.endswith(("_dwordx3", "_dwordx4", "_b96", "_b128")) and \
                        "lds" not in self.text.split():
                    self.sdata = regs_of(ops[0].split()[0])
            else:
                self.defs = regs_of(ops[0])
                self.uses = set().union(*[regs_of(o.split()[0]) for o in ops[1:]])
        else:
            self.defs, self.uses = set(), set()
        self.lds_id = lds_id          # id of this LDS read (for counted waits)
        self.wait_lds = tuple(wait_lds)  # LDS read ids this instruction consumes


class Stream:
    """Straight-line instruction stream with hazard padding and counted lgkmcnt waits.

    Every ds_read must carry an lds_id; an instruction that consumes LDS-read results names
    them in wait_lds and gets the weakest `s_waitcnt lgkmcnt(k)` that covers them (reads
    complete in issue order).  Call `flush_lds()` to forget outstanding reads (after an
    explicit lgkmcnt(0))."""

    MFMA_RAW = 12      # MFMA write -> VALU / VMEM / DS / MFMA A-B read (and write)
    MFMA16_RAW = 8     # ... of a 16x16 (4-pass) MFMA (hipcc: s_nop 7 before the VALU read)
    VALU_TO_MFMA = 2   # VALU write -> MFMA read
    TRANS_RAW = 2      # transcendental write -> VALU read
    MFMA_WAR = 12      # VALU write of an in-flight MFMA's source
    STORE_DATA = 3     # VALU write of the data VGPRs of a VMEM store wider than 64 bits:
                       # 2 wait states between them (gfx940+, LLVM GCNHazardRecognizer; the
                       # distances here count the producing instruction itself)

    def __init__(self):
        self.lines = []
        self.hist = []        # (position, Ins) of the hazard-relevant recent instructions
        self.pos = 0          # wait states issued so far
        self.pending = []     # outstanding LDS read ids, issue order
        self.nops = 0
        self.waits = 0
        self.forced = 0   # waits forced by the 15-read limit
        self.young = 0    # ... of which waited on a read issued < 4 MFMAs earlier (a stall)
        self.nmfma = 0
        self.issued_at = {}

    def comment(self, text):
        self.lines.append(f"\t; {text}")

    def label(self, name):
        self.lines.append(f"{name}:")

    def raw(self, text, ws=1):
        """An instruction outside the hazard model (branches, barriers, SALU)."""
        self.lines.append("\t" + text)
        self.pos += ws

    def _need(self, ins: Ins) -> int:
        need = 0
        for p, h in reversed(self.hist):
            d = self.pos - p
            if d >= 13:
                break
            if h.kind == "mfma":
                raw = self.MFMA16_RAW if "_16x16x" in h.op else self.MFMA_RAW
                if ins.kind == "mfma":
                    # chained accumulator (srcC == the producer's dst) needs no padding
                    touched = (ins.uses - ins.srcc) & h.defs
                    if touched:
                        need = max(need, raw - d)
                elif (ins.uses | ins.defs) & h.defs:
                    need = max(need, raw - d)
                if ins.kind in ("valu", "trans", "ds", "vmem") and ins.defs & (h.uses | h.srcc):
                    need = max(need, self.MFMA_WAR - d)
            elif h.kind == "vmem":
                if ins.kind in ("valu", "trans") and ins.defs & h.sdata:
                    need = max(need, self.STORE_DATA - d)
            elif h.kind in ("valu", "trans"):
                if ins.kind == "mfma" and (ins.uses | ins.defs) & h.defs:
                    need = max(need, self.VALU_TO_MFMA - d)
                if h.kind == "trans" and ins.kind in ("valu", "trans", "vmem", "ds") \
                        and ins.uses & h.defs:
                    need = max(need, self.TRANS_RAW - d)
        return need

    def emit(self, text, lds_id=None, wait_lds=()):
        ins = Ins(text, lds_id, wait_lds)
        if ins.lds_id is not None and len(self.pending) >= 15:
            # lgkmcnt is a 4-bit counter: keep at most 15 LDS reads outstanding
            k = 14
            young = self.nmfma - self.issued_at.get(self.pending[0], -99) < 4
            self.young += young
            self.lines.append(f"\ts_waitcnt lgkmcnt({k})  ; forced: 15 reads in flight"
                              + (" (young)" if young else ""))
            self.pending = self.pending[len(self.pending) - k:]
            self.pos += 1
            self.waits += 1
            self.forced += 1
        if ins.wait_lds:
            idx = [self.pending.index(i) for i in ins.wait_lds if i in self.pending]
            if idx:
                k = len(self.pending) - 1 - max(idx)
                self.lines.append(f"\ts_waitcnt lgkmcnt({min(k, 15)})")
                self.pending = self.pending[max(idx) + 1:]
                self.pos += 1
                self.waits += 1
        need = self._need(ins)
        while need > 0:
            n = min(need, 16)
            self.lines.append(f"\ts_nop {n - 1}")
            self.pos += n
            self.nops += n
            need -= n
        self.lines.append("\t" + ins.text)
        if ins.lds_id is not None:
            self.pending.append(ins.lds_id)
            self.issued_at[ins.lds_id] = self.nmfma
        if ins.kind == "mfma":
            self.nmfma += 1
        if ins.kind in ("mfma", "valu", "trans") or ins.sdata:
            self.hist.append((self.pos, ins))
            if len(self.hist) > 64:
                self.hist = self.hist[-64:]
        self.pos += 1
        return ins

    def flush_lds(self):
        self.pending = []

    def text(self):
        return "\n".join(self.lines) + "\n"


# ------------------------------------------------------------------ shared kernel pieces
# Plain functions over a Stream and register names.  Each emits the same instruction
# sequence for every kernel that uses it; the generators keep only what is theirs (register
# plan, SGPR map, MFMA order, VALU lists, slot tables).
HI = 65536             # ds_read immediates are 16 bits: offsets >= 64 KiB use +64 KiB bases
COST = {"exp": 8.0, "add": 4.0, "cvt": 4.5, "cmp": 4.0, "cnd": 4.0}   # VALU issue cycles


def _first(rng: str) -> int:
    """First register number of 's[60:63]' / 's60'."""
    return int(rng.strip("s[]").split(":")[0])


def swz(d, r):
    """attention.hip swz_row<d>: the 16-B chunk XOR of row r of a bf16 tile with d-element rows
    (d = 64, or 128 / 256 which share one rule)."""
    if d == 64:
        return (((r >> 1) & 1) << 2) | ((r >> 2) & 3)
    return ((r & 3) << 2) | ((r >> 2) & 3)


def toff_bytes(d, r, c):
    """attention.hip toff<bf16, d>(r, c) in bytes."""
    return 2 * (r * d + (((c >> 3) ^ swz(d, r)) << 3) + (c & 7))


def frag_offsets(d, lane, nrow, ntr):
    """A lane's table entries for a bf16 tile with d-element rows: the nrow row-fragment
    offsets (attention.hip mma_rows: k-step s, block row 0), then the 2 ntr transposed-fragment
    offsets (mma_tr: 2 i + hi, column block i, rows +8 hi; col0 = 32 i, sum0 = 0, s2 = 0)."""
    r, hh = lane & 31, lane >> 5
    out = [toff_bytes(d, r, 16 * s + 8 * hh) for s in range(nrow)]
    g, fr = lane >> 4, lane & 15
    q4, p4 = fr >> 2, fr & 3
    for i in range(ntr):
        col = 32 * i + 16 * (g & 1) + 4 * p4
        kr = 4 * (g >> 1) + q4
        out += [toff_bytes(d, kr, col), toff_bytes(d, kr + 8, col)]
    return out


def m16_chunk(ks, g):
    """attention.hip m16_chunk: the 16-B chunk of a row that contraction slot group (ks, g) of a
    v_mfma_f32_16x16x32_bf16 operand over head_dim holds (g = lane >> 4)."""
    return 4 * ks + g


def m16_row(it, i):
    """attention.hip m16_row: the row (of a 32-row block) that MFMA row i of row tile `it` of a
    16x16x32 A operand reads; accumulator rows 4 g .. 4 g + 3 are rows m16_row(it, 4 g) .. + 3."""
    return 16 * (i >> 3) + 4 * ((i >> 2) & 1) + 8 * it + (i & 3)


def frag_offsets16(d, lane):
    """A lane's table entries for the 16x16x32 reads of a bf16 tile with d-element rows: the 4
    row-fragment offsets (attention.hip mma_rows_nb<M16>: 2 it + ks, block row 0), then the 8
    transposed-fragment offsets (mma_tr_nb<M16>: 2 dt + hi, 16-column tile dt of the tile's 64
    columns, low / high half of the contraction group; sum0 = 0)."""
    i, g = lane & 15, lane >> 4
    out = [toff_bytes(d, m16_row(it, i), 8 * m16_chunk(ks, g))
           for it in range(2) for ks in range(2)]
    q4, p4 = i >> 2, i & 3
    out += [toff_bytes(d, m16_row(hi, 4 * g) + q4, 16 * dt + 4 * p4)
            for dt in range(4) for hi in range(2)]
    return out


def lds(V, name, k, off):
    """(base register, immediate) of LDS byte offset `off` from per-lane table entry k of
    `name` ('rowoff' / 'troff'; their +64 KiB copies are 'rowhi' / 'trhi')."""
    if off >= HI:
        return V.r({"rowoff": "rowhi", "troff": "trhi"}[name], k), off - HI
    return V.r(name, k), off


def lane_table_data(symbol, rows):
    """The .rodata text of a per-lane u32 table."""
    data = f"\n.rodata\n.p2align 8\n{symbol}:\n"
    for row in rows:
        data += "\t.long " + ", ".join(str(x) for x in row) + "\n"
    return data


def wave_id(st, V, s_wave):
    """lane = tid & 63 ; s_wave = the wave's index in the workgroup."""
    st.emit(f"v_and_b32 {V.r('lane')}, 63, {V.r('tid')}")
    st.raw(f"v_readfirstlane_b32 {s_wave}, {V.r('tid')}")  # first lane's id = 64 * wave
    st.raw("s_nop 1")
    st.raw(f"s_lshr_b32 {s_wave}, {s_wave}, 6")


def table_addr(st, s_tab, symbol):
    """s_tab (an aligned pair) = the address of the lane table `symbol`."""
    lo = _first(s_tab)
    st.raw(f"s_getpc_b64 s[{lo}:{lo + 1}]")
    st.raw(f"s_add_u32 s{lo}, s{lo}, {symbol}@rel32@lo+4")
    st.raw(f"s_addc_u32 s{lo + 1}, s{lo + 1}, {symbol}@rel32@hi+12")


def wave_and_table(st, V, s_wave, s_tab, symbol):
    wave_id(st, V, s_wave)
    table_addr(st, s_tab, symbol)


def rare_targets(st, s_tgt, prefix):
    """s[s_tgt + 2 v : +1] = the rare-path entry point .L{prefix}_rare{v}, v = 0..3."""
    st.raw(f"s_getpc_b64 s[{s_tgt}:{s_tgt + 1}]")
    st.label(f".L{prefix}_pc")
    for v in (3, 2, 1, 0):
        st.raw(f"s_add_u32 s{s_tgt + 2 * v}, s{s_tgt}, .L{prefix}_rare{v}-.L{prefix}_pc")
        st.raw(f"s_addc_u32 s{s_tgt + 2 * v + 1}, s{s_tgt + 1}, 0")


def mad64(st, dlo, dhi, a, blo, bhi, t):
    """dhi:dlo = a * bhi:blo (low 64 bits); t is scratch."""
    st.raw(f"s_mul_i32 {dlo}, {a}, {blo}")
    st.raw(f"s_mul_hi_u32 {dhi}, {a}, {blo}")
    st.raw(f"s_mul_i32 {t}, {a}, {bhi}")
    st.raw(f"s_add_u32 {dhi}, {dhi}, {t}")


def add64(st, dlo, dhi, alo, ahi):
    """dhi:dlo += ahi:alo."""
    st.raw(f"s_add_u32 {dlo}, {dlo}, {alo}")
    st.raw(f"s_addc_u32 {dhi}, {dhi}, {ahi}")


def rsrc(st, dst, plo, phi, nrec, base):
    """Buffer resource dst (4 SGPRs) over nrec bytes from pointer phi:plo + base (a (lo, hi)
    SGPR pair): 48-bit address, stride 0, raw dword format (0x20000)."""
    d0 = _first(dst)
    st.raw(f"s_add_u32 s{d0}, {plo}, {base[0]}")
    st.raw(f"s_addc_u32 s{d0 + 1}, {phi}, {base[1]}")
    st.raw(f"s_and_b32 s{d0 + 1}, s{d0 + 1}, 0xffff")
    st.raw(f"s_mov_b32 s{d0 + 2}, {nrec}")
    st.raw(f"s_mov_b32 s{d0 + 3}, 0x20000")


def scale_bf16(st, v0, n, s_scale, t0, t1, dst):
    """v[v0 .. v0 + n) *= s_scale per bf16 element (attention.hip RowFrag::scale), each word
    then copied to the AGPR dst(w)."""
    e = st.emit
    for w in range(n):
        x = f"v{v0 + w}"
        e(f"v_lshlrev_b32 {t0}, 16, {x}")
        e(f"v_and_b32 {t1}, 0xffff0000, {x}")
        e(f"v_mul_f32 {t0}, {s_scale}, {t0}")
        e(f"v_mul_f32 {t1}, {s_scale}, {t1}")
        e(f"v_cvt_pk_bf16_f32 {x}, {t0}, {t1}")
        e(f"v_accvgpr_write_b32 {dst(w)}, {x}")


def dma_issue(st, ops, adv=()):
    """LDS-DMA pieces ops = [(M0 setup, buffer_load ... lds)], then the source-offset
    advances adv (after a tile's last piece)."""
    for m0, ld in ops:
        st.raw(m0)
        st.raw("s_nop 0")
        st.emit(ld)
    for a in adv:
        st.emit(a)


def dma_at_gap(st, g, gaps, ops, adv):
    """Inside a body: the piece whose gap is g (gaps[i] holds ops[i]), if any; the last one is
    followed by adv."""
    if g in gaps:
        i = gaps.index(g)
        dma_issue(st, ops[i:i + 1], adv if i == len(gaps) - 1 else ())


def loop_tail(st, s_iter, label):
    st.raw(f"s_sub_u32 {s_iter}, {s_iter}, 1")
    st.raw(f"s_cmp_lg_u32 {s_iter}, 0")
    st.raw(f"s_cbranch_scc1 {label}")


def combine_list(V, chains):
    """The `chains` row-sum accumulators of each query block into ps (a pairwise tree), as
    softmax items (text, cost, earliest gap)."""
    out = []
    if chains == 1:
        return [(f"v_mov_b32 {V.r('ps', j)}, {V.r('c', 4 * j)}", COST["add"], 0)
                for j in range(2)]
    step = 1
    while step < chains:
        last = 2 * step >= chains
        for a in range(0, chains, 2 * step):
            for j in range(2):
                dst = V.r("ps", j) if last else V.r("c", 4 * j + a)
                out.append((f"v_add_f32 {dst}, {V.r('c', 4 * j + a)}, "
                            f"{V.r('c', 4 * j + a + step)}", COST["add"], 0))
        step *= 2
    return out


def place(items, ngaps):
    """Greedy list schedule of VALU items (text, cost) or (text, cost, earliest gap; default 0)
    over ngaps MFMA gaps: gap g takes, in list order, the items whose earliest gap has come,
    until the gap's share of the total cost is used; an item held back by its earliest gap
    lets the later ones pass (only P^T writes are held back); the last gap takes the rest."""
    per = sum(it[1] for it in items) / ngaps
    slots = [[] for _ in range(ngaps)]
    done = [False] * len(items)
    budget = 0.0
    for g in range(ngaps):
        budget += per
        last = g == ngaps - 1
        for k, it in enumerate(items):
            if done[k] or (len(it) > 2 and it[2] > g):
                continue
            if not last and it[1] > budget + 1e-9:
                break
            slots[g].append(it[0])
            budget -= it[1]
            done[k] = True
    assert all(done)
    return slots


# Code placement (MI355X_MICROARCH.md "Two waves per SIMD" item 8: a hand-written stream can
# lose ~13 % under a uniform 4-byte shift).  Measured and removed: a per-kernel 4-byte phase
# shift (one leading s_nop 0) left all nine kernels within +-0.5 %
# (profiles/r04aj_ab_code_placement.txt, DESIGN_HISTORY.md "Code placement").  Nothing here
# reads the environment, so a leftover variable cannot shift the shipped code.
def kernel_text(name, body, *, vgprs, agprs, sgprs, lds_bytes, kernarg_bytes, wg_size,
                wg_ids=(1, 1, 1)):
    """(code + descriptor text, metadata entry) of one kernel (code object v5)."""
    accum = (vgprs + 3) // 4 * 4
    total = accum + agprs
    assert total <= 512, total
    code = f""".text
.globl {name}
.p2align 8
.type {name},@function
{name}:
{body}
\ts_endpgm
.Lfunc_end_{name}:
.size {name}, .Lfunc_end_{name}-{name}

.rodata
.p2align 6
.amdhsa_kernel {name}
  .amdhsa_group_segment_fixed_size {lds_bytes}
  .amdhsa_private_segment_fixed_size 0
  .amdhsa_kernarg_size {kernarg_bytes}
  .amdhsa_user_sgpr_count 2
  .amdhsa_user_sgpr_kernarg_segment_ptr 1
  .amdhsa_system_sgpr_workgroup_id_x {wg_ids[0]}
  .amdhsa_system_sgpr_workgroup_id_y {wg_ids[1]}
  .amdhsa_system_sgpr_workgroup_id_z {wg_ids[2]}
  .amdhsa_system_vgpr_workitem_id 0
  .amdhsa_next_free_vgpr {total}
  .amdhsa_next_free_sgpr {sgprs}
  .amdhsa_accum_offset {accum}
  .amdhsa_reserve_vcc 1
  .amdhsa_float_denorm_mode_32 3
  .amdhsa_float_denorm_mode_16_64 3
  .amdhsa_ieee_mode 1
  .amdhsa_dx10_clamp 1
.end_amdhsa_kernel
"""
    meta = f"""  - .name: {name}
    .symbol: {name}.kd
    .kernarg_segment_size: {kernarg_bytes}
    .group_segment_fixed_size: {lds_bytes}
    .private_segment_fixed_size: 0
    .kernarg_segment_align: 8
    .wavefront_size: 64
    .sgpr_count: {sgprs + 6}
    .vgpr_count: {total}
    .agpr_count: {agprs}
    .max_flat_workgroup_size: {wg_size}
    .args:
      - {{ .offset: 0, .size: {kernarg_bytes}, .value_kind: by_value }}
"""
    return code, meta


def code_object_text(kernels, data=""):
    """One .s holding several kernels: kernels = [(code, meta)], data = extra .rodata."""
    out = '.amdgcn_target "amdgcn-amd-amdhsa--gfx950"\n.amdhsa_code_object_version 5\n'
    out += "".join(c for c, _ in kernels)
    out += data
    out += "\n.amdgpu_metadata\n---\namdhsa.version: [ 1, 2 ]\namdhsa.kernels:\n"
    out += "".join(m for _, m in kernels)
    out += "...\n.end_amdgpu_metadata\n"
    return out
