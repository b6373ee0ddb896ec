"""CPU checks of the hand-scheduled kernel generators (csrc/asm/): the code object the
library embeds assembles for gfx950, every kernel fits the 512-entry register file at one
wave per SIMD, and each body's instruction mix is the one the generator documents (MFMAs
per tile, no padding nops inside the MFMA streams beyond the counted hazards).  No GPU."""
import os
import shutil
import subprocess
import sys

import pytest

from conftest import ROOT

ASM = os.path.join(ROOT, "lipreading-video-generation_amd", "csrc", "asm")
CLANG = "/opt/rocm/llvm/bin/clang"


@pytest.fixture(scope="module")
def gens():
    sys.path.insert(0, ASM)
    try:
        import gen_attn_asm as G
        import gen_d128 as D128
        import gen_fwd as F64
        import gen_fwd128 as F128
        import gen_d256 as D256
        import gen_d256dk as D256K
        yield G, F64, D128, F128, D256, D256K
    finally:
        sys.path.remove(ASM)


def test_code_object_assembles(tmp_path, gens):
    if not shutil.which(CLANG) and not os.path.exists(CLANG):
        pytest.skip("ROCm clang not present")
    out = tmp_path / "attn_asm.s"
    subprocess.run([sys.executable, os.path.join(ASM, "gen_attn_asm.py"), str(out)], check=True)
    text = out.read_text()
    for name in ("vd_attn_bwd_dq_d64", "vd_attn_bwd_dkdv_d64", "vd_attn_fwd_d64",
                 "vd_attn_bwd_dkdv_d128", "vd_attn_bwd_dq_d128", "vd_attn_fwd_d128",
                 "vd_attn_bwd_dq_d256", "vd_attn_bwd_dkdv_d256", "vd_attn_fwd_d256"):
        assert f".amdhsa_kernel {name}" in text, name
    subprocess.run([CLANG, "-x", "assembler", "-target", "amdgcn-amd-amdhsa", "-mcpu=gfx950",
                    "-c", str(out), "-o", str(tmp_path / "a.o")], check=True)


def test_register_budgets(gens):
    G, F64, D128, F128, D256, D256K = gens
    for regs in (G.regs_dq, G.regs_dkdv, F64.regs, D128.regs, D128.dq_regs, F128.regs,
                 D256.regs, D256K.regs_a, D256K.regs_b):
        V, A = regs()
        assert V.next <= 256 and A.next <= 256, (regs, V.next, A.next)
        assert (V.next + 3) // 4 * 4 + A.next <= 512


def _body_counts(lines, start, stop):
    i0 = next(i for i, l in enumerate(lines) if start in l)
    i1 = next(i for i, l in enumerate(lines) if i > i0 and stop in l)
    ops = [l.split()[0] for l in lines[i0:i1] if l.strip() and not l.strip().startswith((";", "."))]
    return {k: ops.count(k) for k in set(ops)}


def test_instruction_mix_per_tile(gens):
    G, F64, D128, F128, D256, D256K = gens
    mf = "v_mfma_f32_32x32x16_bf16"
    _, _, st = D128.gen_dkdv128()
    c = _body_counts(st.lines, "query tile, ring stage 1", "query tile, ring stage 2")
    assert c[mf] == 64 and c["v_exp_f32"] == 32 and c["ds_read_b64_tr_b16"] == 64
    assert c["ds_read_b128"] == 48
    assert c["buffer_load_dwordx4"] == 8 and c["buffer_load_dword"] == 1
    _, st = D128.gen_dq128()
    c = _body_counts(st.lines, "key tile, ring stage 1", "key tile, ring stage 2")
    assert c[mf] == 48 and c["v_exp_f32"] == 32 and c["buffer_load_dwordx4"] == 8
    _, _, st = F128.gen_fwd128()
    c = _body_counts(st.lines, "body, stage 1", "body, stage 2")
    assert c[mf] == 32 and c["v_exp_f32"] == 32 and c["v_cvt_pk_bf16_f32"] == 16
    _, st = F64.gen_fwd()
    c = _body_counts(st.lines, "body, stage 1", "body, stage 2")
    assert c[mf] == 32 and c["v_exp_f32"] == 64 and c["v_cvt_pk_bf16_f32"] == 32
    assert c.get("s_nop", 0) <= 8
    # head_dim 256 (round 4): dQ 48 MFMAs per 32-key tile, 8 + 8 row / 32 transposed reads
    _, _, st = D256.gen_dq256()
    c = _body_counts(st.lines, "key tile, ring stage 1", "key tile, ring stage 2")
    assert c[mf] == 48 and c["v_exp_f32"] == 16 and c["v_cvt_pk_bf16_f32"] == 8
    assert c["ds_read_b128"] == 32 and c["ds_read_b64_tr_b16"] == 32
    assert c["buffer_load_dwordx4"] == 8 and c.get("s_nop", 0) <= 16
    # dK / dV role pairs: 32 MFMAs per 32-query tile in each role, 9 DMA ops
    _, _, st = D256K.gen_dkdv256()
    c = _body_counts(st.lines, "A: query tile, ring stage 1", "A: query tile, ring stage 2")
    assert c[mf] == 32 and c["v_exp_f32"] == 16 and c["ds_write_b128"] == 4
    assert c["buffer_load_dwordx4"] == 8 and c["buffer_load_dword"] == 1
    assert c.get("s_nop", 0) <= 20
    c = _body_counts(st.lines, "B: query tile, ring stage 1", "B: query tile, ring stage 2")
    assert c[mf] == 32 and c["v_mul_f32"] == 16 and c["ds_read_b128"] == 16 + 4 + 4
    assert c.get("s_nop", 0) <= 20


def test_fwd256_body(gens):
    """vd_attn_fwd_d256 (round 4): per 32-key tile 16 S + 16 PV MFMAs, the 16 exp / 8 cvt of
    the lagged softmax, 16 K row and 32 V^T transposed fragment reads, 8 LDS-DMA pieces, one
    rare-path call site; registers within one wave per SIMD; the 4 rare-path entry points."""
    import gen_fwd256 as F256
    V, A = F256.regs()
    assert V.next <= 256 and A.next <= 256 and (V.next + 3) // 4 * 4 + A.next <= 512
    k, st = F256.gen_fwd256()
    mf = "v_mfma_f32_32x32x16_bf16"
    c = _body_counts(st.lines, "key tile, ring stage 1", "key tile, ring stage 2")
    assert c[mf] == 32 and c["v_exp_f32"] == 16 and c["v_cvt_pk_bf16_f32"] == 8
    assert c["ds_read_b128"] == 16 and c["ds_read_b64_tr_b16"] == 32
    assert c["buffer_load_dwordx4"] == 8 and c["s_swappc_b64"] == 1
    assert c.get("s_nop", 0) <= 16
    for v in range(4):
        assert f".Lfwd256_rare{v}:" in k[0]


def test_d256_lane_tables(gens):
    """The head_dim-256 lane tables: 32 u32 per lane, the DMA pieces of the 4 waves (dQ) /
    2 pairs (dK/dV) cover every (row, 16-B chunk) of a 32-row tile exactly once."""
    G, F64, D128, F128, D256, D256K = gens
    t = D256.lane_table()
    assert len(t) == 256 and all(len(r) == 32 for r in t)
    seen = set()
    for w in range(4):
        for lane in range(64):
            for i in range(4):
                seen.add((t[64 * w + lane][16 + i], t[64 * w + lane][20 + i]))
    assert len(seen) == 32 * 32
    t = D256K.lane_table()
    seen = set()
    for w in range(2):  # pair 0 / 1 (waves 2, 3 repeat them for the dO tile)
        for lane in range(64):
            for i in range(8):
                seen.add((t[64 * w + lane][16 + i], t[64 * w + lane][24 + i]))
    assert len(seen) == 32 * 32


def test_stream_hazard_padding(gens):
    """asmgen.Stream pads the gfx950 wait-state hazards the generators rely on (round 4), as
    wait states inserted between back-to-back instructions: a 128-bit VMEM store's data VGPRs
    rewritten by a VALU op, 2 (LLVM's gfx940 rule; the D = 256 fp32 partial epilogues had
    none and lost the stores of lanes 12-15 of every 16); a v_mfma_f32_16x16x32_bf16 result
    read by VALU, 7; a 32x32x16 one, 11; a 64-bit store and an accumulator chain, none."""
    sys.path.insert(0, ASM)
    try:
        from asmgen import Stream
    finally:
        sys.path.remove(ASM)

    def nops(*lines):
        st = Stream()
        for ln in lines:
            st.emit(ln)
        return st.nops

    assert nops("buffer_store_dwordx4 v[0:3], v10, s[0:3], 0 offen",
                "v_accvgpr_read_b32 v0, a0") == 2
    assert nops("buffer_store_dwordx4 v[0:3], v10, s[0:3], 0 offen",
                "v_mov_b32 v9, 0", "v_accvgpr_read_b32 v0, a0") == 1
    assert nops("buffer_store_dwordx2 v[0:1], v10, s[0:3], 0 offen",
                "v_accvgpr_read_b32 v0, a0") == 0
    assert nops("buffer_store_dwordx4 v[0:3], v10, s[0:3], 0 offen",
                "v_accvgpr_read_b32 v4, a0") == 0
    assert nops("v_mfma_f32_16x16x32_bf16 a[0:3], v[0:3], v[4:7], 0",
                "v_accvgpr_read_b32 v8, a0") == 7
    assert nops("v_mfma_f32_32x32x16_bf16 a[0:15], v[0:3], v[4:7], 0",
                "v_accvgpr_read_b32 v8, a0") == 11
    assert nops("v_mfma_f32_32x32x16_bf16 a[0:15], v[0:3], v[4:7], 0",
                "v_mfma_f32_32x32x16_bf16 a[0:15], v[8:11], v[12:15], a[0:15]") == 0


def test_fwd_row_sum_mfma_variant(gens):
    """gen_fwd MSUM=2 (A/B knob, round 4): 8 v_mfma_f32_16x16x32_bf16 per body replace the
    row-sum adds, the selector A operand is set once in the prologue, and the variant still
    fits the register file and assembles."""
    _, F64, *_ = gens
    saved = F64.MSUM
    try:
        F64.MSUM = 2
        k, st = F64.gen_fwd()
    finally:
        F64.MSUM = saved
    text = st.text()
    assert text.count("v_mfma_f32_16x16x32_bf16") == 8 * 16
    assert text.count("v_add_f32") < 200  # the per-score adds are gone (l updates remain)


# ------------------------------------------------------------------ shared generator helpers
@pytest.fixture(scope="module")
def asmgen(gens):
    import asmgen as M
    return M


def _check_place(asmgen, items, ngaps):
    """The scheduler's contract on one item list; returns the gaps."""
    slots = asmgen.place(items, ngaps)
    assert len(slots) == ngaps
    texts = [it[0] for it in items]
    assert len(set(texts)) == len(texts)
    flat = [t for gap in slots for t in gap]
    assert sorted(flat) == sorted(texts)                  # every item in exactly one gap
    gap_of = {t: g for g, gap in enumerate(slots) for t in gap}
    early = {it[0]: (it[2] if len(it) > 2 else 0) for it in items}
    for t in texts:
        assert gap_of[t] >= early[t], (t, gap_of[t], early[t])   # never before its earliest gap
    for e in set(early.values()):                         # equal earliest gap: list order kept
        same = [t for t in texts if early[t] == e]
        assert [t for t in flat if early[t] == e] == same
    return slots


def test_place_hand_written_lists(asmgen):
    # 2-tuples behave as earliest = 0; an even split fills each gap's share
    two = [("a", 1.0), ("b", 1.0), ("c", 1.0), ("d", 1.0)]
    assert _check_place(asmgen, two, 2) == [["a", "b"], ["c", "d"]]
    assert _check_place(asmgen, [(t, c, 0) for t, c in two], 2) == [["a", "b"], ["c", "d"]]
    # a held-back item (earliest gap 2) is overtaken by the two behind it and lands at gap 2
    held = [("w", 1.0, 2), ("x", 1.0, 0), ("y", 1.0, 0), ("z", 1.0, 0)]
    assert _check_place(asmgen, held, 4) == [["x"], ["y"], ["w"], ["z"]]
    # list order within a gap's budget: "c" would fit gap 0 but does not pass "b"; the last
    # gap absorbs the remainder, over its share
    rest = [("a", 2.0), ("b", 5.0), ("c", 1.0)]
    assert _check_place(asmgen, rest, 2) == [["a"], ["b", "c"]]
    # equal earliest gaps keep list order, also behind items that passed them
    eq = [("p0", 1.0, 1), ("p1", 1.0, 1), ("e", 1.0, 0), ("f", 1.0, 0)]
    assert _check_place(asmgen, eq, 2) == [["e", "f"], ["p0", "p1"]]
    # everything held back to the last gap
    late = [("a", 1.0, 2), ("b", 3.0, 2), ("c", 1.0)]
    assert _check_place(asmgen, late, 3) == [["c"], [], ["a", "b"]]
    # mixed tuple shapes, one gap
    assert _check_place(asmgen, [("a", 4.5, 0), ("b", 8.0)], 1) == [["a", "b"]]


def test_place_on_a_real_softmax_list(gens, asmgen):
    """The contract holds on the head_dim-64 forward's masked softmax list (P^T packs held
    back to gaps 9 / 17) over its 32 gaps."""
    _, F64, *_ = gens
    V, _ = F64.regs()
    items = F64.softmax_list(V, 0, True, 3)
    items = [(f"{k}: {it[0]}",) + tuple(it[1:]) for k, it in enumerate(items)]   # unique texts
    assert max(it[2] for it in items) == 17
    _check_place(asmgen, items, 32)


@pytest.mark.parametrize("d", [64, 128, 256])
def test_tile_swizzle(asmgen, d):
    """attention.hip's LDS tile comment: 16-B chunks XOR-swizzled per row so that both read
    shapes are conflict-free (bank = byte / 4 mod 64, i.e. a 256-B bank line of 16 chunk
    slots)."""
    swz, toff = asmgen.swz, asmgen.toff_bytes
    chunks = d // 8
    slot = lambda r, c8: toff(d, r, 8 * c8) // 16 % 16
    for r in range(64):
        # a row's chunks are a permutation of its own chunk slots, elements stay in order
        assert sorted(toff(d, r, 8 * c) for c in range(chunks)) == \
            [2 * r * d + 16 * c for c in range(chunks)]
        assert 0 <= swz(d, r) < min(chunks, 16)
        for c in range(0, d, 8):
            assert [toff(d, r, c + e) - toff(d, r, c) for e in range(8)] == list(range(0, 16, 2))
    for c8 in range(chunks):
        # 8 consecutive rows: one chunk column falls into 8 distinct slots
        for r0 in range(64 - 7):
            assert len({slot(r, c8) for r in range(r0, r0 + 8)}) == 8, (d, c8, r0)
        # ds_read_b128 row fragments: a 16-lane group reads one chunk of 16 rows
        # {0-3, 12-15, 20-27} or {4-11, 16-19, 28-31} (+32): distinct slots
        for base in (0, 32):
            for rows in ((*range(0, 4), *range(12, 16), *range(20, 28)),
                         (*range(4, 12), *range(16, 20), *range(28, 32))):
                assert len({slot(base + r, c8) for r in rows}) == 16, (d, c8, base, rows)
    # ds_read_b64_tr_b16: a 32-lane group reads 4 consecutive chunks of rows 4m..4m+3: the
    # four 64-B pieces fall in different quarters of the bank line
    for m in range(16):
        for c0 in range(0, chunks, 4):
            quarters = []
            for r in range(4 * m, 4 * m + 4):
                q = {slot(r, c0 + k) // 4 for k in range(4)}
                assert len(q) == 1
                quarters += q
            assert sorted(quarters) == [0, 1, 2, 3], (d, m, c0)


def test_mad64_and_rsrc_text(asmgen):
    st = asmgen.Stream()
    asmgen.mad64(st, "s50", "s51", "s4", "s34", "s35", "s90")
    assert st.lines == ["\ts_mul_i32 s50, s4, s34",
                        "\ts_mul_hi_u32 s51, s4, s34",
                        "\ts_mul_i32 s90, s4, s35",
                        "\ts_add_u32 s51, s51, s90"]
    st = asmgen.Stream()
    asmgen.rsrc(st, "s[56:59]", "s16", "s17", "s44", ("s50", "s51"))
    assert st.lines == ["\ts_add_u32 s56, s16, s50",
                        "\ts_addc_u32 s57, s17, s51",
                        "\ts_and_b32 s57, s57, 0xffff",
                        "\ts_mov_b32 s58, s44",
                        "\ts_mov_b32 s59, 0x20000"]


def test_generation_ignores_environment(tmp_path):
    """No switch of the generators is reachable from the environment: the driver writes the
    same bytes with leftover experiment variables set."""
    clean = {k: v for k, v in os.environ.items()
             if not k.startswith("VDIFF_") and k != "PHASE_FLIP"}
    dirty = dict(clean, VDIFF_ASM_KNOB="gen_fwd.MSUM=2", VDIFF_PHASE_FLIP="all", PHASE_FLIP="all")
    runs = []
    for k, env in enumerate((clean, dirty)):   # the two runs side by side
        out = tmp_path / f"attn_{k}.s"
        runs.append((out, subprocess.Popen(
            [sys.executable, os.path.join(ASM, "gen_attn_asm.py"), str(out)], env=env)))
    outs = []
    for out, proc in runs:
        assert proc.wait() == 0
        outs.append(out.read_bytes())
    assert len(outs[0]) > 1 << 20 and outs[0] == outs[1]
