"""CPU checks of the head_dim-64 backward bodies and their MFMA shape (csrc/asm/gen_attn_asm.py,
twins of attn_bwd_dkdv_pipe_kernel / attn_bwd_dq_pipe_kernel in attention.hip).  Each kernel
ships ONE shape: vd_attn_bwd_dkdv_d64 v_mfma_f32_16x16x32_bf16, 128 MFMAs per 64-query tile;
vd_attn_bwd_dq_d64 v_mfma_f32_32x32x16_bf16, 48 per 64-key tile.  For the 16x16x32 kernel the lane
and fragment tables are compared with a NumPy restatement of the HIP twin's index formulas
(m16_chunk, m16_row, toff, mma_rows_nb<M16>, mma_tr_nb<M16>) for all 4 waves x 64 lanes, and one
tile's products are emulated through the tables on random integers -- LDS image, ds_read_b128,
ds_read_b64_tr_b16 and the MFMA operand maps -- so a wrong permutation shows without a GPU."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

ASM = os.path.join(ROOT, "lipreading-video-generation_amd", "csrc", "asm")
CLANG = "/opt/rocm/llvm/bin/clang"
M16, M32 = "v_mfma_f32_16x16x32_bf16", "v_mfma_f32_32x32x16_bf16"


@pytest.fixture(scope="module")
def G():
    sys.path.insert(0, ASM)
    try:
        import gen_attn_asm
        yield gen_attn_asm
    finally:
        sys.path.remove(ASM)


def _body(lines, start, stop):
    i0 = next(i for i, l in enumerate(lines) if start in l)
    i1 = next(i for i, l in enumerate(lines) if i > i0 and stop in l)
    ops = [l.split()[0] for l in lines[i0:i1] if l.strip() and not l.strip().startswith((";", "."))]
    return {k: ops.count(k) for k in set(ops)}


def _shape(c):
    """The one MFMA shape of a body and its count."""
    shapes = [k for k in c if k.startswith("v_mfma")]
    assert len(shapes) == 1, shapes
    return shapes[0], c[shapes[0]]


def test_mfma_and_valu_per_tile(G):
    """dK/dV: exactly 128 MFMAs per tile, all 16x16x32; dQ: exactly 48, all 32x32x16.  The VALU
    multiset per tile is what it was on 32x32x16: exp / mul / cvt 64/64/64 (dK/dV), 64/64/32 (dQ)."""
    _, _, st = G.gen_dkdv()
    c = _body(st.lines, "query tile, ring stage 1", "query tile, ring stage 2")
    assert _shape(c) == (M16, 128)
    assert (c["v_exp_f32"], c["v_mul_f32"], c["v_cvt_pk_bf16_f32"]) == (64, 64, 64)
    assert c["buffer_load_dwordx4"] == 4 and c["buffer_load_dword"] == 1 and c["s_barrier"] == 1
    assert c["ds_read_b64_tr_b16"] == 32
    _, _, st = G.gen_dq()
    c = _body(st.lines, "tile, ring stage 1", "tile, ring stage 2")
    assert _shape(c) == (M32, 48)
    assert (c["v_exp_f32"], c["v_mul_f32"], c["v_cvt_pk_bf16_f32"]) == (64, 64, 32)
    assert c["buffer_load_dwordx4"] == 4 and c["s_barrier"] == 1


def test_one_heavy_instruction_per_short_gap(G):
    """A 16x16x32 MFMA gap hides 8 cycles of vector issue: between two MFMAs of the dK/dV loop
    body there is at most one 8-cycle instruction (v_exp_f32), alone or beside address
    arithmetic, and never more than three VALU instructions."""
    st = G.gen_dkdv()[-1]
    i0 = next(i for i, l in enumerate(st.lines) if "query tile, ring stage 1" in l)
    i1 = next(i for i, l in enumerate(st.lines) if i > i0 and "query tile, ring stage 2" in l)
    ops = [l.split()[0] for l in st.lines[i0:i1] if l.strip()]
    assert ops.count(M16) == 128
    exps = valu = 0
    for op in ops:
        if op.startswith("v_mfma"):
            assert exps <= 1 and valu <= 3, (exps, valu)
            exps = valu = 0
        elif op.startswith("v_"):
            valu += 1
            exps += op == "v_exp_f32"


def test_assembles_and_fits(tmp_path, G):
    if not os.path.exists(CLANG) and not shutil.which(CLANG):
        pytest.skip("ROCm clang not present")
    out = tmp_path / "attn_asm.s"
    subprocess.run([sys.executable, os.path.join(ASM, "gen_attn_asm.py"), str(out)], check=True)
    subprocess.run([CLANG, "-x", "assembler", "-target", "amdgcn-amd-amdhsa", "-mcpu=gfx950",
                    "-c", str(out), "-o", str(tmp_path / "a.o")], check=True)
    for regs in (G.regs_dq, G.regs_dkdv):
        V, A = regs()
        assert V.next <= 256 and A.next <= 256 and (V.next + 3) // 4 * 4 + A.next <= 512
    # the ring and the row constants fit the 160 KiB of a CU with room for nothing else to matter
    assert G.DK_RC_BYTES + 4 * G.DK_STAGE <= 160 * 1024


# ------------------------------------------------------------------ the HIP twin's formulas
def swz64(r):            # attention.hip swz_row<64>
    return (((r >> 1) & 1) << 2) | ((r >> 2) & 3)


def toff(r, c):          # attention.hip toff<bf16, 64>, in elements
    return r * 64 + (((c >> 3) ^ swz64(r)) << 3) + (c & 7)


def m16_chunk(ks, g):    # attention.hip m16_chunk
    return 4 * ks + g


def m16_row(it, i):      # attention.hip m16_row
    return 16 * (i >> 3) + 4 * ((i >> 2) & 1) + 8 * it + (i & 3)


def test_m16_maps_keep_the_contraction_groups_of_the_32x32_form():
    """The 16x16x32 maps are permutations, and every accumulator sees the same sequence of
    8-product contraction groups, in the same slot order, as on v_mfma_f32_32x32x16_bf16 -- the
    condition under which the two shapes return the same bits."""
    assert sorted(m16_chunk(ks, g) for ks in range(2) for g in range(4)) == list(range(8))
    assert sorted(m16_row(it, i) for it in range(2) for i in range(16)) == list(range(32))
    for it in range(2):
        for g in range(4):   # accumulator rows 4 g .. 4 g + 3 are consecutive tile rows
            assert [m16_row(it, 4 * g + r) for r in range(4)] == \
                [m16_row(it, 4 * g) + r for r in range(4)]
    # S, dP over head_dim.  32x32x16 (mma_rows_nb): k-step s = 0..3, lane half hh, slot e is
    # element 16 s + 8 hh + e.  16x16x32: k-step ks, lane group g, slot e is 8 m16_chunk + e.
    old = [[16 * s_ + 8 * hh + e for e in range(8)] for s_ in range(4) for hh in range(2)]
    new = [[8 * m16_chunk(ks, g) + e for e in range(8)] for ks in range(2) for g in range(4)]
    assert old == new
    # G products over the block's 32 rows.  32x32x16 (XOp, mma_tr_nb): k-step s2, half hh, slot
    # e is the row of accumulator register 8 s2 + e: (r & 3) + 8 (r >> 2) + 4 hh.
    old = [[((8 * s2 + e) & 3) + 8 * ((8 * s2 + e) >> 2) + 4 * hh for e in range(8)]
           for s2 in range(2) for hh in range(2)]
    # 16x16x32: lane group g, slot e is register 4 it + r = e of the key / query tile's 8
    new = [[m16_row(e >> 2, 4 * g) + (e & 3) for e in range(8)] for g in range(4)]
    assert old == new


def _m16_kernels(G):
    return [name for name, gen in (("dkdv", G.gen_dkdv), ("dq", G.gen_dq))
            if any(M16 in l for l in gen()[-1].lines)]


def test_lane_tables_match_the_hip_formulas(G):
    assert _m16_kernels(G) == ["dkdv"]
    tab = G.dk_lane_table()
    assert len(tab) == 256 and all(len(r) == 32 for r in tab)
    for w in range(4):
        for lane in range(64):
            row = tab[64 * w + lane]
            i, g = lane & 15, lane >> 4
            want = [2 * toff(m16_row(it, i), 8 * m16_chunk(ks, g))
                    for it in range(2) for ks in range(2)]
            want += [2 * toff(m16_row(hi, 4 * g) + (i >> 2), 16 * dt + 4 * (i & 3))
                     for dt in range(4) for hi in range(2)]
            assert row[:12] == want, (w, lane)
            # DMA pieces (dma_tile<64, 4>): piece p of wave w, row 8 (2 w + p) + lane / 8
            for p in range(2):
                rr = (2 * w + p) * 8 + lane // 8
                assert row[12 + p] == rr and row[14 + p] == ((lane % 8) ^ swz64(rr)) * 16
            assert row[16:20] == [4 * m16_row(0, 4 * g), 4 * m16_row(1, 4 * g),
                                  16 * m16_chunk(0, g), 8 * g]
    # the DMA pieces of the 4 waves cover every 16-B chunk slot of the 64-row tile once
    seen = {(tab[64 * w + l][12 + p], l % 8) for w in range(4) for l in range(64) for p in range(2)}
    assert len(seen) == 64 * 8


# ------------------------------------------------------------------ emulation of one tile
def mfma16(a, b):
    """v_mfma_f32_16x16x32_bf16 on integer fragments a, b [64 lanes][8]: lane (i, g) holds A row
    i / B column i, contraction slots 8 g .. 8 g + 7; result [64][4]: column lane & 15, rows
    4 (lane >> 4) + r."""
    A = np.zeros((16, 32), np.int64)
    B = np.zeros((32, 16), np.int64)
    for l in range(64):
        A[l & 15, 8 * (l >> 4):8 * (l >> 4) + 8] = a[l]
        B[8 * (l >> 4):8 * (l >> 4) + 8, l & 15] = b[l]
    C = A @ B
    return np.array([[C[4 * (l >> 4) + r, l & 15] for r in range(4)] for l in range(64)])


def lds_image(tile):
    """A [64][64] tile as the ring holds it (element index toff)."""
    img = np.zeros(64 * 64, np.int64)
    for r in range(64):
        for c in range(64):
            img[toff(r, c)] = tile[r, c]
    return img


def read_b128(img, byte_addr):
    return np.array([img[a // 2:a // 2 + 8] for a in byte_addr])


def read_tr(img, byte_addr):
    """ds_read_b64_tr_b16: in each group of 16 lanes, lane 4 q + p supplies the address of row q,
    columns 4 p .. 4 p + 3; lane i receives column i of the 4 rows, row q in element q."""
    out = np.zeros((64, 4), np.int64)
    for l in range(64):
        g, i = l >> 4, l & 15
        for q in range(4):
            src = 16 * g + 4 * q + (i >> 2)
            out[l, q] = img[byte_addr[src] // 2 + (i & 3)]
    return out


def test_dkdv_tile_products_through_the_tables(G):
    """S' = Q K^T and dP = dO V^T of every block of one tile, then dV^T += dO^T P and
    dK^T += Q^T dS with the accumulators' own registers as B operands, against plain matrix
    products; the row-constant and the output-row offsets name the same rows / columns."""
    assert "dkdv" in _m16_kernels(G)
    rng = np.random.default_rng(5)
    tab = np.array(G.dk_lane_table()).reshape(4, 64, 32)
    Q, dO = rng.integers(-4, 5, (2, 64, 64))          # one 64-query tile
    K, Vv = rng.integers(-4, 5, (2, 256, 64))         # the workgroup's 256 keys
    qi, oi = lds_image(Q), lds_image(dO)
    lanes = np.arange(64)
    for w in range(4):
        t = tab[w]
        S = np.zeros((2, 2, 64, 16), np.int64)        # [qb][kj][lane][register]
        dP = np.zeros_like(S)
        for qb in range(2):
            for kj in range(2):
                for it in range(2):
                    for jt in range(2):
                        s = np.zeros((64, 4), np.int64)
                        d = np.zeros((64, 4), np.int64)
                        for ks in range(2):
                            ad = t[:, 2 * it + ks] + qb * 4096
                            key = 64 * w + 32 * kj + 16 * jt + (lanes & 15)
                            el = (t[:, 18] + 64 * ks) // 2
                            kf = np.array([K[key[l], el[l]:el[l] + 8] for l in range(64)])
                            vf = np.array([Vv[key[l], el[l]:el[l] + 8] for l in range(64)])
                            s += mfma16(read_b128(qi, ad), kf)
                            d += mfma16(read_b128(oi, ad), vf)
                        o = 4 * (2 * jt + it)
                        S[qb, kj, :, o:o + 4], dP[qb, kj, :, o:o + 4] = s, d
                        for l in range(64):
                            q0 = 32 * qb + m16_row(it, 4 * (l >> 4))
                            assert (t[l, 16 + it] + 128 * qb) == 4 * q0
                            key = 64 * w + 32 * kj + 16 * jt + (l & 15)
                            assert (s[l] == Q[q0:q0 + 4] @ K[key]).all(), (w, qb, kj, it, jt, l)
                            assert (d[l] == dO[q0:q0 + 4] @ Vv[key]).all()
        # G products: P := S, dS := dP as integers (the softmax is elementwise in place)
        adv = np.zeros((64, 64), np.int64)            # [lane][accumulator register]
        adk = np.zeros((64, 64), np.int64)
        for qb in range(2):
            for dt in range(4):
                otr = np.concatenate([read_tr(oi, t[:, 4 + 2 * dt + hi] + qb * 4096)
                                      for hi in range(2)], axis=1)
                qtr = np.concatenate([read_tr(qi, t[:, 4 + 2 * dt + hi] + qb * 4096)
                                      for hi in range(2)], axis=1)
                for kj in range(2):
                    for jt in range(2):
                        a = G.acc_idx(dt, kj, jt)
                        adv[:, a:a + 4] += mfma16(otr, S[qb, kj, :, 8 * jt:8 * jt + 8])
                        adk[:, a:a + 4] += mfma16(qtr, dP[qb, kj, :, 8 * jt:8 * jt + 8])
        Pfull = Q @ K[64 * w:64 * w + 64].T           # [query][key of the wave]
        Dfull = dO @ Vv[64 * w:64 * w + 64].T
        dV, dK = Pfull.T @ dO, Dfull.T @ Q            # [key][d]
        for l in range(64):
            for kj in range(2):
                for jt in range(2):
                    key = 32 * kj + 16 * jt + (l & 15)
                    for dt in range(4):
                        a = G.acc_idx(dt, kj, jt)
                        d0 = (t[l, 19] + 32 * dt) // 2     # the store's first column
                        assert d0 == 16 * dt + 4 * (l >> 4)
                        assert (adv[l, a:a + 4] == dV[key, d0:d0 + 4]).all(), (w, l, kj, jt, dt)
                        assert (adk[l, a:a + 4] == dK[key, d0:d0 + 4]).all()

