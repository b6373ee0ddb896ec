// metrics.hip -- clip quality metrics on the device: per-frame MSE (for PSNR) and SSIM of two
// clips, over the whole frame or over a weighted region, declared in include/vdiff.h
// (vd_clip_metrics*).  Build extension, no reference counterpart.
//
// Definition.  x, y: contiguous [B][C][T][H][W] in `dtype`; a frame is the C planes of one
// (b, t).  weight: fp32 [T][H][W] >= 0 shared by batch and channel, or NULL = all ones.
//   u        = clamp((v - lo) / (hi - lo), 0, 1)                      (the data range is then 1)
//   mse[b,t] = sum_c sum_px w[t,px] (ux - uy)^2 / (C sum_px w[t,px])  (psnr = -10 log10 mse)
//   SSIM (Wang et al. 2004): g = the 11-tap Gaussian, sigma 1.5, normalised in double, rounded
//   to fp32; the window is g (x) g; VALID positions only, so the map of a plane is (H - 10) x
//   (W - 10); with E[.] the window-weighted sum at a position,
//     mx = E[ux], my = E[uy], vx = E[ux^2] - mx^2, vy = E[uy^2] - my^2, cxy = E[ux uy] - mx my,
//     s  = (2 mx my + C1) (2 cxy + C2) / ((mx^2 + my^2 + C1) (vx + vy + C2)),
//     C1 = 0.01^2, C2 = 0.03^2;
//   the score of a plane is the mean of s weighted with w at the window's CENTRE pixel (y + 5,
//   x + 5), and ssim[b,t] the mean over the C planes:
//     ssim[b,t] = sum_c sum_pos w s / (C sum_pos w).
//   wsum_px[t] = sum_px w, wsum_valid[t] = sum_pos w.  A frame whose weight sum is 0 gets NaN
//   (0 / 0) in mse resp. ssim.
//
// Plan.  metrics_tile_kernel: one workgroup per (plane, 32 x 32 tile of map positions).
//   1. The 42 x 42 patch of x and y goes to LDS as PIVOTED values dx = ux - px, dy = uy - py,
//      px, py the pixel at the patch's centre (as gn_stats_kernel's `shift`; the centre halves
//      the largest |dx| of a gradient against the first pixel).  The clamp is applied to the
//      raw value (clamp(v, lo, hi): the same u), so that dx = (vx - pv) / (hi - lo) and the
//      difference d = (vx - vy) / (hi - lo) start from exact fp32 subtractions of neighbouring
//      values instead of two roundings of v - lo.  In the same pass the thread that loaded a
//      pixel the tile OWNS adds w d^2: a tile owns its 32 x 32 pixels, and the last tile of an
//      axis also the 10 border pixels behind them, so every pixel of the plane has one owner.
//   2. Horizontal 11-tap pass of the five moments (dx, dy, dx^2, dy^2, dx dy) into LDS.
//   3. Vertical pass in registers, four positions of one column per thread, then s.  Variance
//      and covariance are shift-invariant only for a window that sums to 1; the fp32 taps sum
//      to S = 1 - e, e of the order 1e-8, and the definition is on the unpivoted u, so the
//      exact first-order terms are put back:
//        mx  = a + px S,  vx = (q - a^2) + e (2 px a + px^2 S),
//        cxy = (qxy - a b) + e (px b + py a + px py S)        (a = E[dx], q = E[dx^2], ...).
//      Without the pivot E[x^2] - mx^2 in fp32 is wrong by ~1e-7 against C2 = 9e-4.
//   4. The tile's sum w s, sum w d^2 and the two weight sums: shuffle tree per wave, then the
//      four waves in index order; one 16-byte record per (plane, tile) into the workspace.
// metrics_finish_kernel: one workgroup per (b, t) adds the records over channels and tiles in
// index order (fp64) and writes mse, ssim; the workgroups of b = 0 write the weight sums.
// Two launches, no atomics, no memset, every workspace word read was written by the same call:
// the same bits every run, eager or replayed from a HIP graph.  Scalar loads: rows need no
// alignment.  Plane offsets are int64.
#include "vd_common.h"
#include <cmath>

namespace {

constexpr int kWin = 11;
constexpr int kHalo = kWin - 1;
constexpr int kTile = 32;
constexpr int kPatch = kTile + kHalo;  // 42
constexpr int kBlock = 256;
constexpr int kRows = 4;               // map positions per thread: kTile * kTile / kBlock
constexpr float kC1 = 1e-4f;           // (0.01 L)^2, L = 1
constexpr float kC2 = 9e-4f;           // (0.03 L)^2

struct Window {
  float g[kWin];
  float S;  // sum of the 2-D window (fp64 sum of the fp32 taps, squared)
  float e;  // 1 - S
};

Window make_window() {
  double g[kWin], s = 0.0;
  for (int k = 0; k < kWin; ++k) {
    const double d = k - kWin / 2;
    g[k] = std::exp(-d * d / (2.0 * 1.5 * 1.5));
    s += g[k];
  }
  Window w;
  double s1 = 0.0;
  for (int k = 0; k < kWin; ++k) {
    w.g[k] = (float)(g[k] / s);
    s1 += (double)w.g[k];
  }
  w.S = (float)(s1 * s1);
  w.e = (float)(1.0 - s1 * s1);
  return w;
}

__device__ __forceinline__ float clampv(float v, float lo, float hi) {
  return v < lo ? lo : (v > hi ? hi : v);  // a NaN stays a NaN
}

template <typename T>
__global__ void __launch_bounds__(kBlock) metrics_tile_kernel(
    const T* __restrict__ x, const T* __restrict__ y, const float* __restrict__ weight,
    const Window win, float lo, float hi, int Tn, int H, int W, int ntx, int ntiles,
    float* __restrict__ ssim_map, float* __restrict__ part) {
  __shared__ float sx[kPatch * kPatch];
  __shared__ float sy[kPatch * kPatch];
  __shared__ float hm[5][kPatch][kTile];
  __shared__ float red[4][kBlock / 64];
  const int tid = threadIdx.x;
  const int64_t plane = blockIdx.x / ntiles;
  const int tile = blockIdx.x % ntiles;
  const int y0 = (tile / ntx) * kTile, x0 = (tile % ntx) * kTile;
  const int MH = H - kHalo, MW = W - kHalo;
  const int mh = MH - y0 < kTile ? MH - y0 : kTile;
  const int mw = MW - x0 < kTile ? MW - x0 : kTile;
  // owned pixels: the last tile of an axis takes the border behind it
  const int oh = MH - y0 <= kTile ? H - y0 : kTile;
  const int ow = MW - x0 <= kTile ? W - x0 : kTile;
  const int64_t HW = (int64_t)H * W;
  const T* xp = x + plane * HW;
  const T* yp = y + plane * HW;
  const float* wp = weight ? weight + (plane % Tn) * HW : nullptr;
  const float span = hi - lo;
  // pivot: the patch's centre pixel, or the plane's last row / column where the patch is ragged
  const int yc = y0 + kPatch / 2 < H ? y0 + kPatch / 2 : H - 1;
  const int xc = x0 + kPatch / 2 < W ? x0 + kPatch / 2 : W - 1;
  const int64_t o0 = (int64_t)yc * W + xc;
  const float pvx = clampv(Elem<T>::ld(xp + o0), lo, hi);
  const float pvy = clampv(Elem<T>::ld(yp + o0), lo, hi);

  float s_mse = 0.f, s_wpx = 0.f;
  for (int i = tid; i < kPatch * kPatch; i += kBlock) {
    const int r = i / kPatch, c = i % kPatch;
    const int gy = y0 + r, gx = x0 + c;
    float dx = 0.f, dy = 0.f;
    if (gy < H && gx < W) {
      const int64_t o = (int64_t)gy * W + gx;
      const float vx = clampv(Elem<T>::ld(xp + o), lo, hi);
      const float vy = clampv(Elem<T>::ld(yp + o), lo, hi);
      dx = (vx - pvx) / span;
      dy = (vy - pvy) / span;
      if (r < oh && c < ow) {
        const float w = wp ? wp[o] : 1.f;
        const float d = (vx - vy) / span;
        s_mse = fmaf(w, d * d, s_mse);
        s_wpx += w;
      }
    }
    sx[i] = dx;
    sy[i] = dy;
  }
  __syncthreads();

  for (int i = tid; i < kPatch * kTile; i += kBlock) {
    const int r = i / kTile, c = i % kTile;
    const float* rx = sx + r * kPatch + c;
    const float* ry = sy + r * kPatch + c;
    float a = 0.f, b = 0.f, aa = 0.f, bb = 0.f, ab = 0.f;
#pragma unroll
    for (int k = 0; k < kWin; ++k) {
      const float fx = rx[k], fy = ry[k];
      const float gx = win.g[k] * fx, gy = win.g[k] * fy;
      a += gx;
      b += gy;
      aa = fmaf(gx, fx, aa);
      bb = fmaf(gy, fy, bb);
      ab = fmaf(gx, fy, ab);
    }
    hm[0][r][c] = a;
    hm[1][r][c] = b;
    hm[2][r][c] = aa;
    hm[3][r][c] = bb;
    hm[4][r][c] = ab;
  }
  __syncthreads();

  const int mx = tid % kTile;
  const int r0 = (tid / kTile) * kRows;
  float acc[5][kRows];
#pragma unroll
  for (int m = 0; m < 5; ++m)
#pragma unroll
    for (int o = 0; o < kRows; ++o) acc[m][o] = 0.f;
#pragma unroll
  for (int rr = 0; rr < kRows + kHalo; ++rr) {
#pragma unroll
    for (int m = 0; m < 5; ++m) {
      const float v = hm[m][r0 + rr][mx];
#pragma unroll
      for (int o = 0; o < kRows; ++o) {
        const int k = rr - o;  // tap of output o this row feeds: ascending k per output
        if (k >= 0 && k < kWin) acc[m][o] = fmaf(win.g[k], v, acc[m][o]);
      }
    }
  }
  const float px = (pvx - lo) / span, py = (pvy - lo) / span;
  float s_ssim = 0.f, s_wv = 0.f;
#pragma unroll
  for (int o = 0; o < kRows; ++o) {
    const int my = r0 + o;
    if (my < mh && mx < mw) {
      const float a = acc[0][o], b = acc[1][o];
      const float mux = fmaf(px, win.S, a), muy = fmaf(py, win.S, b);
      const float vx = (acc[2][o] - a * a) + win.e * (2.f * px * a + px * px * win.S);
      const float vy = (acc[3][o] - b * b) + win.e * (2.f * py * b + py * py * win.S);
      const float cxy = (acc[4][o] - a * b) + win.e * (px * b + py * a + px * py * win.S);
      const float num = (2.f * mux * muy + kC1) * (2.f * cxy + kC2);
      const float den = (mux * mux + muy * muy + kC1) * (vx + vy + kC2);
      const float s = num / den;
      const int gy = y0 + my, gx = x0 + mx;
      if (ssim_map) ssim_map[plane * ((int64_t)MH * MW) + (int64_t)gy * MW + gx] = s;
      const float w = wp ? wp[(int64_t)(gy + kWin / 2) * W + (gx + kWin / 2)] : 1.f;
      s_ssim = fmaf(w, s, s_ssim);
      s_wv += w;
    }
  }

  const float v0 = wave_sum(s_ssim), v1 = wave_sum(s_mse), v2 = wave_sum(s_wpx),
              v3 = wave_sum(s_wv);
  if (tid % 64 == 0) {
    red[0][tid / 64] = v0;
    red[1][tid / 64] = v1;
    red[2][tid / 64] = v2;
    red[3][tid / 64] = v3;
  }
  __syncthreads();
  if (tid < 4) {
    float s = red[tid][0];
    for (int w = 1; w < kBlock / 64; ++w) s += red[tid][w];
    part[(int64_t)blockIdx.x * 4 + tid] = s;
  }
}

// One workgroup per (b, t).  Lane q < 4 adds component q of the records (0: sum w s, 1: sum w
// d^2 over the C planes; 2: sum_px w, 3: sum_pos w of the frame's first plane) in index order.
__global__ void __launch_bounds__(64) metrics_finish_kernel(
    const float* __restrict__ part, int C, int Tn, int ntiles, float* __restrict__ mse,
    float* __restrict__ ssim, float* __restrict__ wsum_px, float* __restrict__ wsum_valid) {
  __shared__ double tot[4];
  const int64_t b = blockIdx.x / Tn;
  const int t = blockIdx.x % Tn;
  const int q = threadIdx.x;
  if (q < 4) {
    double s = 0.0;
    const int cn = q < 2 ? C : 1;
    for (int c = 0; c < cn; ++c) {
      const float* rec = part + (((b * C + c) * Tn + t) * ntiles) * 4 + q;
      for (int k = 0; k < ntiles; ++k) s += (double)rec[(int64_t)k * 4];
    }
    tot[q] = s;
  }
  __syncthreads();
  if (q == 0) {
    ssim[blockIdx.x] = (float)(tot[0] / ((double)C * tot[3]));
    mse[blockIdx.x] = (float)(tot[1] / ((double)C * tot[2]));
    if (b == 0) {
      wsum_px[t] = (float)tot[2];
      wsum_valid[t] = (float)tot[3];
    }
  }
}

inline int64_t metrics_tiles(int H, int W, int* ntx) {
  const int64_t nx = vd_cdiv(W - kHalo, kTile), ny = vd_cdiv(H - kHalo, kTile);
  if (ntx) *ntx = (int)nx;
  return nx * ny;
}

inline bool metrics_shape_ok(int B, int C, int T, int H, int W) {
  if (B <= 0 || C <= 0 || T <= 0 || H < kWin || W < kWin) return false;
  const int64_t planes = (int64_t)B * C * T;
  return planes < ((int64_t)1 << 31) && planes * metrics_tiles(H, W, nullptr) < ((int64_t)1 << 31);
}

}  // namespace

size_t vd_clip_metrics_workspace_size(int B, int C, int T, int H, int W) {
  if (!metrics_shape_ok(B, C, T, H, W)) return 0;
  return (size_t)((int64_t)B * C * T * metrics_tiles(H, W, nullptr)) * 4 * sizeof(float);
}

int vd_clip_metrics(const void* x, const void* y, const float* weight, float lo, float hi, int B,
                    int C, int T, int H, int W, int dtype, float* mse, float* ssim,
                    float* wsum_px, float* wsum_valid, float* ssim_map, void* workspace,
                    void* stream) {
  VD_REQUIRE(H >= kWin && W >= kWin, "frame %d x %d is smaller than the %d x %d SSIM window", H,
             W, kWin, kWin);
  VD_REQUIRE(metrics_shape_ok(B, C, T, H, W), "bad shape (B=%d, C=%d, T=%d, H=%d, W=%d)", B, C, T,
             H, W);
  VD_REQUIRE(x && y && mse && ssim && wsum_px && wsum_valid && workspace,
             "null argument (only weight and ssim_map may be NULL)");
  VD_REQUIRE(std::isfinite(lo) && std::isfinite(hi) && hi > lo, "value range (%g, %g) needs finite lo < hi",
             (double)lo, (double)hi);
  VD_REQUIRE(reinterpret_cast<uintptr_t>(workspace) % sizeof(float) == 0,
             "workspace is not 4-byte aligned");
  static const Window win = make_window();
  int ntx = 0;
  const int ntiles = (int)metrics_tiles(H, W, &ntx);
  const int64_t planes = (int64_t)B * C * T;
  float* part = static_cast<float*>(workspace);
  hipStream_t st = VD_STREAM(stream);
  return VD_DISPATCH_DTYPE(dtype, Tp, {
    metrics_tile_kernel<Tp><<<(unsigned)(planes * ntiles), kBlock, 0, st>>>(
        (const Tp*)x, (const Tp*)y, weight, win, lo, hi, T, H, W, ntx, ntiles, ssim_map, part);
    metrics_finish_kernel<<<(unsigned)((int64_t)B * T), 64, 0, st>>>(part, C, T, ntiles, mse, ssim,
                                                                     wsum_px, wsum_valid);
  });
}
