// window.hip -- long-clip sampling: the two memory-bound kernels around the windowed denoiser
// forward (vdiff.engine.sample_long).  A long latent x [B][C][L][HW] (contiguous NCTHW, the
// samplers' layout) is cut into W overlapping windows of Tw frames, the denoiser runs on the
// windows as one batch, and the windows' predictions are blended back into one long tensor.
//
//   vd_window_gather: win[b * W + w][c][f][hw] = x[b][c][starts[w] + f][hw]        (a copy)
//   vd_window_blend:  out[b][c][l][hw] = sum_k wgt[l][k] win[b * W + cw[l][k]][c][l - starts[cw[l][k]]][hw]
//
// Both are gathers over their OUTPUT elements, one element or one 16-byte vector per thread
// over a flat grid: no atomics, no memset, no workspace, nothing shared between blocks, and a
// fixed summation order (ascending k), so an eager launch and a replayed one give the same bits.
// No table content can move an access out of bounds: the gather clamps a start into [0, L -
// Tw], the blend skips an entry whose window is outside [0, W) or whose local frame is outside
// [0, Tw).
#include "vd_common.h"

namespace {

constexpr int kBlock = 256;

// 16 bytes of T <-> fp32 (4 floats, or 8 bf16)
__device__ __forceinline__ void ld16(const float* p, float (&v)[8]) {
  const float4 a = *reinterpret_cast<const float4*>(p);
  v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
}
__device__ __forceinline__ void ld16(const bf16_t* p, float (&v)[8]) { load8(p, v); }
__device__ __forceinline__ void st16(float* p, const float (&v)[8]) {
  *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
}
__device__ __forceinline__ void st16(bf16_t* p, const float (&v)[8]) { store8(p, v); }

struct WindowShape {
  uint32_t C, L, Tw, W, HW;  // channels, clip frames, window frames, windows, pixels per frame
};

// VEC == 1: one element per thread; otherwise 16 / sizeof(T) elements, moved as one uint4.
// v indexes the vectors of win: [B * W][C][Tw][HW / VEC].
template <typename T, int VEC>
__global__ void __launch_bounds__(kBlock) gather_kernel(const T* __restrict__ x,
                                                        T* __restrict__ win, T* __restrict__ dup,
                                                        const int32_t* __restrict__ starts,
                                                        WindowShape s, int64_t nvec) {
  const int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (v >= nvec) return;
  const uint32_t hwv = s.HW / VEC;
  const int64_t row_vecs = (int64_t)s.Tw * hwv;
  const int64_t row = v / row_vecs;  // (b * W + w) * C + c
  const uint32_t rem = (uint32_t)(v - row * row_vecs);
  const uint32_t f = rem / hwv, hv = rem - f * hwv;
  const uint32_t bw = (uint32_t)row / s.C, c = (uint32_t)row - bw * s.C;
  const uint32_t b = bw / s.W, w = bw - b * s.W;
  int32_t st = starts[w];
  const int32_t last = (int32_t)(s.L - s.Tw);
  st = st < 0 ? 0 : (st > last ? last : st);
  const int64_t src = (((int64_t)b * s.C + c) * s.L + (uint32_t)st + f) * s.HW + (int64_t)hv * VEC;
  const int64_t dst = v * VEC;
  if constexpr (VEC == 1) {
    const T e = x[src];
    win[dst] = e;
    if (dup) dup[dst] = e;
  } else {
    const uint4 e = *reinterpret_cast<const uint4*>(x + src);
    *reinterpret_cast<uint4*>(win + dst) = e;
    if (dup) *reinterpret_cast<uint4*>(dup + dst) = e;
  }
}

// v indexes the vectors of out: [B][C][L][HW / VEC].  The first covering window's product
// initialises the accumulator, the rest are one fp32 fma each in ascending k, and the sum is
// rounded once to T.
template <typename T, int VEC>
__global__ void __launch_bounds__(kBlock) blend_kernel(const T* __restrict__ win,
                                                       T* __restrict__ out,
                                                       const int32_t* __restrict__ starts,
                                                       const int32_t* __restrict__ cover_win,
                                                       const float* __restrict__ cover_wgt,
                                                       int kmax, WindowShape s, int64_t nvec) {
  const int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (v >= nvec) return;
  const uint32_t hwv = s.HW / VEC;
  const int64_t row_vecs = (int64_t)s.L * hwv;
  const int64_t row = v / row_vecs;  // b * C + c
  const uint32_t rem = (uint32_t)(v - row * row_vecs);
  const uint32_t l = rem / hwv, hv = rem - l * hwv;
  const uint32_t b = (uint32_t)row / s.C, c = (uint32_t)row - b * s.C;
  float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  bool first = true;
  for (int k = 0; k < kmax; ++k) {
    const int32_t w = cover_win[(int64_t)l * kmax + k];
    if (w < 0 || (uint32_t)w >= s.W) continue;
    const int64_t f = (int64_t)l - starts[w];
    if (f < 0 || f >= (int64_t)s.Tw) continue;
    const float g = cover_wgt[(int64_t)l * kmax + k];
    const int64_t src =
        ((((int64_t)b * s.W + w) * s.C + c) * s.Tw + f) * s.HW + (int64_t)hv * VEC;
    float e[8];
    if constexpr (VEC == 1) {
      e[0] = Elem<T>::ld(win + src);
    } else {
      ld16(win + src, e);
    }
#pragma unroll
    for (int i = 0; i < VEC; ++i) acc[i] = first ? g * e[i] : __builtin_fmaf(g, e[i], acc[i]);
    first = false;
  }
  const int64_t dst = v * VEC;
  if constexpr (VEC == 1) {
    Elem<T>::st(out + dst, acc[0]);
  } else {
    st16(out + dst, acc);
  }
}

bool aligned16(std::initializer_list<const void*> ptrs) {
  uintptr_t a = 0;
  for (const void* p : ptrs) a |= reinterpret_cast<uintptr_t>(p);
  return a % 16 == 0;
}

// The shape both entry points take, checked before anything is launched.
int check_shape(int64_t B, int64_t C, int64_t L, int64_t Tw, int64_t W, int64_t HW,
                WindowShape* s) {
  VD_REQUIRE(B > 0 && C > 0 && L > 0 && Tw > 0 && W > 0 && HW > 0,
             "empty shape (B=%lld, C=%lld, L=%lld, T=%lld, W=%lld, HW=%lld)", (long long)B,
             (long long)C, (long long)L, (long long)Tw, (long long)W, (long long)HW);
  VD_REQUIRE(Tw <= L, "window of %lld frames is longer than the clip's %lld", (long long)Tw,
             (long long)L);
  // the kernels split an index into 32-bit row / frame / pixel parts; offsets are 64-bit
  const int64_t lim = (int64_t)1 << 31;
  VD_REQUIRE(B < lim && W < lim && C < lim && HW < lim && B * W < lim / C && L < lim / HW,
             "shape too large (B=%lld, C=%lld, L=%lld, W=%lld, HW=%lld: B * W * C and L * HW "
             "must be below 2^31)", (long long)B, (long long)C, (long long)L, (long long)W,
             (long long)HW);
  *s = WindowShape{(uint32_t)C, (uint32_t)L, (uint32_t)Tw, (uint32_t)W, (uint32_t)HW};
  return VD_OK;
}

inline int64_t blocks_for(int64_t nvec) { return vd_cdiv(nvec, kBlock); }

}  // namespace

int vd_window_gather(const void* x, void* win, void* win_dup, const int32_t* starts, int64_t B,
                     int64_t C, int64_t L, int64_t T, int64_t W, int64_t HW, int dtype,
                     void* stream) {
  VD_REQUIRE(x && win && starts, "null argument");
  WindowShape s;
  if (int rc = check_shape(B, C, L, T, W, HW, &s)) return rc;
  const int64_t n = B * W * C * T * HW;
  return VD_DISPATCH_DTYPE(dtype, E, {
    constexpr int V = 16 / (int)sizeof(E);
    const bool vec = HW % V == 0 && aligned16({x, win, win_dup});
    const int64_t nvec = vec ? n / V : n;
    VD_REQUIRE(blocks_for(nvec) < ((int64_t)1 << 31), "grid too large (%lld blocks)",
               (long long)blocks_for(nvec));
    if (vec)
      gather_kernel<E, V><<<(unsigned)blocks_for(nvec), kBlock, 0, VD_STREAM(stream)>>>(
          (const E*)x, (E*)win, (E*)win_dup, starts, s, nvec);
    else
      gather_kernel<E, 1><<<(unsigned)blocks_for(nvec), kBlock, 0, VD_STREAM(stream)>>>(
          (const E*)x, (E*)win, (E*)win_dup, starts, s, nvec);
  });
}

int vd_window_blend(const void* win, void* out, const int32_t* starts, const int32_t* cover_win,
                    const float* cover_wgt, int kmax, int64_t B, int64_t C, int64_t L, int64_t T,
                    int64_t W, int64_t HW, int dtype, void* stream) {
  VD_REQUIRE(win && out && starts && cover_win && cover_wgt, "null argument");
  VD_REQUIRE(kmax >= 1 && kmax <= VD_WINDOW_KMAX, "kmax %d outside [1, %d]", kmax,
             VD_WINDOW_KMAX);
  WindowShape s;
  if (int rc = check_shape(B, C, L, T, W, HW, &s)) return rc;
  const int64_t n = B * C * L * HW;
  return VD_DISPATCH_DTYPE(dtype, E, {
    constexpr int V = 16 / (int)sizeof(E);
    const bool vec = HW % V == 0 && aligned16({win, out});
    const int64_t nvec = vec ? n / V : n;
    VD_REQUIRE(blocks_for(nvec) < ((int64_t)1 << 31), "grid too large (%lld blocks)",
               (long long)blocks_for(nvec));
    if (vec)
      blend_kernel<E, V><<<(unsigned)blocks_for(nvec), kBlock, 0, VD_STREAM(stream)>>>(
          (const E*)win, (E*)out, starts, cover_win, cover_wgt, kmax, s, nvec);
    else
      blend_kernel<E, 1><<<(unsigned)blocks_for(nvec), kBlock, 0, VD_STREAM(stream)>>>(
          (const E*)win, (E*)out, starts, cover_win, cover_wgt, kmax, s, nvec);
  });
}
