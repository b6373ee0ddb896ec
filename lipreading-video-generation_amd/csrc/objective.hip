// objective.hip -- the training objective beyond the reference's MSE on eps: v-prediction
// (Salimans & Ho 2022) and Min-SNR-gamma loss weighting (Hang et al. 2023), forward and
// backward, declared in include/vdiff.h (vd_diffusion_loss*).
//
// Per sample b: i = t[b] clamped into [0, T - 1], sa = sqrt_acp[i], s1m = sqrt_1m_acp[i] (the
// tables vd_q_sample reads: the loss and q_sample see the same bits), snr = (sa / s1m)^2;
//   target  eps: eps;  v: sa eps - s1m x0, formed in registers, never written to memory;
//   w_b     none: 1;  min-snr: min(snr, gamma) / snr (eps), min(snr, gamma) / (snr + 1) (v);
//   loss = 1 / (B P) sum_b w_b sum_i (pred - target)^2.
//
// Forward: a FIXED-order reduction built to the rules of vd_mse_loss / vd_cfg_stats (DESIGN
// section 9.3: torch's one-launch multi-block reductions returned stale values when replayed
// from a HIP graph).  obj_partial_kernel runs on a (blocks per sample, B) grid laid out like
// cfg_stats_kernel: block k of sample b owns one fixed contiguous range (a multiple of 8
// elements, the last one ragged), sums d * d per lane and reduces with the LDS tree of
// mse_partial_kernel into part[b][k].  obj_finish_kernel (one block) adds each sample's partials
// in block order, writes the unweighted per-sample MSE, computes w_b on the device and adds the
// weighted samples in sample order.  Two launches, no atomics, no memset, no semaphore, no
// cross-block communication inside a launch: the same bits every run, eager or replayed.
// Backward: one launch, target and w_b recomputed.
#include "vd_common.h"
#include <initializer_list>

namespace {

constexpr int kBlock = 256;
constexpr int kObjBlocks = 128;  // partials per sample (upper bound)

inline int obj_blocks(int64_t P) {
  const int64_t g = vd_cdiv(P, (int64_t)kBlock * 8);
  return (int)(g < kObjBlocks ? (g > 0 ? g : 1) : kObjBlocks);
}
inline int64_t obj_chunk(int64_t P, int nb) { return vd_cdiv(vd_cdiv(P, nb), 8) * 8; }

template <typename T>
__device__ __forceinline__ void ld_vec(const T* p, float (&v)[8], int n) {
  if (n == 8) {
    load8(p, v);
  } else {
    for (int i = 0; i < n; ++i) v[i] = Elem<T>::ld(p + i);
  }
}
template <typename T>
__device__ __forceinline__ void st_vec(T* p, const float (&v)[8], int n) {
  if (n == 8) {
    store8(p, v);
  } else {
    for (int i = 0; i < n; ++i) Elem<T>::st(p + i, v[i]);
  }
}

struct Objective {
  const float *sa, *s1m;
  const int64_t* t;
  int64_t T;
  int min_snr;
  float gamma;
  // a bad index cannot read out of bounds (as DPMRule clamps its own)
  __device__ __forceinline__ int64_t index(int64_t b) const {
    const int64_t i = t[b];
    return i < 0 ? 0 : (i > T - 1 ? T - 1 : i);
  }
  template <bool PRED_V>
  __device__ __forceinline__ float weight(float a, float c) const {
    if (!min_snr) return 1.f;
    const float r = a / c;
    const float snr = r * r;
    const float m = fminf(snr, gamma);
    return PRED_V ? m / (snr + 1.f) : m / snr;
  }
  // d = pred - target of n elements
  template <bool PRED_V>
  __device__ __forceinline__ void diff(float a, float c, const float* p, const float* x0,
                                       const float* e, float* d, int n) const {
    for (int i = 0; i < n; ++i) {
      const float tg = PRED_V ? a * e[i] - c * x0[i] : e[i];
      d[i] = p[i] - tg;
    }
  }
};

// VEC = 8 needs P % 8 == 0 (then every range is whole 8-vectors) and 16-B alignment.
template <typename T, int VEC, bool PRED_V>
__global__ void __launch_bounds__(kBlock) obj_partial_kernel(
    Objective op, const T* __restrict__ pred, const T* __restrict__ x0,
    const T* __restrict__ eps, int64_t P, int64_t chunk, float* __restrict__ part) {
  __shared__ float red[kBlock];
  const int64_t b = blockIdx.y;
  const int64_t ti = op.index(b);
  const float a = op.sa[ti], c = op.s1m[ti];
  const int64_t lo = (int64_t)blockIdx.x * chunk;
  const int64_t hi = lo + chunk < P ? lo + chunk : P;
  const T* pb = pred + b * P;
  const T* xb = PRED_V ? x0 + b * P : nullptr;
  const T* eb = eps + b * P;
  float s = 0.f;
  for (int64_t i = lo + (int64_t)threadIdx.x * VEC; i < hi; i += (int64_t)kBlock * VEC) {
    float xp[8], xx[8] = {0, 0, 0, 0, 0, 0, 0, 0}, xe[8], d[8];
    ld_vec(pb + i, xp, VEC);
    if (PRED_V) ld_vec(xb + i, xx, VEC);
    ld_vec(eb + i, xe, VEC);
    op.diff<PRED_V>(a, c, xp, xx, xe, d, VEC);
#pragma unroll
    for (int k = 0; k < VEC; ++k) s = fmaf(d[k], d[k], s);
  }
  red[threadIdx.x] = s;
  __syncthreads();
#pragma unroll
  for (int w = kBlock / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) part[b * gridDim.x + blockIdx.x] = red[0];
}

// One block.  Samples are taken kBlock at a time: lane j adds the partials of sample base + j
// in block order, writes its MSE and leaves w_b MSE_b in LDS; lane 0 then adds the tile's
// values in sample order onto the running total.
template <bool PRED_V>
__global__ void __launch_bounds__(kBlock) obj_finish_kernel(
    Objective op, const float* __restrict__ part, int nb, int64_t B, int64_t P,
    float* __restrict__ per_sample, float* __restrict__ loss) {
  __shared__ float red[kBlock];
  float total = 0.f;
  for (int64_t base = 0; base < B; base += kBlock) {
    const int64_t b = base + threadIdx.x;
    if (b < B) {
      const float* row = part + b * nb;
      float s = 0.f;
      for (int k = 0; k < nb; ++k) s += row[k];
      const float mse = s / (float)P;
      per_sample[b] = mse;
      const int64_t ti = op.index(b);
      red[threadIdx.x] = op.weight<PRED_V>(op.sa[ti], op.s1m[ti]) * mse;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      const int n = B - base < kBlock ? (int)(B - base) : kBlock;
      for (int j = 0; j < n; ++j) total += red[j];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) *loss = total / (float)B;
}

// grad_pred = g 2 w_b / (B P) (pred - target); blockIdx.y = sample, so a block takes its
// coefficient once.  scale = 2 / (B P), rounded once from fp64 on the host.
template <typename T, int VEC, bool PRED_V>
__global__ void __launch_bounds__(kBlock) obj_bwd_kernel(
    Objective op, const T* __restrict__ pred, const T* __restrict__ x0,
    const T* __restrict__ eps, const float* __restrict__ gout, float scale, int64_t P,
    T* __restrict__ gpred) {
  const int64_t b = blockIdx.y;
  const int64_t ti = op.index(b);
  const float a = op.sa[ti], c = op.s1m[ti];
  const float coef = (*gout * scale) * op.weight<PRED_V>(a, c);
  const int64_t base = b * P;
  const int64_t nvec = P / VEC;
  for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < nvec;
       v += (int64_t)gridDim.x * blockDim.x) {
    const int64_t e = base + v * VEC;
    float xp[8], xx[8] = {0, 0, 0, 0, 0, 0, 0, 0}, xe[8], d[8];
    ld_vec(pred + e, xp, VEC);
    if (PRED_V) ld_vec(x0 + e, xx, VEC);
    ld_vec(eps + e, xe, VEC);
    op.diff<PRED_V>(a, c, xp, xx, xe, d, VEC);
#pragma unroll
    for (int k = 0; k < VEC; ++k) d[k] = coef * d[k];
    st_vec(gpred + e, d, VEC);
  }
}

// 8-wide path: whole vectors per sample and every pointer 16-B aligned (as cfg_vec8)
inline bool obj_vec8(int64_t per_sample, std::initializer_list<const void*> ptrs) {
  uintptr_t a = 0;
  for (const void* p : ptrs) a |= reinterpret_cast<uintptr_t>(p);
  return per_sample % 8 == 0 && a % 16 == 0;
}

inline int obj_check(const void* pred, const void* x0, const void* eps, const int64_t* t,
                     const float* sa, const float* s1m, int64_t T, int prediction, int weighting,
                     float gamma, int64_t B, int64_t P) {
  VD_REQUIRE(pred && eps && t && sa && s1m, "null argument");
  VD_REQUIRE(prediction == VD_PRED_EPS || prediction == VD_PRED_V, "unknown prediction type %d",
             prediction);
  VD_REQUIRE(weighting == VD_WEIGHT_NONE || weighting == VD_WEIGHT_MIN_SNR,
             "unknown loss weighting %d", weighting);
  VD_REQUIRE(prediction == VD_PRED_EPS || x0, "v-prediction needs x0 (null)");
  VD_REQUIRE(weighting == VD_WEIGHT_NONE || gamma > 0.f, "min-snr gamma %g is not > 0",
             (double)gamma);
  VD_REQUIRE(B > 0 && B <= 65535 && P > 0 && T > 0,
             "bad shape (B=%lld, per_sample=%lld, T=%lld)", (long long)B, (long long)P,
             (long long)T);
  return VD_OK;
}

}  // namespace

size_t vd_diffusion_loss_workspace_size(int64_t B, int64_t per_sample) {
  if (B <= 0 || per_sample <= 0) return 0;
  return (size_t)B * obj_blocks(per_sample) * sizeof(float);
}

int vd_diffusion_loss(const void* pred, const void* x0, const void* eps, const int64_t* t,
                      const float* sqrt_acp, const float* sqrt_1m_acp, int64_t T,
                      int prediction, int weighting, float gamma, int64_t B,
                      int64_t per_sample, int dtype, float* loss, float* per_sample_mse,
                      void* workspace, size_t workspace_bytes, void* stream) {
  const int rc = obj_check(pred, x0, eps, t, sqrt_acp, sqrt_1m_acp, T, prediction, weighting,
                           gamma, B, per_sample);
  if (rc != VD_OK) return rc;
  VD_REQUIRE(loss && per_sample_mse && workspace, "null output or workspace");
  VD_REQUIRE(workspace_bytes >= vd_diffusion_loss_workspace_size(B, per_sample),
             "workspace too small");
  const int nb = obj_blocks(per_sample);
  const int64_t chunk = obj_chunk(per_sample, nb);
  const dim3 grid((unsigned)nb, (unsigned)B);
  const Objective op{sqrt_acp, sqrt_1m_acp, t, T, weighting == VD_WEIGHT_MIN_SNR, gamma};
  float* part = static_cast<float*>(workspace);
  hipStream_t st = VD_STREAM(stream);
  const bool pv = prediction == VD_PRED_V;
  const bool v8 = obj_vec8(per_sample, {pred, pv ? x0 : nullptr, eps});
  return VD_DISPATCH_DTYPE(dtype, Tp, {
    const Tp* p = (const Tp*)pred;
    const Tp* x = (const Tp*)x0;
    const Tp* e = (const Tp*)eps;
    if (pv) {
      if (v8)
        obj_partial_kernel<Tp, 8, true><<<grid, kBlock, 0, st>>>(op, p, x, e, per_sample, chunk,
                                                                 part);
      else
        obj_partial_kernel<Tp, 1, true><<<grid, kBlock, 0, st>>>(op, p, x, e, per_sample, chunk,
                                                                 part);
      obj_finish_kernel<true><<<1, kBlock, 0, st>>>(op, part, nb, B, per_sample, per_sample_mse,
                                                    loss);
    } else {
      if (v8)
        obj_partial_kernel<Tp, 8, false><<<grid, kBlock, 0, st>>>(op, p, x, e, per_sample, chunk,
                                                                  part);
      else
        obj_partial_kernel<Tp, 1, false><<<grid, kBlock, 0, st>>>(op, p, x, e, per_sample, chunk,
                                                                  part);
      obj_finish_kernel<false><<<1, kBlock, 0, st>>>(op, part, nb, B, per_sample,
                                                     per_sample_mse, loss);
    }
  });
}

int vd_diffusion_loss_bwd(const void* pred, const void* x0, const void* eps, const int64_t* t,
                          const float* sqrt_acp, const float* sqrt_1m_acp, int64_t T,
                          int prediction, int weighting, float gamma, const float* grad_loss,
                          int64_t B, int64_t per_sample, int dtype, void* grad_pred,
                          void* stream) {
  const int rc = obj_check(pred, x0, eps, t, sqrt_acp, sqrt_1m_acp, T, prediction, weighting,
                           gamma, B, per_sample);
  if (rc != VD_OK) return rc;
  VD_REQUIRE(grad_loss && grad_pred, "null gradient argument");
  const Objective op{sqrt_acp, sqrt_1m_acp, t, T, weighting == VD_WEIGHT_MIN_SNR, gamma};
  const float scale = (float)(2.0 / ((double)B * (double)per_sample));
  hipStream_t st = VD_STREAM(stream);
  const bool pv = prediction == VD_PRED_V;
  const bool v8 = obj_vec8(per_sample, {pred, pv ? x0 : nullptr, eps, grad_pred});
  const int64_t work = vd_cdiv(per_sample / (v8 ? 8 : 1), kBlock);
  const int64_t cap = 256 * 16;  // 16 blocks per CU, then grid-stride
  const dim3 grid((unsigned)(work < cap ? (work > 0 ? work : 1) : cap), (unsigned)B);
  return VD_DISPATCH_DTYPE(dtype, Tp, {
    const Tp* p = (const Tp*)pred;
    const Tp* x = (const Tp*)x0;
    const Tp* e = (const Tp*)eps;
    Tp* g = (Tp*)grad_pred;
    if (pv) {
      if (v8)
        obj_bwd_kernel<Tp, 8, true><<<grid, kBlock, 0, st>>>(op, p, x, e, grad_loss, scale,
                                                             per_sample, g);
      else
        obj_bwd_kernel<Tp, 1, true><<<grid, kBlock, 0, st>>>(op, p, x, e, grad_loss, scale,
                                                             per_sample, g);
    } else {
      if (v8)
        obj_bwd_kernel<Tp, 8, false><<<grid, kBlock, 0, st>>>(op, p, x, e, grad_loss, scale,
                                                              per_sample, g);
      else
        obj_bwd_kernel<Tp, 1, false><<<grid, kBlock, 0, st>>>(op, p, x, e, grad_loss, scale,
                                                              per_sample, g);
    }
  });
}
