// gradclip.hip -- gradient clipping by global L2 norm over a descriptor table of fp32 ranges
// (torch.nn.utils.clip_grad_norm_'s result, built to the rules of vd_mse_loss / vd_cfg_stats:
// fixed summation order, no atomics, no memset, no semaphore, no cross-block communication
// inside a launch, every scalar read on the device -- the same bits eager and replayed from a
// HIP graph).
//
// The host cuts every gradient tensor into ranges (one vd_grad_desc each, as vd_ema_update's
// table); blocks walk the table grid-stride, one range per block at a time, so every element
// belongs to exactly one (descriptor, lane) and no result depends on the grid.
//
// Three launches:
//   1. grad_sumsq_kernel   partial[i] = sum of squares of range i                (vd_grad_sumsq)
//   2. grad_finish_kernel  one block: total of the partials, norm, coef -> record (vd_grad_clip)
//   3. grad_scale_kernel   g *= coef where coef < 1, coef read from the record   (vd_grad_clip)
//
// Summation layout of a partial (kBlock lanes, kVec elements per vector):
//   a range whose pointer is 16-B aligned has nv = n / kVec whole vectors; lane l takes vectors
//   l, l + kBlock, l + 2 kBlock, ... and adds the kVec squares of each in element order with
//   one fused multiply-add per element (s = fma(x, x, s), one rounding); the n - kVec nv tail
//   elements go to lanes 0, 1, ... one each (l, l + kBlock, ... in general), appended to the
//   lane's chain.  Any other range has nv = 0: lane l takes elements l, l + kBlock, ...
//   Then the LDS tree of mse_partial_kernel: log2(kBlock) rounds, lane l += lane l + w for
//   w = kBlock / 2 ... 1.
//
// How the total is combined: a ONE-BLOCK FINISH LAUNCH that writes device scalars, not every
// block of the scaling launch re-adding the partials as cfg_factor does.  cfg_factor re-adds at
// most 128 partials; here a model has thousands of ranges (13 452 on the config-2 list), so
// 2048 blocks re-adding them would read about as many bytes from L2 as the gradient pass reads
// from HBM.  The finish block adds the partials in fp64: lane l takes partials l, l + kBlock, ...
// in index order, then the same tree in fp64 -- one fixed order, independent of any grid, and
// its roundings (2^-53) leave the error bound to the partials alone.  norm = (float) sqrt(total),
// coef = min(1, max_norm / (norm + 1e-6f)) in fp32 (torch's clip_grad_norm_ formula); a
// non-finite norm (a NaN or Inf gradient, or squares that overflow fp32: nothing is rescaled
// away) records coef = 1.  The scaling launch reads coef from the record, which the finish
// launch wrote earlier on the same stream; coef == 1 returns before any load, so "measure
// only" (max_norm = +inf) and unclipped steps cost the read of the gradients once.
#include "vd_common.h"
#include <math.h>

namespace {

constexpr int kBlock = 256;  // lanes per block
constexpr int kVec = 8;      // elements per lane and vector (two 16-B accesses)
constexpr int kMaxGrid = 2048;  // 8 blocks per CU, then grid-stride

__global__ void __launch_bounds__(kBlock) grad_sumsq_kernel(const vd_grad_desc* __restrict__ descs,
                                                            int n_desc,
                                                            float* __restrict__ partial) {
  __shared__ float red[kBlock];
  for (int i = blockIdx.x; i < n_desc; i += gridDim.x) {
    const vd_grad_desc d = descs[i];
    const int64_t nv = (reinterpret_cast<uintptr_t>(d.g) % 16 == 0) ? d.n / kVec : 0;
    float s = 0.f;
    for (int64_t v = threadIdx.x; v < nv; v += kBlock) {
      float x[kVec];
      load8(d.g + v * kVec, x);
#pragma unroll
      for (int k = 0; k < kVec; ++k) s = fmaf(x[k], x[k], s);
    }
    for (int64_t e = nv * kVec + threadIdx.x; e < d.n; e += kBlock) {
      const float x = d.g[e];
      s = fmaf(x, x, s);
    }
    red[threadIdx.x] = s;
    __syncthreads();
#pragma unroll
    for (int w = kBlock / 2; w > 0; w >>= 1) {
      if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
      __syncthreads();
    }
    if (threadIdx.x == 0) partial[i] = red[0];
    __syncthreads();  // red[0] is read before the next range overwrites it
  }
}

__global__ void __launch_bounds__(kBlock) grad_finish_kernel(const float* __restrict__ partial,
                                                             int n_desc, float max_norm,
                                                             float* __restrict__ record) {
  __shared__ double red[kBlock];
  double s = 0.0;
  for (int i = threadIdx.x; i < n_desc; i += kBlock) s += (double)partial[i];
  red[threadIdx.x] = s;
  __syncthreads();
#pragma unroll
  for (int w = kBlock / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const float norm = (float)sqrt(red[0]);
    float coef = 1.f;
    if (isfinite(norm)) coef = fminf(1.f, max_norm / (norm + 1e-6f));
    record[0] = norm;
    record[1] = coef;
  }
}

__global__ void __launch_bounds__(kBlock) grad_scale_kernel(const vd_grad_desc* __restrict__ descs,
                                                            int n_desc,
                                                            const float* __restrict__ record) {
  const float coef = record[1];
  if (!(coef < 1.f)) return;  // nothing to clip (or a non-finite norm): nothing is written
  for (int i = blockIdx.x; i < n_desc; i += gridDim.x) {
    const vd_grad_desc d = descs[i];
    const int64_t nv = (reinterpret_cast<uintptr_t>(d.g) % 16 == 0) ? d.n / kVec : 0;
    // no loop vectorisation: it paired the elements of two iterations for v_pk_mul_f32 and
    // then stored them with sixteen 4-byte stores instead of four 16-byte ones (the pass ran
    // at 0.46 of the copy rate)
#pragma clang loop vectorize(disable) interleave(disable)
    for (int64_t v = threadIdx.x; v < nv; v += kBlock) {
      float x[kVec];
      load8(d.g + v * kVec, x);
#pragma unroll
      for (int k = 0; k < kVec; ++k) x[k] *= coef;
      store8(d.g + v * kVec, x);
    }
    for (int64_t e = nv * kVec + threadIdx.x; e < d.n; e += kBlock) d.g[e] *= coef;
  }
}

inline int grid_for_descs(int n_desc) { return n_desc < kMaxGrid ? n_desc : kMaxGrid; }

}  // namespace

extern "C" {

size_t vd_grad_clip_workspace_size(int n_desc) {
  return n_desc > 0 ? (size_t)n_desc * sizeof(float) : 0;
}

int vd_grad_sumsq(const vd_grad_desc* descs, int n_desc, void* workspace, size_t workspace_bytes,
                  void* stream) {
  VD_REQUIRE(descs && workspace, "null argument");
  VD_REQUIRE(n_desc > 0, "empty descriptor table (n_desc=%d)", n_desc);
  VD_REQUIRE(workspace_bytes >= vd_grad_clip_workspace_size(n_desc),
             "workspace %zu < %zu bytes", workspace_bytes, vd_grad_clip_workspace_size(n_desc));
  grad_sumsq_kernel<<<grid_for_descs(n_desc), kBlock, 0, VD_STREAM(stream)>>>(
      descs, n_desc, static_cast<float*>(workspace));
  return vd::check_launch("vd_grad_sumsq");
}

int vd_grad_clip(const vd_grad_desc* descs, int n_desc, const void* workspace, float max_norm,
                 float* record, void* stream) {
  VD_REQUIRE(descs && workspace && record, "null argument");
  VD_REQUIRE(n_desc > 0, "empty descriptor table (n_desc=%d)", n_desc);
  VD_REQUIRE(max_norm > 0.f, "max_norm = %g: must be > 0 (+inf: measure only)", (double)max_norm);
  hipStream_t st = VD_STREAM(stream);
  grad_finish_kernel<<<1, kBlock, 0, st>>>(static_cast<const float*>(workspace), n_desc, max_norm,
                                           record);
  grad_scale_kernel<<<grid_for_descs(n_desc), kBlock, 0, st>>>(descs, n_desc, record);
  return vd::check_launch("vd_grad_clip");
}

}  // extern "C"
