// adam.hip -- the Adam / AdamW step over a descriptor table of fp32 ranges, with the
// learning-rate schedule, the per-tensor bias correction and the bad-step decision read and
// taken on the device (built to the rules of vd_ema_update / vd_grad_clip: fixed order, no
// atomics, no memset, no semaphore, no cross-block communication inside a launch, nothing read
// on the host -- the same bits eager and replayed from a HIP graph).
//
// The host cuts every parameter into ranges (one vd_adam_desc each: p, m, v, g, n and the
// tensor's index into the step-count array; the ranges of a tensor are consecutive rows).
// Blocks walk the table grid-stride, so every element belongs to exactly one (row, lane) and no
// result depends on the grid.
//
// Two launches:
//   1. adam_update_kernel   p, m, v of every range from g                     (grid-stride)
//   2. adam_advance_kernel  one block: step counts, the four state words, the record
// Both take the SAME decision from the same device words, which launch 1 never writes and
// launch 2 writes only after every lane of its one block has read them (a barrier):
//   skip  <=>  max_bad_run > 0 and (tripped_at >= 0 or loss non-finite or norm non-finite)
// A skipped launch 1 returns before any load of a range.
//
// Scalars, in fp64, once per block (lr_s and the constants) or once per change of the step count
// along the rows a block walks (bc1, bc2: per tensor, torch's per-parameter count), each then
// rounded to fp32 ONCE:
//   lr_s  = lr * warm(s) * decay(s)              s = applied
//   omb1  = fl(1 - beta1)    b2 = fl(beta2)    omb2 = fl(1 - beta2)
//   epsf  = fl(eps)          wdf = fl(wd)      keep = fl(1 - lr_s wd)
//   step  = fl(lr_s / bc1)   bc2s = fl(sqrt(bc2))         bc1 = 1 - beta1^t, bc2 = 1 - beta2^t
//
// Operation order per element, fp32, every line one IEEE operation with one rounding (fmaf is
// the fused multiply-add; contraction is switched off for this file, so nothing else fuses; the
// divide and the square root are hipcc's default correctly rounded ones, no fast-math flag):
//   L2 mode only:          g  = fmaf(wdf, p, g)
//                          d  = g - m
//                          m  = fmaf(omb1, d, m)
//                          a  = b2 * v
//                          gg = g * g
//                          v  = fmaf(omb2, gg, a)
//   decoupled mode only:   p  = p * keep
//                          r  = sqrtf(v)
//                          r  = r / bc2s
//                          r  = r + epsf
//                          u  = m / r
//                          p  = fmaf(-step, u, p)
// (torch's _fused_adam / _single_tensor_adam formula: eps is added after the division by
// sqrt(bc2), and lr / bc1 multiplies the quotient.)  wd == 0 runs neither mode's line.
//
// The hyperparameters are host values in the launch's arguments: a captured launch freezes them
// (capture again after changing one).  Everything that changes from step to step -- the counts,
// the schedule position, the loss, the norm -- is read from device memory.
#include "vd_common.h"
#include <math.h>

#pragma clang fp contract(off)

namespace {

constexpr int kBlock = 256;     // lanes per block
constexpr int kVec = 8;         // elements per lane and vector (two 16-B accesses per array)
constexpr int kMaxGrid = 2048;  // 8 blocks per CU, then grid-stride

enum { kPlain = 0, kDecoupled = 1, kL2 = 2 };

// state words
enum { kApplied = 0, kSkipped = 1, kRun = 2, kTripped = 3 };

__device__ __forceinline__ bool adam_skip(const vd_adam_hyper& h, const int64_t* state,
                                          const float* loss, const float* norm) {
  if (h.max_bad_run <= 0) return false;
  if (state[kTripped] >= 0) return true;
  if (loss && !isfinite(*loss)) return true;
  if (norm && !isfinite(*norm)) return true;
  return false;
}

// lr * warm(s) * decay(s) in fp64
__device__ __forceinline__ double adam_lr(const vd_adam_hyper& h, int64_t s) {
  const double W = (double)h.warmup_steps;
  double warm = 1.0;
  if (h.warmup_steps > 0) warm = fmin(1.0, ((double)s + 1.0) / W);
  double decay = 1.0;
  if (h.schedule != VD_LR_CONSTANT) {
    double q = ((double)s - W) / ((double)h.total_steps - W);
    q = fmin(fmax(q, 0.0), 1.0);
    const double r = h.min_ratio;
    if (h.schedule == VD_LR_COSINE)
      decay = r + (1.0 - r) * (1.0 + cos(M_PI * q)) * 0.5;
    else
      decay = r + (1.0 - r) * (1.0 - q);
  }
  return h.lr * warm * decay;
}

struct Consts {  // per block
  float omb1, b2, omb2, eps, wd, keep;
};
struct Bias {    // per step count
  float step, bc2s;
};

template <int MODE>
__device__ __forceinline__ void adam_elem(float& p, float& m, float& v, float g, const Consts& c,
                                          const Bias& b) {
  if (MODE == kL2) g = fmaf(c.wd, p, g);
  const float d = g - m;
  m = fmaf(c.omb1, d, m);
  const float a = c.b2 * v;
  const float gg = g * g;
  v = fmaf(c.omb2, gg, a);
  if (MODE == kDecoupled) p = p * c.keep;
  float r = sqrtf(v);
  r = r / b.bc2s;
  r = r + c.eps;
  const float u = m / r;
  p = fmaf(-b.step, u, p);
}

template <int MODE>
__global__ void __launch_bounds__(kBlock) adam_update_kernel(const vd_adam_desc* __restrict__ descs,
                                                             int n_desc, vd_adam_hyper h,
                                                             const int64_t* __restrict__ steps,
                                                             const int64_t* __restrict__ state,
                                                             const float* __restrict__ loss,
                                                             const float* __restrict__ norm) {
  if (adam_skip(h, state, loss, norm)) return;  // nothing is loaded, nothing is written
  const double lr_s = adam_lr(h, state[kApplied]);
  Consts c;
  c.omb1 = (float)(1.0 - h.beta1);
  c.b2 = (float)h.beta2;
  c.omb2 = (float)(1.0 - h.beta2);
  c.eps = (float)h.eps;
  c.wd = (float)h.weight_decay;
  c.keep = (float)(1.0 - lr_s * h.weight_decay);
  Bias b = {0.f, 1.f};
  int64_t t_cur = -1;
  for (int i = blockIdx.x; i < n_desc; i += gridDim.x) {
    const vd_adam_desc d = descs[i];
    const int64_t t = steps[d.tensor] + 1;
    if (t != t_cur) {  // uniform over the block; every tensor of a usual step has the same count
      t_cur = t;
      const double bc1 = 1.0 - pow(h.beta1, (double)t);
      const double bc2 = 1.0 - pow(h.beta2, (double)t);
      b.step = (float)(lr_s / bc1);
      b.bc2s = (float)sqrt(bc2);
    }
    const uintptr_t bits = reinterpret_cast<uintptr_t>(d.p) | reinterpret_cast<uintptr_t>(d.m) |
                           reinterpret_cast<uintptr_t>(d.v) | reinterpret_cast<uintptr_t>(d.g);
    const int64_t nv = (bits % 16 == 0) ? d.n / kVec : 0;
    // no loop vectorisation (gradclip.hip's note: it turned the 16-byte stores into 4-byte ones)
#pragma clang loop vectorize(disable) interleave(disable)
    for (int64_t k = threadIdx.x; k < nv; k += kBlock) {
      float p[kVec], m[kVec], v[kVec], g[kVec];
      load8(d.p + k * kVec, p);
      load8(d.m + k * kVec, m);
      load8(d.v + k * kVec, v);
      load8(d.g + k * kVec, g);
#pragma unroll
      for (int e = 0; e < kVec; ++e) adam_elem<MODE>(p[e], m[e], v[e], g[e], c, b);
      store8(d.p + k * kVec, p);
      store8(d.m + k * kVec, m);
      store8(d.v + k * kVec, v);
    }
    for (int64_t e = nv * kVec + threadIdx.x; e < d.n; e += kBlock) {
      float p = d.p[e], m = d.m[e], v = d.v[e];
      adam_elem<MODE>(p, m, v, d.g[e], c, b);
      d.p[e] = p;
      d.m[e] = m;
      d.v[e] = v;
    }
  }
}

__global__ void __launch_bounds__(kBlock) adam_advance_kernel(const vd_adam_desc* __restrict__ descs,
                                                              int n_desc, vd_adam_hyper h,
                                                              int64_t* steps, int64_t* state,
                                                              const float* loss, const float* norm,
                                                              float* lr_out, int64_t* skip_flag_out) {
  const bool skip = adam_skip(h, state, loss, norm);
  const int64_t applied = state[kApplied], skipped = state[kSkipped], run = state[kRun];
  const int64_t tripped = state[kTripped];
  __syncthreads();  // every lane holds the decision before lane 0 rewrites the words
  if (!skip) {
    // the first row of every tensor advances its count (a tensor's rows are consecutive)
    for (int i = threadIdx.x; i < n_desc; i += kBlock) {
      const int64_t t = descs[i].tensor;
      if (i == 0 || descs[i - 1].tensor != t) steps[t] += 1;
    }
  }
  if (threadIdx.x == 0) {
    const int64_t index = applied + skipped;  // this step's global index
    lr_out[0] = (float)adam_lr(h, applied);
    if (!skip) {
      state[kApplied] = applied + 1;
      state[kRun] = 0;
      skip_flag_out[0] = -1;
    } else {
      state[kSkipped] = skipped + 1;
      state[kRun] = run + 1;
      if (run + 1 > (int64_t)h.max_bad_run && tripped < 0) state[kTripped] = index;
      skip_flag_out[0] = index;
    }
  }
}

inline int grid_for_descs(int n_desc) { return n_desc < kMaxGrid ? n_desc : kMaxGrid; }

inline bool in_unit(double x) { return x >= 0.0 && x < 1.0; }  // false for NaN

}  // namespace

extern "C" {

int vd_adam_step(const vd_adam_desc* descs, int n_desc, const vd_adam_hyper* h, int64_t* steps,
                 int64_t* state, const float* loss, const float* grad_norm, float* lr_out,
                 int64_t* skip_flag_out, void* stream) {
  VD_REQUIRE(descs && h && steps && state && lr_out && skip_flag_out, "null argument");
  VD_REQUIRE(n_desc > 0, "empty descriptor table (n_desc=%d)", n_desc);
  VD_REQUIRE(in_unit(h->beta1) && in_unit(h->beta2), "betas (%g, %g): each in [0, 1)", h->beta1,
             h->beta2);
  VD_REQUIRE(h->eps > 0.0 && isfinite(h->eps), "eps = %g: must be > 0", h->eps);
  VD_REQUIRE(h->lr >= 0.0 && isfinite(h->lr), "lr = %g: must be >= 0", h->lr);
  VD_REQUIRE(h->weight_decay >= 0.0 && isfinite(h->weight_decay),
             "weight_decay = %g: must be >= 0", h->weight_decay);
  VD_REQUIRE(h->min_ratio >= 0.0 && h->min_ratio <= 1.0, "min_ratio = %g: outside [0, 1]",
             h->min_ratio);
  VD_REQUIRE(h->schedule == VD_LR_CONSTANT || h->schedule == VD_LR_COSINE ||
                 h->schedule == VD_LR_LINEAR,
             "unknown schedule %d", (int)h->schedule);
  VD_REQUIRE(h->warmup_steps >= 0, "warmup_steps = %lld: must be >= 0",
             (long long)h->warmup_steps);
  VD_REQUIRE(h->max_bad_run >= 0, "max_bad_run = %d: must be >= 0", (int)h->max_bad_run);
  VD_REQUIRE(h->schedule == VD_LR_CONSTANT || h->total_steps > h->warmup_steps,
             "total_steps = %lld <= warmup_steps = %lld with a decaying schedule",
             (long long)h->total_steps, (long long)h->warmup_steps);
  hipStream_t st = VD_STREAM(stream);
  const int grid = grid_for_descs(n_desc);
  if (h->weight_decay == 0.0)
    adam_update_kernel<kPlain><<<grid, kBlock, 0, st>>>(descs, n_desc, *h, steps, state, loss,
                                                        grad_norm);
  else if (h->decoupled)
    adam_update_kernel<kDecoupled><<<grid, kBlock, 0, st>>>(descs, n_desc, *h, steps, state, loss,
                                                            grad_norm);
  else
    adam_update_kernel<kL2><<<grid, kBlock, 0, st>>>(descs, n_desc, *h, steps, state, loss,
                                                     grad_norm);
  adam_advance_kernel<<<1, kBlock, 0, st>>>(descs, n_desc, *h, steps, state, loss, grad_norm,
                                            lr_out, skip_flag_out);
  return vd::check_launch("vd_adam_step");
}

}  // extern "C"
