// elementwise.hip -- HBM-bound wave-level kernels of the diffusion hot path:
// timestep embedding, DDPM scheduler math, classifier-free guidance, the DDIM / DPM-Solver++
// sampler step with its dynamic threshold, nearest upsampling, the MSE loss, conv glue and the
// weight EMA.
//
// Every tensor kernel moves 8 elements per lane (16 B for bf16, 2x16 B for
// fp32) when the per-sample length allows it, and gathers the per-sample
// schedule scalars from the fp32 tables on device (no host sync on t).
#include "vd_common.h"
#include <math.h>
#include <initializer_list>
#include <type_traits>

namespace {

constexpr int kBlock = 256;

inline int grid_for(int64_t work) {
  int64_t g = vd_cdiv(work, kBlock);
  const int64_t cap = 256 * 16;  // 16 blocks per CU, then grid-stride
  return (int)(g < cap ? (g > 0 ? g : 1) : cap);
}

// The one alignment rule of the per-sample kernels (scheduler math, guidance, DPM): the 8-wide
// path needs whole vectors per sample and every non-null pointer 16-B aligned; anything else
// runs one element at a time.
inline bool cfg_vec8(int64_t per_sample, std::initializer_list<const void*> ptrs) {
  uintptr_t a = 0;
  for (const void* p : ptrs) a |= reinterpret_cast<uintptr_t>(p);
  return per_sample % 8 == 0 && a % 16 == 0;
}

// ------------------------------------------------------------ timestep embedding
// freqs: the caller's table (nullptr: computed here)
__global__ void temb_kernel(const int64_t* __restrict__ t, int B, int dim, float log_max_period,
                            const float* __restrict__ freqs, float* __restrict__ out) {
  const int half = dim / 2;
  const int n = B * dim;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const int b = i / dim, j = i % dim;
    float v = 0.f;
    if (j < 2 * half) {
      const int f = j < half ? j : j - half;
      // utils.py:150-152: exp(-ln(max_period) * arange(half) / half) in fp32
      const float freq = freqs ? freqs[f] : expf(-log_max_period * (float)f / (float)half);
      const float arg = (float)t[b] * freq;
      v = j < half ? cosf(arg) : sinf(arg);
    }
    out[i] = v;
  }
}

// ------------------------------------------------------------ scheduler math
// A per-element op sees (b, scalars) and 8-wide vectors of its inputs.
struct QSample {
  const float *sa, *s1m;
  __device__ void operator()(int64_t tb, const float* xa, const float* xb, const float*,
                             float* o0, float*, int n) const {
    const float a = sa[tb], c = s1m[tb];
    for (int i = 0; i < n; ++i) o0[i] = a * xa[i] + c * xb[i];
  }
};

struct PSampleV1 {
  const float *betas, *alphas, *acp, *s1m;
  __device__ void operator()(int64_t tb, const float* xt, const float* eps, const float* z,
                             float* xprev, float* x0, int n) const {
    const float s1 = s1m[tb];
    const float sq_acp = sqrtf(acp[tb]);
    const float beta = betas[tb];
    const float sq_alpha = sqrtf(alphas[tb]);
    float sigma = 0.f;
    if (tb > 0) sigma = sqrtf((1.f - acp[tb - 1]) / (1.f - acp[tb]) * beta);
    for (int i = 0; i < n; ++i) {
      float x = (xt[i] - s1 * eps[i]) / sq_acp;
      x0[i] = fminf(fmaxf(x, -1.f), 1.f);
      float mean = (xt[i] - (beta * eps[i]) / s1) / sq_alpha;
      xprev[i] = tb > 0 ? mean + sigma * z[i] : mean;
    }
  }
};

struct PSampleV2 {
  const float *betas, *alphas, *acp, *sa, *s1m;
  __device__ void operator()(int64_t tb, const float* xt, const float* eps, const float* z,
                             float* xprev, float* x0, int n) const {
    const float s1 = s1m[tb];
    const float sq_alpha = sqrtf(alphas[tb]);
    const float sigma = sqrtf((1.f - acp[tb]) * betas[tb]);
    const float a = sa[tb];
    for (int i = 0; i < n; ++i) {
      float mean = xt[i] - (s1 * eps[i]) / sq_alpha;
      xprev[i] = mean + sigma * z[i];
      float x = (xt[i] - s1 * eps[i]) / a;
      x0[i] = fminf(fmaxf(x, -1.f), 1.f);
    }
  }
};

struct PSampleCos {
  const float *acp, *sa, *s1m;
  __device__ void operator()(int64_t tb, const float* xt, const float* eps, const float* z,
                             float* xprev, float* mean_out, int n) const {
    const float s1 = s1m[tb], a = sa[tb];
    float sigma = 0.f;
    if (tb > 0) sigma = sqrtf(acp[tb - 1] * (1.f - acp[tb]) / (1.f - acp[tb - 1]));
    for (int i = 0; i < n; ++i) {
      float mean = (xt[i] - s1 * eps[i]) / a;
      mean_out[i] = mean;
      xprev[i] = tb > 0 ? mean + sigma * z[i] : mean;
    }
  }
};

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

// Generic 3-in / 2-out per-sample op.  VEC = 8 under cfg_vec8's rule.
template <typename T, typename Op, int VEC>
__global__ void sched_kernel(Op op, const T* __restrict__ a, const T* __restrict__ b,
                             const T* __restrict__ c, T* __restrict__ o0, T* __restrict__ o1,
                             const int64_t* __restrict__ t, int64_t B, int64_t per_sample) {
  const int64_t nvec = B * per_sample / VEC;
  for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < nvec;
       v += (int64_t)gridDim.x * blockDim.x) {
    const int64_t e = v * VEC;
    const int64_t bi = e / per_sample;
    float xa[8], xb[8], xc[8] = {0, 0, 0, 0, 0, 0, 0, 0}, y0[8], y1[8];
    ld_vec(a + e, xa, VEC);
    ld_vec(b + e, xb, VEC);
    if (c) ld_vec(c + e, xc, VEC);
    op(t[bi], xa, xb, xc, y0, y1, VEC);
    st_vec(o0 + e, y0, VEC);
    if (o1) st_vec(o1 + e, y1, VEC);
  }
}

template <typename Op>
int launch_sched(Op op, const void* a, const void* b, const void* c, void* o0, void* o1,
                 const int64_t* t, int64_t B, int64_t per_sample, int dtype, void* stream) {
  VD_REQUIRE(a && b && o0 && t, "null tensor argument");
  VD_REQUIRE(B > 0 && per_sample > 0, "empty tensor (B=%lld, per_sample=%lld)", (long long)B,
             (long long)per_sample);
  const bool v8 = cfg_vec8(per_sample, {a, b, c, o0, o1});
  const int64_t work = B * per_sample / (v8 ? 8 : 1);
  return VD_DISPATCH_DTYPE(dtype, T, {
    if (v8)
      sched_kernel<T, Op, 8><<<grid_for(work), kBlock, 0, VD_STREAM(stream)>>>(
          op, (const T*)a, (const T*)b, (const T*)c, (T*)o0, (T*)o1, t, B, per_sample);
    else
      sched_kernel<T, Op, 1><<<grid_for(work), kBlock, 0, VD_STREAM(stream)>>>(
          op, (const T*)a, (const T*)b, (const T*)c, (T*)o0, (T*)o1, t, B, per_sample);
  });
}

// ------------------------------------------------------------ upsample
template <typename T, int VEC>
__global__ void upsample_kernel(const T* __restrict__ x, T* __restrict__ y, int64_t BT, int H,
                                int W, int C) {
  const int cv = C / VEC;
  const int64_t n = BT * H * W * cv;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int c0 = (int)(i % cv) * VEC;
    int64_t p = i / cv;
    const int w = (int)(p % W);
    p /= W;
    const int h = (int)(p % H);
    const int64_t bt = p / H;
    float v[8];
    ld_vec(x + i * VEC, v, VEC);
    const int64_t W2 = 2 * W;
    const int64_t row0 = ((bt * 2 * H + 2 * h) * W2 + 2 * w) * C + c0;
    st_vec(y + row0, v, VEC);
    st_vec(y + row0 + C, v, VEC);
    st_vec(y + row0 + W2 * C, v, VEC);
    st_vec(y + row0 + W2 * C + C, v, VEC);
  }
}

template <typename T, int VEC>
__global__ void upsample_bwd_kernel(const T* __restrict__ dy, T* __restrict__ dx, int64_t BT,
                                    int H, int W, int C) {
  const int cv = C / VEC;
  const int64_t n = BT * H * W * cv;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int c0 = (int)(i % cv) * VEC;
    int64_t p = i / cv;
    const int w = (int)(p % W);
    p /= W;
    const int h = (int)(p % H);
    const int64_t bt = p / H;
    const int64_t W2 = 2 * W;
    const int64_t row0 = ((bt * 2 * H + 2 * h) * W2 + 2 * w) * C + c0;
    float a[8], b[8], c[8], d[8], s[8];
    ld_vec(dy + row0, a, VEC);
    ld_vec(dy + row0 + C, b, VEC);
    ld_vec(dy + row0 + W2 * C, c, VEC);
    ld_vec(dy + row0 + W2 * C + C, d, VEC);
    for (int k = 0; k < VEC; ++k) s[k] = (a[k] + b[k]) + (c[k] + d[k]);
    st_vec(dx + i * VEC, s, VEC);
  }
}

// ------------------------------------------------------------ MSE loss (train.py:103, 130)
// Fixed-order two-launch reduction: mse_partial_kernel sums a fixed contiguous range per
// block (8 elements per lane, a lane's sum, then an LDS tree) into partial[block];
// mse_finish_kernel (one block) sums the partials in block order and scales by 1/n.  No
// semaphore, no memset, no cross-block communication inside a launch: the same bits every
// run, eager or replayed from a HIP graph (torch's one-launch multi-block
// mean -- a hipMemsetAsync'd semaphore plus a last-block combine -- returned stale values
// when replayed under HIP's graph packet capture).
constexpr int kMseBlocks = 1024;

inline int mse_blocks(int64_t n) {
  const int64_t per = (int64_t)kBlock * 8;
  const int64_t g = vd_cdiv(n, per);
  return (int)(g < kMseBlocks ? (g > 0 ? g : 1) : kMseBlocks);
}

template <typename T>
__global__ void __launch_bounds__(kBlock) mse_partial_kernel(
    const T* __restrict__ pred, const T* __restrict__ tgt, int64_t n, int64_t chunk,
    float* __restrict__ partial) {
  __shared__ float red[kBlock];
  const int64_t lo = (int64_t)blockIdx.x * chunk;
  const int64_t hi = lo + chunk < n ? lo + chunk : n;
  float s = 0.f;
  // chunk is a multiple of 8: every 8-vector lies in one block's range
  for (int64_t i = lo + (int64_t)threadIdx.x * 8; i < hi; i += (int64_t)kBlock * 8) {
    if (i + 8 <= hi) {
      float a[8], b[8];
      load8(pred + i, a);
      load8(tgt + i, b);
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const float d = a[k] - b[k];
        s = fmaf(d, d, s);
      }
    } else {
      for (int64_t j = i; j < hi; ++j) {
        const float d = Elem<T>::ld(pred + j) - Elem<T>::ld(tgt + j);
        s = fmaf(d, d, s);
      }
    }
  }
  red[threadIdx.x] = s;
  __syncthreads();
#pragma unroll
  for (int w = kBlock / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) partial[blockIdx.x] = red[0];
}

__global__ void __launch_bounds__(kBlock) mse_finish_kernel(const float* __restrict__ partial,
                                                            int nblocks, float inv_n,
                                                            float* __restrict__ out) {
  __shared__ float red[kBlock];
  float s = 0.f;
  for (int i = threadIdx.x; i < nblocks; i += kBlock) s += partial[i];
  red[threadIdx.x] = s;
  __syncthreads();
#pragma unroll
  for (int w = kBlock / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) *out = red[0] * inv_n;
}

// d loss / d pred = 2 (pred - tgt) / n * g, g = the loss gradient (a device scalar)
template <typename T>
__global__ void __launch_bounds__(kBlock) mse_bwd_kernel(
    const T* __restrict__ pred, const T* __restrict__ tgt, const float* __restrict__ gout,
    float scale, int64_t n, T* __restrict__ gpred) {
  const float c = scale * *gout;
  const int64_t nv = n / 8;
  for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < nv;
       v += (int64_t)gridDim.x * blockDim.x) {
    float a[8], b[8];
    load8(pred + 8 * v, a);
    load8(tgt + 8 * v, b);
#pragma unroll
    for (int k = 0; k < 8; ++k) a[k] = c * (a[k] - b[k]);
    store8(gpred + 8 * v, a);
  }
  for (int64_t j = nv * 8 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n;
       j += (int64_t)gridDim.x * blockDim.x)
    Elem<T>::st(gpred + j, c * (Elem<T>::ld(pred + j) - Elem<T>::ld(tgt + j)));
}

// ------------------------------------------------------------ classifier-free audio guidance
// eps = f_b * g with g = u + w (c - u) (c / u: the denoiser's noise with / without the audio)
// and, with rescale = phi > 0, f_b = phi sqrt(SS(c) / SS(g)) + (1 - phi) per sample,
// SS(x) = sum (x_i - mean(x))^2: the std-rescale of Lin et al. 2023 (the n - 1 of the unbiased
// std cancels in the ratio).  Statistics (vd_cfg_stats): a fixed-order two-pass reduction over
// the caller's workspace [B][nb][4] fp32.  Block k of sample b owns one fixed contiguous range
// (a multiple of 8 elements, the last one ragged).  cfg_sum_kernel writes its sums of c and g
// to slots 0 / 1; the centred pass adds the sample's nb sums (lane k holds partial k, then the
// same fixed LDS tree: every block the same adds, so the same mean bits), and writes its sums
// of (c - mean_c)^2 and (g - mean_g)^2 to slots 2 / 3 -- centred, so a sample with |mean| >>
// sigma loses nothing to cancellation as sum x^2 - (sum x)^2 / P would.  The consumers
// (cfg_factor) add slots 2 / 3 the same way.
// No atomics, no memset, no semaphore, no cross-block communication inside a launch: the same
// bits every run, eager or replayed from a HIP graph (torch's one-launch
// multi-block reductions -- torch.std is one -- use a hipMemsetAsync'd semaphore plus a
// last-block combine, which returned stale values when replayed under HIP's graph packet
// capture).
constexpr int kCfgBlocks = 128;  // partials per sample (upper bound; one per lane of a block)
static_assert(kCfgBlocks <= kBlock, "cfg_partial_sums: one partial per lane");

inline int cfg_blocks(int64_t P) {
  const int64_t g = vd_cdiv(P, (int64_t)kBlock * 8);
  return (int)(g < kCfgBlocks ? (g > 0 ? g : 1) : kCfgBlocks);
}
inline int64_t cfg_chunk(int64_t P, int nb) { return vd_cdiv(vd_cdiv(P, nb), 8) * 8; }

// The guided noise of n elements, shared by the statistics and by both consumers.
struct CfgGuide {
  float w;
  __device__ __forceinline__ void run(const float* c, const float* u, float f, bool scale,
                                      float* g, int n) const {
    for (int i = 0; i < n; ++i) {
      const float v = fmaf(w, c[i] - u[i], u[i]);
      g[i] = scale ? f * v : v;
    }
  }
};

// both lanes' values summed by the LDS tree of mse_partial_kernel; the result in red[.][0]
__device__ __forceinline__ void cfg_block_sum2(float (&red)[2][kBlock], float a, float b) {
  red[0][threadIdx.x] = a;
  red[1][threadIdx.x] = b;
  __syncthreads();
#pragma unroll
  for (int w = kBlock / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) {
      red[0][threadIdx.x] += red[0][threadIdx.x + w];
      red[1][threadIdx.x] += red[1][threadIdx.x + w];
    }
    __syncthreads();
  }
}

// The sample's nb partials of slots `slot` and `slot + 1` summed: lane k takes partial k (one
// load per lane instead of a serial walk), then the fixed tree.  Ends with a barrier: red is
// free again.
__device__ __forceinline__ void cfg_partial_sums(float (&red)[2][kBlock], const float* row,
                                                 int nb, int slot, float& a, float& b) {
  float pa = 0.f, pb = 0.f;
  if ((int)threadIdx.x < nb) {
    pa = row[threadIdx.x * 4 + slot];
    pb = row[threadIdx.x * 4 + slot + 1];
  }
  cfg_block_sum2(red, pa, pb);
  a = red[0][0];
  b = red[1][0];
  __syncthreads();
}

// CENTRED = false: slots 0 / 1 = sum c, sum g; true: slots 2 / 3 = centred sums of squares.
// VEC = 8 needs per_sample % 8 == 0 (then every range is whole 8-vectors) and 16-B alignment.
template <typename T, int VEC, bool CENTRED>
__global__ void __launch_bounds__(kBlock) cfg_stats_kernel(const T* __restrict__ c,
                                                           const T* __restrict__ u, CfgGuide op,
                                                           int64_t P, int64_t chunk, float* part) {
  __shared__ float red[2][kBlock];
  const int nb = gridDim.x;
  const int64_t b = blockIdx.y;
  float* row = part + b * nb * 4;
  float mc = 0.f, mg = 0.f;
  if (CENTRED) {
    cfg_partial_sums(red, row, nb, 0, mc, mg);
    mc /= (float)P;
    mg /= (float)P;
  }
  const int64_t lo = (int64_t)blockIdx.x * chunk;
  const int64_t hi = lo + chunk < P ? lo + chunk : P;
  const T* cb = c + b * P;
  const T* ub = u + b * P;
  float sc = 0.f, sg = 0.f;
  for (int64_t i = lo + (int64_t)threadIdx.x * VEC; i < hi; i += (int64_t)kBlock * VEC) {
    float xc[8], xu[8], g[8];
    ld_vec(cb + i, xc, VEC);
    ld_vec(ub + i, xu, VEC);
    op.run(xc, xu, 1.f, false, g, VEC);
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      if (CENTRED) {
        const float dc = xc[k] - mc, dg = g[k] - mg;
        sc = fmaf(dc, dc, sc);
        sg = fmaf(dg, dg, sg);
      } else {
        sc += xc[k];
        sg += g[k];
      }
    }
  }
  cfg_block_sum2(red, sc, sg);
  if (threadIdx.x == 0) {
    row[blockIdx.x * 4 + (CENTRED ? 2 : 0)] = red[0][0];
    row[blockIdx.x * 4 + (CENTRED ? 3 : 1)] = red[1][0];
  }
}

// f_b from the sample's partials, added in the fixed order of cfg_partial_sums: every block of
// a sample, in either consumer, gets the same bits.  Called by all kBlock threads of a block.
// A constant guided noise (SS(g) = 0: the all-zero eps of a freshly initialised model, whose
// output conv is zero) has no std to match; it is left as it is, f_b = 1, where the formula's
// 0 / 0 would turn the whole sample into NaN.
__device__ __forceinline__ float cfg_factor(const float* __restrict__ part, int64_t b, int nb,
                                            float phi) {
  __shared__ float red[2][kBlock];
  float qc, qg;
  cfg_partial_sums(red, part + b * nb * 4, nb, 2, qc, qg);
  if (qg == 0.f) return 1.f;
  return phi * sqrtf(qc / qg) + (1.f - phi);
}

// The model output of one vector, shared by every consumer (the combine, the sampler step, the
// x0 histogram): c as it is, or, guided, CfgGuide::run(c, u, f, scale).  `guided` is a constant
// where the caller knows it: a test of the pointer itself would hold u's load back behind c's.
template <typename T, int VEC>
__device__ __forceinline__ void model_out(const T* c, const T* u, bool guided, const CfgGuide& gd,
                                          float f, bool scale, float (&m)[8]) {
  float xc[8];
  ld_vec(c, xc, VEC);
  if (guided) {
    float xu[8];
    ld_vec(u, xu, VEC);
    gd.run(xc, xu, f, scale, m, VEC);
  } else {
#pragma unroll
    for (int k = 0; k < VEC; ++k) m[k] = xc[k];
  }
}

// The guided noise written out (the DDPM p_sample_* kernels take it as their eps).
template <typename T, int VEC>
__global__ void __launch_bounds__(kBlock) cfg_combine_kernel(
    CfgGuide gd, const T* __restrict__ c, const T* __restrict__ u, T* __restrict__ out,
    const float* __restrict__ part, int nb, float phi, int64_t per_sample) {
  const int64_t b = blockIdx.y;
  const bool scale = phi > 0.f;
  const float f = scale ? cfg_factor(part, b, nb, phi) : 1.f;
  const int64_t base = b * per_sample;
  const int64_t nvec = per_sample / VEC;
  for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < nvec;
       v += (int64_t)gridDim.x * blockDim.x) {
    const int64_t e = base + v * VEC;
    float g[8];
    model_out<T, VEC>(c + e, u + e, true, gd, f, scale, g);
    st_vec(out + e, g, VEC);
  }
}

// One block column per sample: sample b is row b % 65535 of layer b / 65535 (a grid has at most
// 65535 rows; the entry points that check B <= 65535 launch one layer).
constexpr int64_t kGridRows = 65535;
inline dim3 cfg_grid(int64_t per_sample, int vec, int64_t B) {
  return dim3((unsigned)grid_for(per_sample / vec), (unsigned)(B < kGridRows ? B : kGridRows),
              (unsigned)vd_cdiv(B, kGridRows));
}

// ------------------------------------------------------------ sampler step (DDIM, DPM-Solver++)
// A rule is two per-element pieces, x0 from (xt, model output) and x_prev from (xt, x0,
// direction term, third input), and carries its scalars: sample_x0(b) takes those of the x0
// piece (all the x0 histogram needs), sample(b) those of both.
//
// DDIM (Song et al. 2021): x0 = (xt - sqrt(1 - a_t) eps) / sqrt(a_t), x_prev = sqrt(a_p) x0 +
// dir eps (+ sigma z), a_t = acp[t[b]], a_p = acp[t_prev[b]] (1 for t_prev = -1).  PRED_V: the
// model output is v (Salimans & Ho 2022): x0 = sqrt(a_t) xt - sqrt(1 - a_t) v, and the direction
// term is eps = sqrt(1 - a_t) xt + sqrt(a_t) v.  A clamped or thresholded x0 leaves the direction
// term the model's own.  The third input is z, read when it is given.
struct DDIMScalars {
  const float* acp;
  const int64_t *t, *tprev;
  float eta;
  int has_z;
  float at, sq_at, sq_1mat, sigma, dir, sq_ap;
  __device__ __forceinline__ void sample_x0(int64_t b) {
    at = acp[t[b]];
    sq_at = sqrtf(at), sq_1mat = sqrtf(1.f - at);
  }
  __device__ __forceinline__ void sample(int64_t b) {
    sample_x0(b);
    const int64_t tp = tprev[b];
    const float ap = tp >= 0 ? acp[tp] : 1.f;
    sigma = eta * sqrtf((1.f - ap) / (1.f - at) * (1.f - at / ap));
    dir = sqrtf(fmaxf(1.f - ap - sigma * sigma, 0.f));
    sq_ap = sqrtf(ap);
  }
  __device__ __forceinline__ bool third() const { return has_z; }
  // e_k: the direction a perfect denoiser would give at a known x0 (masked step)
  __device__ __forceinline__ float direction_known(float xt, float xk) const {
    return (xt - sq_at * xk) / sq_1mat;
  }
  __device__ __forceinline__ float x_prev(float, float x0, float e, float z) const {
    float v = sq_ap * x0 + dir * e;
    if (has_z) v += sigma * z;
    return v;
  }
};
template <bool PRED_V>
struct DDIMRule : DDIMScalars {
  __device__ __forceinline__ float x0(float xt, float m) const {
    if constexpr (PRED_V)
      return sq_at * xt - sq_1mat * m;
    else
      return (xt - sq_1mat * m) / sq_at;
  }
  __device__ __forceinline__ float direction(float xt, float m) const {
    if constexpr (PRED_V)
      return sq_1mat * xt + sq_at * m;
    else
      return m;
  }
};

// DPM-Solver++(2M): x0 = (xt - sigma_t eps) / alpha_t, x_prev = A xt + B x0 + C x0_last, with
// the row [alpha_t, sigma_t, A, B, C, 0, 0, 0] of the host's fp32 table picked by a device
// scalar: the launch arguments never change, so a captured graph replays for every step.  The
// row is uniform across the launch.  The third input is the history, x0_last; C == 0 (the
// first-order rows and the last one): it is not read -- at step 0 it is uninitialised, and
// 0 * NaN is NaN.  x_prev is formed from the fp32 x0, not from the value a bf16 history rounds
// it to.
struct DPMRule {
  const float* coef;
  int64_t n_steps;
  const int64_t* step;
  float alpha, sigma, A, B, C;
  __device__ __forceinline__ void sample_x0(int64_t) {
    int64_t s = *step;
    s = s < 0 ? 0 : (s > n_steps - 1 ? n_steps - 1 : s);
    const float* r = coef + s * 8;
    alpha = r[0], sigma = r[1], A = r[2], B = r[3], C = r[4];
  }
  __device__ __forceinline__ void sample(int64_t b) { sample_x0(b); }
  __device__ __forceinline__ bool third() const { return C != 0.f; }
  __device__ __forceinline__ float x0(float xt, float m) const { return (xt - sigma * m) / alpha; }
  __device__ __forceinline__ float direction(float, float m) const { return m; }
  __device__ __forceinline__ float direction_known(float, float) const { return 0.f; }  // unused
  __device__ __forceinline__ float x_prev(float xt, float x0, float, float last) const {
    float v = A * xt + B * x0;
    if (C != 0.f) v += C * last;
    return v;
  }
};

// The one step kernel: model output (guided and std-rescaled when GUIDED) -> x0 -> static clamp
// (clip) or, THR, the dynamic threshold x0 = clamp(x0, -s, s) / s with the sample's s = thr[b]
// >= 1 of vd_x0_abs_quantile -> x_prev.  Reads xt, c (u) and the rule's third input (z | the
// history); writes x_prev, xdup (the same values: the graph sampler's doubled-batch input) and x0,
// the latter two when given.  A block works on one sample (cfg_grid), so it takes the sample's
// scalars, f_b and s_b once, from scalar loads ahead of every store.
// Aliasing: x_prev may be xt, and the DPM history arrives as both `third` and `x0o`, read and
// written in place: a lane reads its elements before it writes them and no other lane touches
// them, so xt, third, xprev, xdup and x0o carry no __restrict__.
//
// KNOWN (masked sampling): after the clamp or the threshold, x0 is replaced by the known clip
// x_k where keep says so.  keep is fp32 [Bk][S], Bk in {1, B}, S a divisor of per_sample: element
// i of a sample reads keep[i % S], so one mask row serves every channel (and, Bk = 1, every
// sample).  k <= 0: x0 and the direction term are the model's, the expressions and bits of the
// unmasked step; k >= 1: x0 = x_k and the direction becomes the rule's direction_known -- both
// selects, so a non-finite model output there reaches no output; in between both are blended,
// (1 - k) y + k x_k.  x_k is never clamped or divided by the threshold.  The step runs 8-wide
// exactly where the unmasked step does (cfg_vec8, known and keep among the pointers): its k <= 0
// bits are the unmasked kernel's only at the same width, whose instantiations do not all fuse the
// same products.  The mask index is one remainder per vector; with S % 8 == 0 the vector lies
// inside one channel and its eight mask values are one vector load, otherwise they are read one
// element at a time.
// known and keep are inputs only and alias no output.  KNOWN = false: `kn` is empty and unread.
// Every vector is first stepped and stored unmasked; one that holds a kept element is then
// formed again and stored over it (the comment in the kernel says why).
__device__ __forceinline__ float opaque(float v) {
  asm volatile("" : "+v"(v));  // no instruction: the value, as one the optimiser knows nothing of
  return v;
}

template <typename T, bool KNOWN>
struct KnownOps {};
template <typename T>
struct KnownOps<T, true> {
  const T* known;
  const float* keep;
  int64_t S, row;  // row: keep's sample stride, 0 (Bk = 1) or S
};

template <typename T, int VEC, typename Rule, bool THR, bool GUIDED, bool KNOWN>
__global__ void __launch_bounds__(kBlock) step_kernel(
    Rule rule, CfgGuide gd, const T* xt, const T* __restrict__ c, const T* __restrict__ u,
    const T* third, T* xprev, T* xdup, T* x0o, const float* __restrict__ part, int nb, float phi,
    const float* __restrict__ thr, int clip, int64_t B, int64_t per_sample,
    KnownOps<T, KNOWN> kn) {
  // The sample: the row, strided over the grid's rows by the layer (cfg_grid).  A row past B (the
  // last layer's) takes the last sample's scalars and an empty range: an early return would hold
  // every other argument's load back behind B's.
  const int64_t row = blockIdx.y + (int64_t)blockIdx.z * gridDim.y;
  const int64_t b = row < B ? row : B - 1;
  // the rule's scalars first: their dependent loads run beside the sum of f_b's partials
  rule.sample(b);
  const bool has3 = rule.third();
  const float s = THR ? thr[b] : 1.f;
  const bool scale = GUIDED && phi > 0.f;
  const float f = scale ? cfg_factor(part, b, nb, phi) : 1.f;
  const int64_t base = b * per_sample;
  const int64_t nvec = row < B ? per_sample / VEC : 0;
  for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < nvec;
       v += (int64_t)gridDim.x * blockDim.x) {
    const int64_t e = base + v * VEC;
    float xa[8], m[8], x3[8] = {0, 0, 0, 0, 0, 0, 0, 0}, y0[8], y1[8];
    ld_vec(xt + e, xa, VEC);
    model_out<T, VEC>(c + e, GUIDED ? u + e : nullptr, GUIDED, gd, f, scale, m);
    if (has3) ld_vec(third + e, x3, VEC);
    [[maybe_unused]] float xk[8], kp[8];
    if constexpr (KNOWN) {
      // the vector's place in the mask row: one remainder per vector (32-bit where it fits)
      const int64_t i0 = v * VEC;
      const int64_t sp = per_sample <= 0xffffffffll
                             ? (int64_t)((uint32_t)i0 % (uint32_t)kn.S)
                             : i0 % kn.S;
      ld_vec(kn.known + e, xk, VEC);
      const float* krow = kn.keep + b * kn.row;
      if (VEC == 1 || kn.S % VEC == 0) {
        ld_vec(krow + sp, kp, VEC);  // the vector lies inside one channel of the mask
      } else {
        // it may cross into the next channel: its mask values one element at a time, the index
        // stepped and wrapped, so that no access straddles the end of the mask row
        int64_t j = sp;
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
          kp[i] = krow[j];
          if (++j == kn.S) j = 0;
        }
      }
    }
#pragma unroll
    for (int i = 0; i < VEC; ++i) {
      float x0 = rule.x0(xa[i], m[i]);
      if (clip) x0 = fminf(fmaxf(x0, -1.f), 1.f);
      if constexpr (THR) x0 = fminf(fmaxf(x0, -s), s) / s;
      y1[i] = x0;
      y0[i] = rule.x_prev(xa[i], x0, rule.direction(xa[i], m[i]), x3[i]);
    }
    st_vec(xprev + e, y0, VEC);
    if (xdup) st_vec(xdup + e, y0, VEC);
    if (x0o) st_vec(x0o + e, y1, VEC);
    if constexpr (KNOWN) {
      // Up to here the vector went through the unmasked step, statement for statement, stores
      // included: that is what gives k <= 0 the unmasked kernel's bits.  (Formed in one block
      // with the masked values, or from selected operands, the sums fuse another of their
      // products into the multiply-add and the last bit moves.)  A vector with a kept element
      // is formed again from copies of the operands that the optimiser cannot see through, and
      // stored over the first result; its k <= 0 elements keep the values of the first pass.
      bool any = false;
#pragma unroll
      for (int i = 0; i < VEC; ++i) any |= kp[i] > 0.f;
      if (any) {
        float z0[8], z1[8];
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
          const float xb = opaque(xa[i]), yb = opaque(y1[i]), pb = opaque(y0[i]);
          const float lb = opaque(x3[i]);
          const float db = rule.direction(xb, opaque(m[i]));
          const float k = kp[i];
          float xm = xk[i], dm = rule.direction_known(xb, xk[i]);
          if (k < 1.f) {
            xm = (1.f - k) * yb + k * xm;
            dm = (1.f - k) * db + k * dm;
          }
          const bool kept = k > 0.f;
          z1[i] = kept ? xm : yb;
          z0[i] = kept ? rule.x_prev(xb, xm, dm, lb) : pb;
        }
        st_vec(xprev + e, z0, VEC);
        if (xdup) st_vec(xdup + e, z0, VEC);
        if (x0o) st_vec(x0o + e, z1, VEC);
      }
    }
  }
}

// ------------------------------------------------------------ dynamic thresholding
// s_b = min(max(q_b, floor), cap), q_b the rank-th smallest |x0| of sample b (0-based; an element
// of the data): Imagen's dynamic threshold (Saharia et al. 2022, section 2.3) with the "higher"
// order statistic.  x0 is never written to memory: every pass forms it again from the step's
// inputs with the step kernel's own source -- the rule's x0 piece on model_out's vector, with
// cfg_factor's f_b.  The step kernel is another instantiation: where an x0 has two products (v)
// the compiler picks per instantiation which one it fuses, so the step's x0 can differ from this
// one in the last bit (inside the bound the tests hold s to, tests/_thr_cases.py).
//
// Method: a most-significant-digit radix select over the bit pattern of |x0| (non-negative
// floats order as their uint32 patterns; a NaN sorts above +inf), four 8-bit digits, EIGHT
// launches: per digit one histogram launch and one scan launch.
//   histogram: block k of sample b counts the digit of the elements of its fixed range
//     (cfg_chunk's ranges) whose higher digits equal the prefix found so far, into LDS (integer
//     atomics: a count does not depend on the order) and stores its row ws[b][k][256] with plain
//     stores.  kThrCopies sub-histograms per block, picked by the lane: the first digit is the
//     sign and seven exponent bits, so a wave's lanes meet in two or three bins, and same-address
//     LDS atomics serialise.
//   scan: one block per sample adds the rows (integer adds: any order gives the same counts),
//     finds the bin that holds the rank and writes prefix and remaining rank to the sample's
//     state words; the last scan writes s[b].
// All four histogram launches are ONE kernel instantiation with the shift as an argument: the
// same machine code forms x0, so every pass sees the same bits whatever the compiler contracts.
// No global atomics, no float atomics, no memset, no cross-block communication inside a launch;
// every workspace word that is read was written earlier in the same call.
constexpr int kThrBins = 256;
constexpr int kThrCopies = 16;
constexpr int kThrState = 4;  // uint32 per sample: prefix, remaining rank, 2 unused
static_assert(kThrBins == kBlock, "x0_hist_kernel: thread d stores bin d");

// Device view of vd_x0_source (include/vdiff.h).  u == nullptr: unguided.
struct X0Source {
  int rule;
  bool pred_v;
  DDIMScalars ddim;
  DPMRule dpm;
  CfgGuide gd;
  const float* part;
  int nb_cfg;
  float phi;
};

inline size_t thr_state_offset(int64_t B, int nb) { return (size_t)B * nb * kThrBins; }

template <typename T, int VEC>
__global__ void __launch_bounds__(kBlock) x0_hist_kernel(
    X0Source src, const T* __restrict__ x, const T* __restrict__ c, const T* __restrict__ u,
    int64_t P, int64_t chunk, int shift, uint32_t* __restrict__ ws, const uint32_t* state) {
  __shared__ uint32_t hist[kThrBins * kThrCopies];
  const int nb = gridDim.x;
  const int64_t b = blockIdx.y;
  const bool guided = u != nullptr;
  const bool scale = guided && src.phi > 0.f;
  const float f = scale ? cfg_factor(src.part, b, src.nb_cfg, src.phi) : 1.f;
  // the digits above this one, found by the earlier scans (none before the first pass)
  const bool first = shift == 24;
  const uint32_t prefix = first ? 0u : state[b * kThrState];
  const int hi = first ? 0 : shift + 8;
  for (int i = threadIdx.x; i < kThrBins * kThrCopies; i += kBlock) hist[i] = 0u;
  __syncthreads();
  if (src.rule == VD_X0_DDIM) src.ddim.sample_x0(b);
  if (src.rule == VD_X0_DPM) src.dpm.sample_x0(b);
  const int64_t lo = (int64_t)blockIdx.x * chunk;
  const int64_t end = lo + chunk < P ? lo + chunk : P;
  const int64_t base = b * P;
  const int copy = threadIdx.x & (kThrCopies - 1);
  for (int64_t i = lo + (int64_t)threadIdx.x * VEC; i < end; i += (int64_t)kBlock * VEC) {
    const int64_t e = base + i;
    float xa[8], x0[8];
    ld_vec(x + e, xa, VEC);
    if (src.rule == VD_X0_IDENTITY) {
#pragma unroll
      for (int k = 0; k < VEC; ++k) x0[k] = xa[k];
    } else {
      float m[8];
      model_out<T, VEC>(c + e, guided ? u + e : nullptr, guided, src.gd, f, scale, m);
      auto form = [&](const auto& rule) {
#pragma unroll
        for (int k = 0; k < VEC; ++k) x0[k] = rule.x0(xa[k], m[k]);
      };
      if (src.rule == VD_X0_DPM)
        form(src.dpm);
      else if (src.pred_v)
        form(DDIMRule<true>{src.ddim});
      else
        form(DDIMRule<false>{src.ddim});
    }
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      const uint32_t bits = __float_as_uint(x0[k]) & 0x7fffffffu;
      if (first || (bits >> hi) == prefix)
        atomicAdd(&hist[((bits >> shift) & (kThrBins - 1)) * kThrCopies + copy], 1u);
    }
  }
  __syncthreads();
  // thread d adds bin d's copies, starting at its own: the lanes of a wave read different banks
  uint32_t n = 0;
#pragma unroll
  for (int j = 0; j < kThrCopies; ++j)
    n += hist[threadIdx.x * kThrCopies + ((j + threadIdx.x) & (kThrCopies - 1))];
  ws[(b * nb + blockIdx.x) * kThrBins + threadIdx.x] = n;
}

// kThrScanParts groups of kThrBins threads: group j adds rows j, j + kThrScanParts, ... of its
// bin (a single block per sample walks up to 128 rows, and its time is the latency of those
// loads: four independent streams, each unrolled, in place of one cut a scan from 19 to
// a few microseconds), then group 0 adds the groups' sums and scans the bins.
constexpr int kThrScanParts = 4;

__global__ void __launch_bounds__(kThrBins* kThrScanParts)
    x0_scan_kernel(const uint32_t* __restrict__ ws, int nb, int shift, uint32_t rank, float floor_,
                   float cap, uint32_t* state, float* __restrict__ s_out) {
  __shared__ uint32_t part[kThrScanParts][kThrBins];
  __shared__ uint32_t cum[kThrBins];
  const int64_t b = blockIdx.x;
  const int d = threadIdx.x & (kThrBins - 1);
  const int grp = threadIdx.x / kThrBins;
  const bool first = shift == 24;
  const uint32_t prefix = first ? 0u : state[b * kThrState];
  const uint32_t want = first ? rank : state[b * kThrState + 1];
  const uint32_t* rows = ws + b * nb * kThrBins;
  uint32_t n = 0;
#pragma unroll 8
  for (int k = grp; k < nb; k += kThrScanParts) n += rows[k * kThrBins + d];
  part[grp][d] = n;
  __syncthreads();  // also: every thread has read the state words before one is rewritten
  if (grp == 0) {
#pragma unroll
    for (int j = 1; j < kThrScanParts; ++j) n += part[j][d];
    cum[d] = n;
  }
  __syncthreads();
  // inclusive scan over the bins (Hillis-Steele; integer adds, any order gives the same counts)
  for (int off = 1; off < kThrBins; off <<= 1) {
    const uint32_t add = (grp == 0 && d >= off) ? cum[d - off] : 0u;
    __syncthreads();
    if (grp == 0) cum[d] += add;
    __syncthreads();
  }
  if (grp != 0) return;
  const uint32_t incl = cum[d], excl = incl - n;
  // the counts are those of the elements under `prefix`, more than `want` of them: one bin
  if (want >= excl && want < incl) {
    const uint32_t found = (prefix << 8) | (uint32_t)d;
    if (shift == 0) {
      // fmaxf: a NaN quantile becomes the floor
      s_out[b] = fminf(fmaxf(__uint_as_float(found), floor_), cap);
    } else {
      state[b * kThrState] = found;
      state[b * kThrState + 1] = want - excl;
    }
  }
}

// ------------------------------------------------------------ sampler step: host side
// What the eight step entry points hand to check_step and launch_step.  c / u: the model output
// with / without the audio (u NULL: unguided); third: z (DDIM) or the history (DPM), x0 the
// optional x0 output (DDIM) or the history again (DPM); thresh non-NULL: the thresholded step.
struct StepArgs {
  int rule = VD_X0_DDIM;  // VD_X0_DDIM | VD_X0_DPM
  int prediction = VD_PRED_EPS;
  const void *xt = nullptr, *c = nullptr, *u = nullptr, *third = nullptr;
  void *xprev = nullptr, *xdup = nullptr, *x0 = nullptr;
  const int64_t *t = nullptr, *tprev = nullptr;  // DDIM
  const float* acp = nullptr;
  float eta = 0.f;
  const float* coef = nullptr;  // DPM
  int64_t n_steps = 0;
  const int64_t* step = nullptr;
  float w = 1.f, rescale = 0.f;
  const void* workspace = nullptr;
  const float* thresh = nullptr;
  int clip = 0;
  int64_t B = 0, per_sample = 0;
  const void* known = nullptr;  // masked step: the clip to keep and keep fp32 [Bk][S]
  const float* keep = nullptr;
  int64_t Bk = 0, S = 0;
};

// The one place a rule is built: launch_step and vd_x0_abs_quantile (t_prev NULL: its x0 piece
// alone) both take theirs from here.
inline DDIMScalars make_ddim(const float* acp, const int64_t* t, const int64_t* tprev, float eta,
                             bool has_z) {
  DDIMScalars r = {};
  r.acp = acp, r.t = t, r.tprev = tprev, r.eta = eta, r.has_z = has_z;
  return r;
}
inline DPMRule make_dpm(const float* coef, int64_t n_steps, const int64_t* step) {
  DPMRule r = {};
  r.coef = coef, r.n_steps = n_steps, r.step = step;
  return r;
}

enum StepKind { STEP_PLAIN, STEP_CFG, STEP_THR };

// The conditions the entry points share.  STEP_PLAIN takes any B (cfg_grid adds a layer of rows
// for every 65535 samples); STEP_CFG needs u; STEP_THR needs thresh, and the workspace only
// when guided.
int check_step(const StepArgs& a, StepKind kind) {
  const bool dpm = a.rule == VD_X0_DPM;
  VD_REQUIRE(a.xt && a.c && a.xprev && (kind != STEP_CFG || a.u) && (kind != STEP_THR || a.thresh)
                 && (dpm ? a.x0 && a.coef && a.step : a.t && a.tprev && a.acp),
             "null argument");
  const bool shape_ok = a.B > 0 && (kind == STEP_PLAIN || a.B <= 65535) && a.per_sample > 0;
  const char* bad =
      kind != STEP_PLAIN ? "bad shape" : (dpm ? "empty tensor or table" : "empty tensor");
  if (dpm)
    VD_REQUIRE(shape_ok && a.n_steps > 0, "%s (B=%lld, per_sample=%lld, n_steps=%lld)", bad,
               (long long)a.B, (long long)a.per_sample, (long long)a.n_steps);
  else
    VD_REQUIRE(shape_ok, "%s (B=%lld, per_sample=%lld)", bad, (long long)a.B,
               (long long)a.per_sample);
  if (kind != STEP_PLAIN) {
    VD_REQUIRE(a.rescale >= 0.f && a.rescale <= 1.f, "rescale %g outside [0, 1]",
               (double)a.rescale);
    VD_REQUIRE(!a.u || a.rescale == 0.f || a.workspace,
               "rescale > 0 needs the vd_cfg_stats workspace (null)");
  }
  VD_REQUIRE((a.known != nullptr) == (a.keep != nullptr),
             "known and keep are given together or not at all");
  if (a.known) {
    VD_REQUIRE((a.Bk == 1 || a.Bk == a.B) && a.S > 0 && a.per_sample % a.S == 0,
               "bad keep mask (Bk=%lld for B=%lld, S=%lld for per_sample=%lld)", (long long)a.Bk,
               (long long)a.B, (long long)a.S, (long long)a.per_sample);
    VD_REQUIRE(!(a.thresh && a.clip), "thresh and clip exclude each other");
  }
  if (!dpm) {
    VD_REQUIRE(a.eta == 0.f || a.third, "eta > 0 needs z");
    VD_REQUIRE(a.prediction == VD_PRED_EPS || a.prediction == VD_PRED_V,
               "unknown prediction type %d", a.prediction);
  }
  return VD_OK;
}

template <typename F>
void dispatch_bool(bool v, F&& f) {
  if (v)
    f(std::true_type{});
  else
    f(std::false_type{});
}

template <typename T, typename Rule>
void launch_rule(const Rule& rule, const StepArgs& a, hipStream_t st) {
  // masked: the unmasked step's width (its bits where k <= 0), known and keep aligned as well
  const bool v8 = cfg_vec8(a.per_sample, {a.xt, a.c, a.u, a.third, a.xprev, a.xdup, a.x0, a.known,
                                          a.keep});
  const dim3 grid = cfg_grid(a.per_sample, v8 ? 8 : 1, a.B);
  dispatch_bool(v8, [&](auto V8) {
    dispatch_bool(a.thresh != nullptr, [&](auto THR) {
      dispatch_bool(a.u != nullptr, [&](auto GUIDED) {
        dispatch_bool(a.known != nullptr, [&](auto KNOWN) {
          constexpr bool kKnown = decltype(KNOWN)::value;
          KnownOps<T, kKnown> kn;
          if constexpr (kKnown)
            kn = {(const T*)a.known, a.keep, a.S, a.Bk == 1 ? (int64_t)0 : a.S};
          step_kernel<T, decltype(V8)::value ? 8 : 1, Rule, decltype(THR)::value,
                      decltype(GUIDED)::value, kKnown><<<grid, kBlock, 0, st>>>(
              rule, CfgGuide{a.w}, (const T*)a.xt, (const T*)a.c, (const T*)a.u,
              (const T*)a.third, (T*)a.xprev, (T*)a.xdup, (T*)a.x0,
              static_cast<const float*>(a.workspace), cfg_blocks(a.per_sample), a.rescale,
              a.thresh, a.clip, a.B, a.per_sample, kn);
        });
      });
    });
  });
}

// Vector width (cfg_vec8 over all non-null pointers), grid, and the dispatch over dtype, rule,
// threshold, guidance, mask and VEC: one launch line.
int launch_step(const StepArgs& a, int dtype, void* stream) {
  hipStream_t st = VD_STREAM(stream);
  return VD_DISPATCH_DTYPE(dtype, T, {
    if (a.rule == VD_X0_DPM) {
      launch_rule<T>(make_dpm(a.coef, a.n_steps, a.step), a, st);
    } else {
      const DDIMScalars r = make_ddim(a.acp, a.t, a.tprev, a.eta, a.third != nullptr);
      if (a.prediction == VD_PRED_V)
        launch_rule<T>(DDIMRule<true>{r}, a, st);
      else
        launch_rule<T>(DDIMRule<false>{r}, a, st);
    }
  });
}

// A DDIM step's arguments as every DDIM entry point fills them.
StepArgs ddim_args(const void* xt, const void* c, const void* u, const void* z, void* x_prev,
                   void* x_prev_dup, void* x0, const int64_t* t, const int64_t* t_prev,
                   const float* acp, float eta, int clip, int prediction, int64_t B,
                   int64_t per_sample) {
  StepArgs a;
  a.prediction = prediction;
  a.xt = xt, a.c = c, a.u = u, a.third = z;
  a.xprev = x_prev, a.xdup = x_prev_dup, a.x0 = x0;
  a.t = t, a.tprev = t_prev, a.acp = acp, a.eta = eta, a.clip = clip;
  a.B = B, a.per_sample = per_sample;
  return a;
}

// The same for DPM-Solver++: the history is the third input and the x0 output.
StepArgs dpm_args(const void* xt, const void* c, const void* u, void* x_prev, void* x_prev_dup,
                  void* x0_hist, const float* coef, int64_t n_steps, const int64_t* step, int clip,
                  int64_t B, int64_t per_sample) {
  StepArgs a;
  a.rule = VD_X0_DPM;
  a.xt = xt, a.c = c, a.u = u, a.third = x0_hist;
  a.xprev = x_prev, a.xdup = x_prev_dup, a.x0 = x0_hist;
  a.coef = coef, a.n_steps = n_steps, a.step = step, a.clip = clip;
  a.B = B, a.per_sample = per_sample;
  return a;
}

// w, rescale and workspace of a guided or thresholded step
StepArgs guided(StepArgs a, float w, float rescale, const void* workspace, const float* thresh) {
  a.w = w, a.rescale = rescale, a.workspace = workspace, a.thresh = thresh;
  return a;
}

// known / keep of a masked step, and the kind its other operands make it
StepArgs masked(StepArgs a, const void* known, const float* keep, int64_t Bk, int64_t S) {
  a.known = known, a.keep = keep, a.Bk = Bk, a.S = S;
  return a;
}
inline StepKind kind_of(const StepArgs& a) {
  return a.thresh ? STEP_THR : (a.u ? STEP_CFG : STEP_PLAIN);
}

int run_step(const StepArgs& a, StepKind kind, int dtype, void* stream) {
  const int rc = check_step(a, kind);
  return rc != VD_OK ? rc : launch_step(a, dtype, stream);
}

}  // namespace


// ---------------------------------------------------------------- conv glue
// Per-(sample, channel) sums of a channels-last activation: the bias gradient and the
// ResBlock emb-add (chan_add) gradient of a conv in one pass over dY (reference autograd of
// conv_nd's bias, utils.py:59-69, and of `h + emb_out` at unet.py:255-258).  Stage 1: a
// block owns a run of rows of one sample, each thread sums 8 channels over its rows in fp32,
// the block reduces through LDS and stores its partial row part[b][blk][C].  Stage 2 sums
// the partial rows per channel (deterministic; no same-address atomics, which serialise).
constexpr int kSumBlocks = 1024;  // stage-1 blocks per sample (upper bound: finish registers)
// stage-1 blocks per sample actually launched (default 256; VDIFF_CSUM_BLOCKS, <= kSumBlocks,
// for A/B runs) and the rows each stage-1 thread keeps in flight (VDIFF_CSUM_UNROLL 1 or 4;
// default 4 since round 4: the step's sums 1.10 -> 0.73 ms, e.g. 192 x 262144 36.3 -> 19.4 us
// at 5.2 TB/s, bit-identical (same add order); profiles/r04af_ab_channel_sums.txt)
static int csum_env(const char* name, int dflt, int lo, int hi) {
  const char* e = getenv(name);
  const int v = e ? atoi(e) : dflt;
  return v < lo ? lo : (v > hi ? hi : v);
}
const int g_csum_blocks = csum_env("VDIFF_CSUM_BLOCKS", 256, 1, kSumBlocks);
const int g_csum_unroll = csum_env("VDIFF_CSUM_UNROLL", 4, 1, 4);

template <typename T, int U>
__global__ __launch_bounds__(256) void channel_sums_kernel(const T* __restrict__ x, int64_t S,
                                                           int C, int cs, int64_t rows_per_blk,
                                                           float* __restrict__ part) {
  __shared__ float red[256 * 8];
  const int b = blockIdx.y;
  const int tpr = C / 8;                 // threads per row (C <= 2048)
  const int rpi = 256 / tpr;             // rows per iteration
  const int tid = threadIdx.x;
  const int lr = tid / tpr, c8 = (tid % tpr) * 8;
  float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  const int64_t r0 = (int64_t)blockIdx.x * rows_per_blk;
  int64_t r1 = r0 + rows_per_blk;
  if (r1 > S) r1 = S;
  if (lr < rpi) {
    const T* base = x + (int64_t)b * S * cs + c8;
    int64_t r = r0 + lr;
    if constexpr (U > 1) {  // U rows' loads in flight before their adds (same add order)
      for (; r + (U - 1) * rpi < r1; r += U * rpi) {
        float v[U][8];
#pragma unroll
        for (int u = 0; u < U; ++u) load8(base + (r + u * rpi) * cs, v[u]);
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
          for (int e = 0; e < 8; ++e) acc[e] += v[u][e];
      }
    }
    for (; r < r1; r += rpi) {
      float v[8];
      load8(base + r * cs, v);
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[e] += v[e];
    }
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) red[tid * 8 + e] = acc[e];
  __syncthreads();
  // thread t < C sums channel t over the rpi row lanes
  float* dst = part + ((int64_t)b * gridDim.x + blockIdx.x) * C;
  for (int c = tid; c < C; c += 256) {
    const int g = c / 8, e = c % 8;
    float sum = 0.f;
    for (int k = 0; k < rpi; ++k) sum += red[(k * tpr + g) * 8 + e];
    dst[c] = sum;
  }
}

// 32 channels per block, 32 row lanes per channel: at most 8 independent partial loads per
// lane (kSumBlocks = 1024 / 32), all in flight before the adds; fixed-order LDS reduce
__global__ __launch_bounds__(1024) void channel_sums_finish_kernel(const float* __restrict__ part,
                                                                   int nblk, int C,
                                                                   float* __restrict__ out) {
  __shared__ float red[32][33];
  const int cl = threadIdx.x & 31, kl = threadIdx.x >> 5;
  const int c = blockIdx.x * 32 + cl, b = blockIdx.y;
  float v[kSumBlocks / 32];
#pragma unroll
  for (int i = 0; i < kSumBlocks / 32; ++i) {
    const int k = kl + 32 * i;
    v[i] = (c < C && k < nblk) ? part[((int64_t)b * nblk + k) * C + c] : 0.f;
  }
  float sum = 0.f;
#pragma unroll
  for (int i = 0; i < kSumBlocks / 32; ++i) sum += v[i];
  red[kl][cl] = sum;
  __syncthreads();
  if (kl == 0 && c < C) {
#pragma unroll
    for (int k = 1; k < 32; ++k) sum += red[k][cl];
    out[(int64_t)b * C + c] = sum;
  }
}

// fp32 torch weight [Co][Ci][taps] -> packed operand in the activation dtype, channels
// zero-padded: fwd  [Co][taps][Cip]  (transpose = 0)
//              bwd  [Cip][taps][Cop] (transpose = 1, the transposed-conv operand)
template <typename T>
__global__ void pack_weight_kernel(const float* __restrict__ w, int Co, int Ci, int taps, int Cip,
                                   int Cop, int transpose, T* __restrict__ out) {
  const int64_t total = transpose ? (int64_t)Cip * taps * Cop : (int64_t)Co * taps * Cip;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * blockDim.x) {
    int co, ci, tap;
    if (!transpose) {
      ci = (int)(i % Cip);
      tap = (int)((i / Cip) % taps);
      co = (int)(i / ((int64_t)Cip * taps));
    } else {
      co = (int)(i % Cop);
      tap = (int)((i / Cop) % taps);
      ci = (int)(i / ((int64_t)Cop * taps));
    }
    const float v = (co < Co && ci < Ci) ? w[((int64_t)co * Ci + ci) * taps + tap] : 0.f;
    Elem<T>::st(out + i, v);
  }
}

// vd_conv_pack_weights: the step's conv operands in one launch, as LDS-tiled transposes.
// A tile is 4 output channels x 64 input channels (the [Co][taps][Ci] layout) or 8 input
// channels x 64 output channels (the transposed [Ci][taps][Co] layout), all taps: the source
// rows w[co][ci0 ..][0 .. taps) are read contiguously (fp32), transposed in LDS, and the
// destination rows of 64 channels written as 16-B vectors.  Every block derives the jobs' tile
// counts and their prefix sums itself (the descriptors live on the device) and walks the
// tiles grid-stride.  A job with more than kPackMaxTaps taps (none in the UNet) is packed
// element by element in blocks of 2048 outputs.  Round 4's element-wise form (64-bit index
// math and a job search per element, strided reads) took 0.69 ms per train step.
constexpr int kPackMaxTaps = 27;
constexpr int kPackRow = 65;  // LDS row of 64 channels + 1: consecutive taps on distinct banks
constexpr int kPackSmem = 8 * kPackMaxTaps * kPackRow * 4;  // the transposed tile, the larger

// rows (outer channels) per tile: ~100-200 source floats per row of taps, so that a tile
// carries enough work for its two barriers (1x1 jobs: 64 x 64 tiles)
__host__ __device__ constexpr int pack_rows(int taps, bool transpose) {
  return taps == 1 ? 64 : taps <= 9 ? 16 : (transpose ? 8 : 4);
}

__device__ __forceinline__ int pack_tiles(const vd_pack_desc& d) {
  if (d.taps > kPackMaxTaps) return (int)((d.transpose ? (int64_t)d.Cip * d.taps * d.Cop
                                                       : (int64_t)d.Co * d.taps * d.Cip) +
                                          2047) / 2048;
  // the row counts pack_tile<T, TAPS> uses: specialised 1 / 9 / 27 taps, else the 27-tap rows
  const bool spec = d.taps == 1 || d.taps == 9 || d.taps == 27;
  const int R = pack_rows(spec ? d.taps : kPackMaxTaps, d.transpose);
  return d.transpose ? ((d.Cip + R - 1) / R) * ((d.Cop + 63) / 64)
                     : ((d.Co + R - 1) / R) * ((d.Cip + 63) / 64);
}

// One tile: NO outer rows (co, or ci when transposed) x 64 inner channels x all taps.  The
// source of outer row o is the run w[...][inner0 ..][0 .. taps) (non-transposed: contiguous
// 64 * taps floats of w[co]; transposed: R * taps floats of w[co][ci0 ..] for each of the
// 64 co) -- both read as (row, r) pairs with 32-bit offsets; LDS image [o][tap][65].
template <typename T, int TAPS>
__device__ __forceinline__ void pack_tile(const vd_pack_desc& d, int lt, float* ptile) {
  const int tp = TAPS ? TAPS : d.taps;
  const bool tr = d.transpose;
  constexpr int RN = pack_rows(TAPS ? TAPS : kPackMaxTaps, false);
  constexpr int RT = pack_rows(TAPS ? TAPS : kPackMaxTaps, true);
  // load rows: non-transposed RN co rows of 64 * tp floats; transposed 64 co rows of RT * tp
  const int nrows = tr ? 64 : RN;
  const int per = tr ? RT * tp : 64 * tp;
  const int ninner = tr ? d.Cop : d.Cip;                 // padded inner extent of the output
  const int nib = (ninner + 63) / 64;
  const int outer0 = (lt / nib) * (tr ? RT : RN), inner0 = (lt % nib) * 64;
  const int co0 = tr ? inner0 : outer0, ci0 = tr ? outer0 : inner0;
  const int rowlen = d.Ci * tp;                          // floats per co in w
  const float* src = d.w + co0 * rowlen + ci0 * tp;      // (co0, ci0, tap 0)
  const int ci_lim = d.Ci - ci0, co_lim = d.Co - co0;
  constexpr int NL = 16;
  for (int base = 0; base < nrows * per; base += NL * kBlock) {
    float v[NL];
    int dst[NL];
#pragma unroll
    for (int u = 0; u < NL; ++u) {
      const int idx = base + u * kBlock + threadIdx.x;
      const int row = idx / per, r = idx - row * per;    // row: co offset (both layouts read
      const int cil = r / tp, tap = r - cil * tp;        // w[co] rows); r: (ci offset, tap)
      const bool ok = idx < nrows * per && row < co_lim && cil < ci_lim;
      v[u] = ok ? src[row * rowlen + r] : 0.f;
      // LDS [outer][tap][inner]: non-transposed outer = co (row), inner = ci (cil);
      // transposed outer = ci (cil), inner = co (row)
      dst[u] = idx < nrows * per ? ((tr ? cil : row) * tp + tap) * kPackRow + (tr ? row : cil)
                                 : -1;
    }
#pragma unroll
    for (int u = 0; u < NL; ++u)
      if (dst[u] >= 0) ptile[dst[u]] = v[u];
  }
  __syncthreads();
  const int orows = tr ? RT : RN;                        // output rows: (outer, tap)
  const int olim = tr ? d.Cip - ci0 : d.Co - co0;
  T* out = (T*)d.out;
  for (int idx = threadIdx.x; idx < orows * tp * 8; idx += kBlock) {
    const int row = idx >> 3, c8 = (idx & 7) * 8;
    const int o = row / tp, tap = row - o * tp;
    if (o < olim && inner0 + c8 < ninner) {
      float f[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) f[k] = ptile[row * kPackRow + c8 + k];
      store8(out + ((int64_t)(outer0 + o) * tp + tap) * ninner + inner0 + c8, f);
    }
  }
}

template <typename T>
__global__ void __launch_bounds__(kBlock) pack_weights_kernel(
    const vd_pack_desc* __restrict__ descs, int n) {
  extern __shared__ __attribute__((aligned(16))) float ptile[];
  __shared__ int tstart[1025];
  // tstart[j + 1] = the jobs' tile counts, then an inclusive Hillis-Steele scan over them
  // (parallel: a serial walk over the descriptors costs a global-load latency per job)
  if (threadIdx.x == 0) tstart[0] = 0;
  for (int j = threadIdx.x; j < n; j += kBlock) tstart[j + 1] = pack_tiles(descs[j]);
  __syncthreads();
  for (int off = 1; off < n; off <<= 1) {
    int v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int j = threadIdx.x + k * kBlock + 1;
      v[k] = (j <= n && j - off >= 1) ? tstart[j - off] : 0;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int j = threadIdx.x + k * kBlock + 1;
      if (j <= n) tstart[j] += v[k];
    }
    __syncthreads();
  }
  const int ntiles = tstart[n];
  for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {  // the last job whose first tile <= t
      const int mid = (lo + hi + 1) >> 1;
      if (tstart[mid] <= t) lo = mid; else hi = mid - 1;
    }
    const vd_pack_desc d = descs[lo];
    const int lt = t - tstart[lo];
    const int taps = d.taps;
    T* out = (T*)d.out;
    if (taps > kPackMaxTaps) {  // element-wise fallback
      const int inner = d.transpose ? d.Cop : d.Cip;
      const int64_t size = d.transpose ? (int64_t)d.Cip * taps * d.Cop
                                       : (int64_t)d.Co * taps * d.Cip;
      for (int64_t e = (int64_t)lt * 2048 + threadIdx.x; e < size && e < (int64_t)(lt + 1) * 2048;
           e += kBlock) {
        const int64_t rest = e / inner;
        const int in = (int)(e % inner), tap = (int)(rest % taps), o = (int)(rest / taps);
        const int co = d.transpose ? in : o, ci = d.transpose ? o : in;
        Elem<T>::st(out + e, (co < d.Co && ci < d.Ci)
                                 ? d.w[((int64_t)co * d.Ci + ci) * taps + tap] : 0.f);
      }
      continue;
    }
    switch (taps) {  // compile-time divisors (a runtime integer division costs ~40 VALU)
      case 27: pack_tile<T, 27>(d, lt, ptile); break;
      case 9: pack_tile<T, 9>(d, lt, ptile); break;
      case 1: pack_tile<T, 1>(d, lt, ptile); break;
      default: pack_tile<T, 0>(d, lt, ptile); break;
    }
    __syncthreads();  // the tile buffer is reused by the next tile
  }
}

// ------------------------------------------------------------ weight EMA
// One launch for every tracked parameter and up to four rates.  The host cuts each tensor
// into fixed-size ranges (one vd_ema_desc each); blocks walk that table grid-stride, so the
// table may be of any length (no in-kernel scan over it as in pack_weights_kernel) and every
// element belongs to exactly one (descriptor, lane) whatever the grid.  The update count and
// the bad-step flag are read from device memory, so a captured launch replays with the current
// count; nothing but the shadows is written.
namespace {

struct EmaArgs {
  float rate[4];
  const int64_t* num_updates;  // read when warmup
  const int64_t* skip;         // may be null
  int warmup;
};

template <int K>
__global__ void __launch_bounds__(kBlock) ema_kernel(const vd_ema_desc* __restrict__ descs,
                                                     int n_desc, EmaArgs a) {
  if (a.skip && *a.skip >= 0) return;
  float w[K];  // 1 - d_j
  {
    float cap = 1.f;
    if (a.warmup) {
      const int64_t n = *a.num_updates;
      cap = (float)(1 + n) / (float)(10 + n);
    }
#pragma unroll
    for (int j = 0; j < K; ++j) w[j] = 1.0f - (a.warmup ? fminf(a.rate[j], cap) : a.rate[j]);
  }
  for (int i = blockIdx.x; i < n_desc; i += gridDim.x) {
    const vd_ema_desc d = descs[i];
    uintptr_t align = reinterpret_cast<uintptr_t>(d.src);
#pragma unroll
    for (int j = 0; j < K; ++j) align |= reinterpret_cast<uintptr_t>(d.dst[j]);
    // 8 elements per lane where every pointer allows 16-B accesses, else element by element
    const int64_t nv = (align % 16 == 0) ? d.n / 8 : 0;
    for (int64_t v = threadIdx.x; v < nv; v += kBlock) {
      float p[8], e[K][8];
      load8(d.src + v * 8, p);  // read once for all K rates; every load before any store
#pragma unroll
      for (int j = 0; j < K; ++j) load8(d.dst[j] + v * 8, e[j]);
#pragma unroll
      for (int j = 0; j < K; ++j) {
#pragma unroll
        for (int q = 0; q < 8; ++q) e[j][q] = fmaf(w[j], p[q] - e[j][q], e[j][q]);
        store8(d.dst[j] + v * 8, e[j]);
      }
    }
    for (int64_t s = nv * 8 + threadIdx.x; s < d.n; s += kBlock) {
      const float p = d.src[s];
#pragma unroll
      for (int j = 0; j < K; ++j) {
        const float e = d.dst[j][s];
        d.dst[j][s] = fmaf(w[j], p - e, e);
      }
    }
  }
}

}  // namespace

extern "C" {

int vd_ema_update(const vd_ema_desc* descs, int n_desc, int k, const float* rates, int warmup,
                  const int64_t* num_updates, const int64_t* skip_if_nonneg, void* stream) {
  VD_REQUIRE(descs && rates, "null argument");
  VD_REQUIRE(n_desc > 0, "empty descriptor table (n_desc=%d)", n_desc);
  VD_REQUIRE(k >= 1 && k <= 4, "k=%d outside 1..4", k);
  EmaArgs a = {};
  for (int j = 0; j < k; ++j) {
    VD_REQUIRE(rates[j] >= 0.f && rates[j] < 1.f, "rate %d = %g outside [0, 1)", j,
               (double)rates[j]);
    a.rate[j] = rates[j];
  }
  VD_REQUIRE(!warmup || num_updates, "warmup needs num_updates");
  a.num_updates = num_updates;
  a.skip = skip_if_nonneg;
  a.warmup = warmup != 0;
  const int grid = n_desc < 2048 ? n_desc : 2048;  // 8 blocks per CU, then grid-stride
  hipStream_t st = VD_STREAM(stream);
  switch (k) {
    case 1: ema_kernel<1><<<grid, kBlock, 0, st>>>(descs, n_desc, a); break;
    case 2: ema_kernel<2><<<grid, kBlock, 0, st>>>(descs, n_desc, a); break;
    case 3: ema_kernel<3><<<grid, kBlock, 0, st>>>(descs, n_desc, a); break;
    default: ema_kernel<4><<<grid, kBlock, 0, st>>>(descs, n_desc, a); break;
  }
  return vd::check_launch("vd_ema_update");
}

size_t vd_mse_loss_workspace_size(int64_t n) {
  return (size_t)mse_blocks(n) * sizeof(float);
}

int vd_mse_loss(const void* pred, const void* target, int64_t n, int dtype, float* out,
                void* workspace, size_t workspace_bytes, void* stream) {
  VD_REQUIRE(pred && target && out && workspace, "null argument");
  VD_REQUIRE(n > 0, "empty tensor");
  VD_REQUIRE(dtype == VD_F32 || dtype == VD_BF16, "bad dtype %d", dtype);
  VD_REQUIRE((reinterpret_cast<uintptr_t>(pred) | reinterpret_cast<uintptr_t>(target)) % 16 == 0,
             "pred / target must be 16-B aligned");
  const int nb = mse_blocks(n);
  VD_REQUIRE(workspace_bytes >= (size_t)nb * sizeof(float), "workspace too small");
  const int64_t chunk = vd_cdiv(vd_cdiv(n, nb), 8) * 8;
  float* partial = static_cast<float*>(workspace);
  hipStream_t st = VD_STREAM(stream);
  if (dtype == VD_F32)
    mse_partial_kernel<float><<<nb, kBlock, 0, st>>>(static_cast<const float*>(pred),
                                                     static_cast<const float*>(target), n,
                                                     chunk, partial);
  else
    mse_partial_kernel<bf16_t><<<nb, kBlock, 0, st>>>(static_cast<const bf16_t*>(pred),
                                                      static_cast<const bf16_t*>(target), n,
                                                      chunk, partial);
  mse_finish_kernel<<<1, kBlock, 0, st>>>(partial, nb, (float)(1.0 / (double)n), out);
  return vd::check_launch("vd_mse_loss");
}

int vd_mse_loss_bwd(const void* pred, const void* target, const float* grad_loss, int64_t n,
                    int dtype, void* grad_pred, void* stream) {
  VD_REQUIRE(pred && target && grad_loss && grad_pred, "null argument");
  VD_REQUIRE(n > 0, "empty tensor");
  VD_REQUIRE(dtype == VD_F32 || dtype == VD_BF16, "bad dtype %d", dtype);
  VD_REQUIRE((reinterpret_cast<uintptr_t>(pred) | reinterpret_cast<uintptr_t>(target) |
              reinterpret_cast<uintptr_t>(grad_pred)) % 16 == 0, "buffers must be 16-B aligned");
  const float scale = (float)(2.0 / (double)n);
  hipStream_t st = VD_STREAM(stream);
  const int g = grid_for(vd_cdiv(n, 8));
  if (dtype == VD_F32)
    mse_bwd_kernel<float><<<g, kBlock, 0, st>>>(static_cast<const float*>(pred),
                                                static_cast<const float*>(target), grad_loss,
                                                scale, n, static_cast<float*>(grad_pred));
  else
    mse_bwd_kernel<bf16_t><<<g, kBlock, 0, st>>>(static_cast<const bf16_t*>(pred),
                                                 static_cast<const bf16_t*>(target), grad_loss,
                                                 scale, n, static_cast<bf16_t*>(grad_pred));
  return vd::check_launch("vd_mse_loss_bwd");
}

int vd_timestep_embedding(const int64_t* t, int B, int dim, float max_period, float* out,
                          void* stream) {
  VD_REQUIRE(t && out, "null argument");
  VD_REQUIRE(B > 0 && dim > 0, "bad shape B=%d dim=%d", B, dim);
  temb_kernel<<<grid_for((int64_t)B * dim), kBlock, 0, VD_STREAM(stream)>>>(
      t, B, dim, logf(max_period), nullptr, out);
  return vd::check_launch("vd_timestep_embedding");
}

int vd_timestep_embedding_tab(const int64_t* t, int B, int dim, const float* freqs, float* out,
                              void* stream) {
  VD_REQUIRE(t && out && (freqs || dim < 2), "null argument");
  VD_REQUIRE(B > 0 && dim > 0, "bad shape B=%d dim=%d", B, dim);
  temb_kernel<<<grid_for((int64_t)B * dim), kBlock, 0, VD_STREAM(stream)>>>(t, B, dim, 0.f,
                                                                            freqs, out);
  return vd::check_launch("vd_timestep_embedding_tab");
}

int vd_q_sample(const void* x0, const void* eps, void* xt, const int64_t* t, const float* sqrt_acp,
                const float* sqrt_1m_acp, int64_t B, int64_t per_sample, int dtype, void* stream) {
  VD_REQUIRE(sqrt_acp && sqrt_1m_acp, "null table");
  return launch_sched(QSample{sqrt_acp, sqrt_1m_acp}, x0, eps, nullptr, xt, nullptr, t, B,
                      per_sample, dtype, stream);
}

int vd_p_sample_v1(const void* xt, const void* eps, const void* z, void* x_prev, void* x0,
                   const int64_t* t, const float* betas, const float* alphas, const float* acp,
                   const float* sqrt_1m_acp, int64_t B, int64_t per_sample, int dtype,
                   void* stream) {
  VD_REQUIRE(betas && alphas && acp && sqrt_1m_acp, "null table");
  VD_REQUIRE(z && x0, "p_sample_v1 needs z and x0 buffers");
  return launch_sched(PSampleV1{betas, alphas, acp, sqrt_1m_acp}, xt, eps, z, x_prev, x0, t, B,
                      per_sample, dtype, stream);
}

int vd_p_sample_v2(const void* xt, const void* eps, const void* z, void* x_prev, void* x0,
                   const int64_t* t, const float* betas, const float* alphas, const float* acp,
                   const float* sqrt_acp, const float* sqrt_1m_acp, int64_t B,
                   int64_t per_sample, int dtype, void* stream) {
  VD_REQUIRE(betas && alphas && acp && sqrt_acp && sqrt_1m_acp, "null table");
  VD_REQUIRE(z && x0, "p_sample_v2 needs z and x0 buffers");
  return launch_sched(PSampleV2{betas, alphas, acp, sqrt_acp, sqrt_1m_acp}, xt, eps, z, x_prev,
                      x0, t, B, per_sample, dtype, stream);
}

int vd_p_sample_cosine(const void* xt, const void* eps, const void* z, void* x_prev,
                       void* mean_out, const int64_t* t, const float* acp, const float* sqrt_acp,
                       const float* sqrt_1m_acp, int64_t B, int64_t per_sample, int dtype,
                       void* stream) {
  VD_REQUIRE(acp && sqrt_acp && sqrt_1m_acp, "null table");
  VD_REQUIRE(z && mean_out, "p_sample_cosine needs z and mean buffers");
  return launch_sched(PSampleCos{acp, sqrt_acp, sqrt_1m_acp}, xt, eps, z, x_prev, mean_out, t, B,
                      per_sample, dtype, stream);
}

int vd_ddim_step_pred(const void* xt, const void* eps, const void* z, void* x_prev, void* x0,
                      const int64_t* t, const int64_t* t_prev, const float* acp, float eta,
                      int clip, int prediction, int64_t B, int64_t per_sample, int dtype,
                      void* stream) {
  return run_step(ddim_args(xt, eps, nullptr, z, x_prev, nullptr, x0, t, t_prev, acp, eta, clip,
                            prediction, B, per_sample),
                  STEP_PLAIN, dtype, stream);
}

int vd_ddim_step(const void* xt, const void* eps, const void* z, void* x_prev, void* x0,
                 const int64_t* t, const int64_t* t_prev, const float* acp, float eta, int clip,
                 int64_t B, int64_t per_sample, int dtype, void* stream) {
  return vd_ddim_step_pred(xt, eps, z, x_prev, x0, t, t_prev, acp, eta, clip, VD_PRED_EPS, B,
                           per_sample, dtype, stream);
}

size_t vd_cfg_workspace_size(int64_t B, int64_t per_sample) {
  if (B <= 0 || per_sample <= 0) return 0;
  return (size_t)B * cfg_blocks(per_sample) * 4 * sizeof(float);
}

int vd_cfg_stats(const void* eps_c, const void* eps_u, float w, int64_t B, int64_t per_sample,
                 int dtype, void* workspace, size_t workspace_bytes, void* stream) {
  VD_REQUIRE(eps_c && eps_u && workspace, "null argument");
  VD_REQUIRE(B > 0 && B <= 65535 && per_sample > 0, "bad shape (B=%lld, per_sample=%lld)",
             (long long)B, (long long)per_sample);
  VD_REQUIRE(workspace_bytes >= vd_cfg_workspace_size(B, per_sample), "workspace too small");
  const int nb = cfg_blocks(per_sample);
  const int64_t chunk = cfg_chunk(per_sample, nb);
  const dim3 grid((unsigned)nb, (unsigned)B);
  const CfgGuide gd{w};
  float* part = static_cast<float*>(workspace);
  hipStream_t st = VD_STREAM(stream);
  const bool v8 = cfg_vec8(per_sample, {eps_c, eps_u});
  return VD_DISPATCH_DTYPE(dtype, T, {
    const T* c = (const T*)eps_c;
    const T* u = (const T*)eps_u;
    if (v8) {
      cfg_stats_kernel<T, 8, false><<<grid, kBlock, 0, st>>>(c, u, gd, per_sample, chunk, part);
      cfg_stats_kernel<T, 8, true><<<grid, kBlock, 0, st>>>(c, u, gd, per_sample, chunk, part);
    } else {
      cfg_stats_kernel<T, 1, false><<<grid, kBlock, 0, st>>>(c, u, gd, per_sample, chunk, part);
      cfg_stats_kernel<T, 1, true><<<grid, kBlock, 0, st>>>(c, u, gd, per_sample, chunk, part);
    }
  });
}

int vd_ddim_step_cfg_pred(const void* xt, const void* eps_c, const void* eps_u, const void* z,
                          void* x_prev, void* x_prev_dup, void* x0, const int64_t* t,
                          const int64_t* t_prev, const float* acp, float w, float rescale,
                          const void* workspace, float eta, int clip, int prediction,
                          int64_t B, int64_t per_sample, int dtype, void* stream) {
  return run_step(guided(ddim_args(xt, eps_c, eps_u, z, x_prev, x_prev_dup, x0, t, t_prev, acp,
                                   eta, clip, prediction, B, per_sample),
                         w, rescale, workspace, nullptr),
                  STEP_CFG, dtype, stream);
}

int vd_ddim_step_cfg(const void* xt, const void* eps_c, const void* eps_u, const void* z,
                     void* x_prev, void* x_prev_dup, void* x0, const int64_t* t,
                     const int64_t* t_prev, const float* acp, float w, float rescale,
                     const void* workspace, float eta, int clip, int64_t B, int64_t per_sample,
                     int dtype, void* stream) {
  return vd_ddim_step_cfg_pred(xt, eps_c, eps_u, z, x_prev, x_prev_dup, x0, t, t_prev, acp, w,
                               rescale, workspace, eta, clip, VD_PRED_EPS, B, per_sample, dtype,
                               stream);
}

int vd_dpm_step(const void* xt, const void* eps, void* x_prev, void* x0_hist, const float* coef,
                int64_t n_steps, const int64_t* step, int clip, int64_t B, int64_t per_sample,
                int dtype, void* stream) {
  return run_step(dpm_args(xt, eps, nullptr, x_prev, nullptr, x0_hist, coef, n_steps, step, clip,
                           B, per_sample),
                  STEP_PLAIN, dtype, stream);
}

int vd_dpm_step_cfg(const void* xt, const void* eps_c, const void* eps_u, void* x_prev,
                    void* x_prev_dup, void* x0_hist, const float* coef, int64_t n_steps,
                    const int64_t* step, float w, float rescale, const void* workspace, int clip,
                    int64_t B, int64_t per_sample, int dtype, void* stream) {
  return run_step(guided(dpm_args(xt, eps_c, eps_u, x_prev, x_prev_dup, x0_hist, coef, n_steps,
                                  step, clip, B, per_sample),
                         w, rescale, workspace, nullptr),
                  STEP_CFG, dtype, stream);
}

size_t vd_x0_quantile_workspace_size(int64_t B, int64_t per_sample) {
  if (B <= 0 || per_sample <= 0) return 0;
  return (thr_state_offset(B, cfg_blocks(per_sample)) + (size_t)B * kThrState) * sizeof(uint32_t);
}

int vd_x0_abs_quantile(const vd_x0_source* src, int64_t rank, float floor, float cap, int64_t B,
                       int64_t per_sample, int dtype, float* s, void* workspace,
                       size_t workspace_bytes, void* stream) {
  VD_REQUIRE(src && s && workspace, "null argument");
  VD_REQUIRE(B > 0 && B <= 65535 && per_sample > 0 && per_sample <= (int64_t)0xffffffffll,
             "bad shape (B=%lld, per_sample=%lld)", (long long)B, (long long)per_sample);
  VD_REQUIRE(rank >= 0 && rank < per_sample, "rank %lld outside [0, per_sample = %lld)",
             (long long)rank, (long long)per_sample);
  VD_REQUIRE(cap >= floor, "cap %g below floor %g", (double)cap, (double)floor);
  VD_REQUIRE(reinterpret_cast<uintptr_t>(workspace) % 4 == 0, "workspace must be 4-B aligned");
  VD_REQUIRE(workspace_bytes >= vd_x0_quantile_workspace_size(B, per_sample),
             "workspace too small");
  VD_REQUIRE(src->x, "null source tensor");
  X0Source xs = {};
  xs.rule = src->rule;
  if (src->rule == VD_X0_IDENTITY) {
    VD_REQUIRE(!src->eps && !src->eps_u, "the identity source reads x alone");
  } else if (src->rule == VD_X0_DDIM) {
    VD_REQUIRE(src->eps && src->t && src->acp, "DDIM source: null eps, t or acp");
    VD_REQUIRE(src->prediction == VD_PRED_EPS || src->prediction == VD_PRED_V,
               "unknown prediction type %d", src->prediction);
    xs.pred_v = src->prediction == VD_PRED_V;
    xs.ddim = make_ddim(src->acp, src->t, nullptr, 0.f, false);
  } else if (src->rule == VD_X0_DPM) {
    VD_REQUIRE(src->eps && src->coef && src->step && src->n_steps > 0,
               "DPM source: null eps, coef or step, or an empty table");
    xs.dpm = make_dpm(src->coef, src->n_steps, src->step);
  } else {
    return vd::fail(VD_EINVAL, "unknown x0 rule %d", src->rule);
  }
  if (src->eps_u) {
    VD_REQUIRE(src->rescale >= 0.f && src->rescale <= 1.f, "rescale %g outside [0, 1]",
               (double)src->rescale);
    VD_REQUIRE(src->rescale == 0.f || src->cfg_workspace,
               "rescale > 0 needs the vd_cfg_stats workspace (null)");
    xs.gd = CfgGuide{src->w};
    xs.part = static_cast<const float*>(src->cfg_workspace);
    xs.nb_cfg = cfg_blocks(per_sample);
    xs.phi = src->rescale;
  }
  const int nb = cfg_blocks(per_sample);
  const int64_t chunk = cfg_chunk(per_sample, nb);
  const dim3 grid((unsigned)nb, (unsigned)B);
  uint32_t* rows = static_cast<uint32_t*>(workspace);
  uint32_t* state = rows + thr_state_offset(B, nb);
  hipStream_t st = VD_STREAM(stream);
  const bool v8 = cfg_vec8(per_sample, {src->x, src->eps, src->eps_u});
  return VD_DISPATCH_DTYPE(dtype, T, {
    const T* x = (const T*)src->x;
    const T* c = (const T*)src->eps;
    const T* u = (const T*)src->eps_u;
    for (int shift = 24; shift >= 0; shift -= 8) {
      if (v8)
        x0_hist_kernel<T, 8><<<grid, kBlock, 0, st>>>(xs, x, c, u, per_sample, chunk, shift, rows,
                                                      state);
      else
        x0_hist_kernel<T, 1><<<grid, kBlock, 0, st>>>(xs, x, c, u, per_sample, chunk, shift, rows,
                                                      state);
      x0_scan_kernel<<<(unsigned)B, kThrBins * kThrScanParts, 0, st>>>(
          rows, nb, shift, (uint32_t)rank, floor, cap, state, s);
    }
  });
}

int vd_ddim_step_thr(const void* xt, const void* eps_c, const void* eps_u, const void* z,
                     void* x_prev, void* x_prev_dup, void* x0, const int64_t* t,
                     const int64_t* t_prev, const float* acp, float w, float rescale,
                     const void* workspace, float eta, int prediction, const float* thresh,
                     int64_t B, int64_t per_sample, int dtype, void* stream) {
  return run_step(guided(ddim_args(xt, eps_c, eps_u, z, x_prev, x_prev_dup, x0, t, t_prev, acp,
                                   eta, 0, prediction, B, per_sample),
                         w, rescale, workspace, thresh),
                  STEP_THR, dtype, stream);
}

int vd_dpm_step_thr(const void* xt, const void* eps_c, const void* eps_u, void* x_prev,
                    void* x_prev_dup, void* x0_hist, const float* coef, int64_t n_steps,
                    const int64_t* step, float w, float rescale, const void* workspace,
                    const float* thresh, int64_t B, int64_t per_sample, int dtype,
                    void* stream) {
  return run_step(guided(dpm_args(xt, eps_c, eps_u, x_prev, x_prev_dup, x0_hist, coef, n_steps,
                                  step, 0, B, per_sample),
                         w, rescale, workspace, thresh),
                  STEP_THR, dtype, stream);
}

int vd_ddim_step_known(const void* xt, const void* eps_c, const void* eps_u, const void* z,
                       void* x_prev, void* x_prev_dup, void* x0, const int64_t* t,
                       const int64_t* t_prev, const float* acp, float w, float rescale,
                       const void* workspace, float eta, int clip, int prediction,
                       const float* thresh, const void* known, const float* keep, int64_t Bk,
                       int64_t S, int64_t B, int64_t per_sample, int dtype, void* stream) {
  const StepArgs a = masked(guided(ddim_args(xt, eps_c, eps_u, z, x_prev, x_prev_dup, x0, t,
                                             t_prev, acp, eta, clip, prediction, B, per_sample),
                                   w, rescale, workspace, thresh),
                            known, keep, Bk, S);
  return run_step(a, kind_of(a), dtype, stream);
}

int vd_dpm_step_known(const void* xt, const void* eps_c, const void* eps_u, void* x_prev,
                      void* x_prev_dup, void* x0_hist, const float* coef, int64_t n_steps,
                      const int64_t* step, float w, float rescale, const void* workspace,
                      int clip, const float* thresh, const void* known, const float* keep,
                      int64_t Bk, int64_t S, int64_t B, int64_t per_sample, int dtype,
                      void* stream) {
  const StepArgs a = masked(guided(dpm_args(xt, eps_c, eps_u, x_prev, x_prev_dup, x0_hist, coef,
                                            n_steps, step, clip, B, per_sample),
                                   w, rescale, workspace, thresh),
                            known, keep, Bk, S);
  return run_step(a, kind_of(a), dtype, stream);
}

int vd_cfg_combine(const void* eps_c, const void* eps_u, void* eps_out, float w, float rescale,
                   const void* workspace, int64_t B, int64_t per_sample, int dtype,
                   void* stream) {
  VD_REQUIRE(eps_c && eps_u && eps_out, "null argument");
  VD_REQUIRE(B > 0 && B <= 65535 && per_sample > 0, "bad shape (B=%lld, per_sample=%lld)",
             (long long)B, (long long)per_sample);
  VD_REQUIRE(rescale >= 0.f && rescale <= 1.f, "rescale %g outside [0, 1]", (double)rescale);
  VD_REQUIRE(rescale == 0.f || workspace, "rescale > 0 needs the vd_cfg_stats workspace (null)");
  const CfgGuide gd{w};
  const int nb = cfg_blocks(per_sample);
  const float* part = static_cast<const float*>(workspace);
  hipStream_t st = VD_STREAM(stream);
  const bool v8 = cfg_vec8(per_sample, {eps_c, eps_u, eps_out});
  return VD_DISPATCH_DTYPE(dtype, T, {
    if (v8)
      cfg_combine_kernel<T, 8><<<cfg_grid(per_sample, 8, B), kBlock, 0, st>>>(
          gd, (const T*)eps_c, (const T*)eps_u, (T*)eps_out, part, nb, rescale, per_sample);
    else
      cfg_combine_kernel<T, 1><<<cfg_grid(per_sample, 1, B), kBlock, 0, st>>>(
          gd, (const T*)eps_c, (const T*)eps_u, (T*)eps_out, part, nb, rescale, per_sample);
  });
}

int vd_upsample_nearest_hw(const void* x, void* y, int B, int T, int H, int W, int C, int dtype,
                           void* stream) {
  VD_REQUIRE(x && y, "null argument");
  VD_REQUIRE(B > 0 && T > 0 && H > 0 && W > 0 && C > 0, "bad shape");
  const int64_t BT = (int64_t)B * T;
  const bool v8 = C % 8 == 0;
  const int64_t work = BT * H * W * (v8 ? C / 8 : C);
  return VD_DISPATCH_DTYPE(dtype, Tp, {
    if (v8)
      upsample_kernel<Tp, 8><<<grid_for(work), kBlock, 0, VD_STREAM(stream)>>>(
          (const Tp*)x, (Tp*)y, BT, H, W, C);
    else
      upsample_kernel<Tp, 1><<<grid_for(work), kBlock, 0, VD_STREAM(stream)>>>(
          (const Tp*)x, (Tp*)y, BT, H, W, C);
  });
}

int vd_upsample_nearest_hw_bwd(const void* dy, void* dx, int B, int T, int H, int W, int C,
                               int dtype, void* stream) {
  VD_REQUIRE(dy && dx, "null argument");
  VD_REQUIRE(B > 0 && T > 0 && H > 0 && W > 0 && C > 0, "bad shape");
  const int64_t BT = (int64_t)B * T;
  const bool v8 = C % 8 == 0;
  const int64_t work = BT * H * W * (v8 ? C / 8 : C);
  return VD_DISPATCH_DTYPE(dtype, Tp, {
    if (v8)
      upsample_bwd_kernel<Tp, 8><<<grid_for(work), kBlock, 0, VD_STREAM(stream)>>>(
          (const Tp*)dy, (Tp*)dx, BT, H, W, C);
    else
      upsample_bwd_kernel<Tp, 1><<<grid_for(work), kBlock, 0, VD_STREAM(stream)>>>(
          (const Tp*)dy, (Tp*)dx, BT, H, W, C);
  });
}

size_t vd_channel_sums_workspace_size(int B, int C) {
  if (B <= 0 || C <= 0) return 0;
  return (size_t)B * kSumBlocks * C * sizeof(float);
}

int vd_channel_sums(const void* x, int B, int64_t S, int C, int cstride, int dtype, float* out,
                    void* workspace, void* stream) {
  VD_REQUIRE(x && out && workspace, "null argument");
  VD_REQUIRE(B > 0 && S > 0 && C > 0 && C % 8 == 0 && C <= 2048, "bad shape B=%d C=%d", B, C);
  const int cs = cstride ? cstride : C;
  VD_REQUIRE(cs >= C && cs % 8 == 0, "bad channel stride %d", cs);
  hipStream_t st = VD_STREAM(stream);
  // about kSumBlocks blocks per sample, at least 4 row iterations each
  const int64_t rpi = 256 / (C / 8);
  int64_t blocks = g_csum_blocks;
  int64_t maxb = vd_cdiv(S, rpi * 4);
  if (blocks > maxb) blocks = maxb;
  if (blocks < 1) blocks = 1;
  const int64_t rows = vd_cdiv(S, blocks);
  blocks = vd_cdiv(S, rows);
  float* part = reinterpret_cast<float*>(workspace);
  return VD_DISPATCH_DTYPE(dtype, Tp, {
    if (g_csum_unroll >= 4)
      channel_sums_kernel<Tp, 4><<<dim3((unsigned)blocks, (unsigned)B), 256, 0, st>>>(
          (const Tp*)x, S, C, cs, rows, part);
    else
      channel_sums_kernel<Tp, 1><<<dim3((unsigned)blocks, (unsigned)B), 256, 0, st>>>(
          (const Tp*)x, S, C, cs, rows, part);
    channel_sums_finish_kernel<<<dim3((unsigned)vd_cdiv(C, 32), (unsigned)B), 1024, 0, st>>>(
        part, (int)blocks, C, out);
  });
}

int vd_conv_pack_weights(const vd_pack_desc* descs, int n, int64_t total, int dtype,
                         void* stream) {
  VD_REQUIRE(descs && n > 0 && n <= 1024 && total > 0, "bad pack job list");
  return VD_DISPATCH_DTYPE(dtype, Tp, {
    (void)total;
    pack_weights_kernel<Tp><<<2048, kBlock, kPackSmem, VD_STREAM(stream)>>>(descs, n);
  });
}

int vd_conv_pack_weight(const float* w, int Co, int Ci, int taps, int Cip, int Cop, int transpose,
                        int dtype, void* out, void* stream) {
  VD_REQUIRE(w && out, "null argument");
  VD_REQUIRE(Co > 0 && Ci > 0 && taps > 0 && Cip >= Ci && Cop >= Co, "bad weight shape");
  const int64_t total = transpose ? (int64_t)Cip * taps * Cop : (int64_t)Co * taps * Cip;
  return VD_DISPATCH_DTYPE(dtype, Tp, {
    pack_weight_kernel<Tp><<<grid_for(total), kBlock, 0, VD_STREAM(stream)>>>(
        w, Co, Ci, taps, Cip, Cop, transpose, (Tp*)out);
  });
}

}  // extern "C"
