// Rounding of the two bf16 MFMA shapes, bit for bit (stand-alone; one wave per problem):
//   hipcc -O2 --offload-arch=gfx950 mfma_order.hip -o mfma_order && ./mfma_order
// D = C + A B over K = 32 as two chained v_mfma_f32_32x32x16_bf16 against one
// v_mfma_f32_16x16x32_bf16 per 16 x 16 tile whose lane group g holds the products k = 8 g .. 8 g + 7
// (the 8 of lane half hh of k-step s, g = 2 s + hh), on 4,096 random 32 x 32 x 32 problems (plain,
// wide operand exponents, large C, tiny C).  Measured on MI355X (profiles/r07_bwd_m16.md): 0
// of 4,194,304 outputs differ, also with the 8 slots of every group reversed; with the groups
// rotated by one lane group 5-44 % differ.  So the matrix core adds one lane group's 8 products
// to the accumulator at a time, in group order, and the order inside a group does not matter:
// a 16x16x32 kernel that keeps the 32x32x16 kernel's groups returns the same bits
// (attention.hip m16_chunk / m16_row).
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <cmath>
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
#define T 4096
__device__ bf16x8 ld8(const uint16_t* p, int stride) {
  uint16_t v[8];
  for (int e = 0; e < 8; ++e) v[e] = p[e * stride];
  bf16x8 r; memcpy(&r, v, 16); return r;
}
// A [T][32 rows][32 k], B [T][32 k][32 cols], C [T][32][32]
__global__ void k32(const uint16_t* A, const uint16_t* B, const float* C, float* D) {
  const int t = blockIdx.x, l = threadIdx.x, hh = l >> 5, rc = l & 31;
  A += t * 1024; B += t * 1024; C += t * 1024; D += t * 1024;
  f32x16 acc;
  for (int r = 0; r < 16; ++r) acc[r] = C[((r & 3) + 8 * (r >> 2) + 4 * hh) * 32 + rc];
  for (int s = 0; s < 2; ++s) {
    bf16x8 a = ld8(A + rc * 32 + 16 * s + 8 * hh, 1);
    bf16x8 b = ld8(B + (16 * s + 8 * hh) * 32 + rc, 32);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc, 0, 0, 0);
  }
  for (int r = 0; r < 16; ++r) D[((r & 3) + 8 * (r >> 2) + 4 * hh) * 32 + rc] = acc[r];
}
// rot: lane group g holds k block (g + rot) & 3 ; rev: slot e holds product 7 - e of the block
__global__ void k16(const uint16_t* A, const uint16_t* B, const float* C, float* D, int rot, int rev) {
  const int t = blockIdx.x, l = threadIdx.x, g = l >> 4, i = l & 15;
  A += t * 1024; B += t * 1024; C += t * 1024; D += t * 1024;
  const int kb = 8 * ((g + rot) & 3);
  for (int ti = 0; ti < 2; ++ti)
    for (int tj = 0; tj < 2; ++tj) {
      uint16_t va[8], vb[8];
      for (int e = 0; e < 8; ++e) {
        const int k = kb + (rev ? 7 - e : e);
        va[e] = A[(16 * ti + i) * 32 + k];
        vb[e] = B[k * 32 + 16 * tj + i];
      }
      bf16x8 a, b; memcpy(&a, va, 16); memcpy(&b, vb, 16);
      f32x4 c;
      for (int r = 0; r < 4; ++r) c[r] = C[(16 * ti + 4 * g + r) * 32 + 16 * tj + i];
      c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
      for (int r = 0; r < 4; ++r) D[(16 * ti + 4 * g + r) * 32 + 16 * tj + i] = c[r];
    }
}
static uint16_t bf(float x) { uint32_t u; memcpy(&u, &x, 4); u += 0x7fff + ((u >> 16) & 1); return u >> 16; }
static float rnd() { float s = 0; for (int i = 0; i < 4; ++i) s += rand() / (float)RAND_MAX - 0.5f; return s; }
int main() {
  const size_t n = (size_t)T * 1024;
  uint16_t *hA = new uint16_t[n], *hB = new uint16_t[n]; float* hC = new float[n];
  srand(7);
  for (size_t i = 0; i < n; ++i) {
    const int mode = (i / 1024) % 4;   // 0: plain, 1: wide exponents, 2: big C, 3: tiny C
    const float sa = mode == 1 ? ldexpf(1.f, rand() % 13 - 6) : 1.f;
    hA[i] = bf(rnd() * sa * 1.3f); hB[i] = bf(rnd() * (mode == 1 ? ldexpf(1.f, rand() % 13 - 6) : 1.f) * 1.3f);
    hC[i] = rnd() * (mode == 2 ? 4096.f : mode == 3 ? 1e-3f : 8.f);
  }
  uint16_t *A, *B; float *C, *D0, *D1;
  if (hipMalloc(&A, n * 2) || hipMalloc(&B, n * 2) || hipMalloc(&C, n * 4) || hipMalloc(&D0, n * 4) ||
      hipMalloc(&D1, n * 4)) { printf("alloc failed\n"); return 2; }
  hipMemcpy(A, hA, n * 2, hipMemcpyHostToDevice); hipMemcpy(B, hB, n * 2, hipMemcpyHostToDevice);
  hipMemcpy(C, hC, n * 4, hipMemcpyHostToDevice);
  float *h0 = new float[n], *h1 = new float[n];
  k32<<<T, 64>>>(A, B, C, D0);
  if (hipDeviceSynchronize() != hipSuccess) { printf("k32 failed\n"); return 3; }
  hipMemcpy(h0, D0, n * 4, hipMemcpyDeviceToHost);
  for (int v = 0; v < 4; ++v) {
    const int rot = v == 1, rev = v == 2;
    if (v == 3) { k32<<<T, 64>>>(A, B, C, D1); }  // control: the same kernel again
    else k16<<<T, 64>>>(A, B, C, D1, rot, rev);
    if (hipDeviceSynchronize() != hipSuccess) { printf("variant %d failed\n", v); return 3; }
    hipMemcpy(h1, D1, n * 4, hipMemcpyDeviceToHost);
    size_t bad[4] = {0, 0, 0, 0}; double worst = 0;
    for (size_t i = 0; i < n; ++i)
      if (memcmp(&h0[i], &h1[i], 4)) { ++bad[(i / 1024) % 4]; worst = fmax(worst, fabs(h0[i] - h1[i]) / fmax(fabs(h0[i]), 1e-30)); }
    printf("variant %d (%s): mismatches by data mode %zu %zu %zu %zu of %zu each, worst rel %.3g\n", v,
           v == 0 ? "16x16x32, block g = k 8g..8g+7" : v == 1 ? "16x16x32, blocks rotated by one group"
           : v == 2 ? "16x16x32, slots reversed inside each block" : "32x32x16 again (control)",
           bad[0], bad[1], bad[2], bad[3], n / 4, worst);
  }
  return 0;
}
