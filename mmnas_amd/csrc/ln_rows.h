// What the float4 row-per-wave LayerNorm kernels share (the reference's modules.py:44-56: Bessel-corrected std, eps added to the
// std).  One wave holds one row: lane l keeps float4 v[NV] at columns 4 * (l + 64 * i), a lane's four values are summed as
// (x + y) + (z + w), lanes meet in wave_sum, columns c >= d hold zeros and are masked.
//   ln_row_apply      v = LayerNorm(v)                      mixed.hip node_mix_fwd_kernel / node_mix_bwd_kernel
//   ln_bwd_k2         coefficient of the backward's std term  every backward copy
// The row arithmetic itself stays written out in rowops.hip (ln_fwd_kernel, ln_bwd_kernel), mixed.hip (the LNB row), small.hip
// (sa_small_bwd_kernel) and vgdhead.hip (forward), although it is the same text.  The build contracts a * b + c, and in a sum of
// two products such as x * x + y * y the vectoriser decides which product is rounded and which rides in the fma.  At NV = 1 it
// decides differently from kernel to kernel (ln_fwd_kernel<1> rounds x * x, node_mix_fwd_kernel<1> rounds y * y; rows 0-1 and
// 2-3 of sa_small_bwd_kernel<256> differ from each other), so these copies never agreed to the last bit at d <= 256, and behind
// one helper each of them lands on one choice: results move by an ulp (profiles/r16_ln_rows_bits.txt).  NV >= 2 agrees.
// The partial-row hand-off of ln_bwd_kernel and of the LNB tail (pure additions: one helper gave the parent's bits) stays written
// out twice as well: behind one function ln_bwd_kernel<2> measured about 1 % slower at M = 6400, d = 512 on two boxes
// (profiles/r16_ln_rows_ab.txt).
// Copies whose arithmetic is another expression tree altogether:
//   small.hip's forward epilogues hold the row as float v[4 * NV] and add element by element (another summation order);
//   retrieval.hip itm_pair_head_kernel holds one float per lane; gemmln.hip keeps panel statistics across lanes;
//   vgdhead.hip's backward recovers sd from the saved 1 / (sd + eps) and gets g pre-multiplied; its six-row hand-off has its
//   own wave -> row map.
// tests/test_ln_rows_gpu.py holds all of them to the module's float64 autograd on degenerate rows.
#pragma once
#include "common.h"

namespace mmnas {

// v = LayerNorm(v), a and b read from memory
template <int NV>
__device__ __forceinline__ void ln_row_apply(float4 (&v)[NV], const float* __restrict__ a, const float* __restrict__ b, int lane, int d,
                                             float eps) {
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < NV; ++i) s += (v[i].x + v[i].y) + (v[i].z + v[i].w);
  const float mean = wave_sum(s) / (float)d;
  float ss = 0.f;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = (lane + 64 * i) * 4;
    if (c < d) {
      v[i].x -= mean; v[i].y -= mean; v[i].z -= mean; v[i].w -= mean;
      ss += (v[i].x * v[i].x + v[i].y * v[i].y) + (v[i].z * v[i].z + v[i].w * v[i].w);
    }
  }
  const float sd = sqrtf(wave_sum(ss) / (float)(d - 1));
  const float inv = 1.0f / (sd + eps);
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = (lane + 64 * i) * 4;
    if (c < d) {
      const float4 av = *reinterpret_cast<const float4*>(a + c);
      const float4 bv = *reinterpret_cast<const float4*>(b + c);
      v[i].x = av.x * v[i].x * inv + bv.x; v[i].y = av.y * v[i].y * inv + bv.y;
      v[i].z = av.z * v[i].z * inv + bv.z; v[i].w = av.w * v[i].w * inv + bv.w;
    }
  }
}

// The coefficient of the std term of every hand-written LayerNorm backward (rowops.hip ln_bwd_kernel and its copies in mixed.hip, small.hip, vgdhead.hip):
// sgc / (n1 * sd * sden^2), n1 = d - 1, sden = sd + eps, inv = 1 / sden, rn1 = 1 / n1 (row-invariant).  Two edges:
//   sd == 0 (a constant row): 0 -- the reference's autograd masks std's backward to 0 there, so dx = (g - mean(g)) / eps;
//     the plain quotient is 0 / 0.
//   the denominator overflows (sd above ~5e11): sgc * inv^3 / n1 -- sd + eps == sd there, so 1 / sd == inv; the plain
//     quotient is sgc / inf = 0 where the term is as large as the first one.
// The edges select the OPERANDS of the one quotient (0 / 1, big / 1), so the division stays unconditional and an ordinary
// row's quotient is the plain one.
__device__ __forceinline__ float ln_bwd_k2(float sgc, float n1, float rn1, float sd, float sden, float inv) {
  const float den = n1 * sd * sden * sden;
  const float big = ((sgc * inv) * inv) * (inv * rn1);
  const bool live = sd > 0.f, plain = live && den < __builtin_inff();
  const float num = plain ? sgc : (live ? big : 0.f);
  return num / (plain ? den : 1.f);
}

}  // namespace mmnas
