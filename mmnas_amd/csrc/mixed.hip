// Supernet node plumbing of the architecture step (MixedOp, mmnas/model/mixed.py):
//   * the gated sum of a node's candidate outputs (mixed.py:59-68) and its backward -- the gradient of every gate is
//     the inner product <dL/dout, o_j>, which the reference obtains from ~10 ATen kernels per candidate
//     (select, mul, add, and their autograd: expand, mul, sum);
//   * the architecture-parameter update of all nodes in one launch: dL/dalpha from dL/dgate (mixed.py:171-198,
//     'full' mode) followed by the Adam step of alpha_optim (search_vqa.py:194,331-332); for 'two' mode the gradient
//     over the sampled pair, the same Adam step and the pair's rescale (mixed.py:179-208, search_vqa.py:330-335).
// HBM-bound streaming kernels (one pass over the candidate outputs).
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "common.h"
#include "ln_rows.h"

namespace mmnas {

constexpr int MAXC = MMNAS_MIXED_MAX;
#define MMNAS_MIX_REDUCE_MAX 32
static_assert(MAXC == 8, "mixed_sum_reduce_kernel assumes 8 candidate slots");

struct MixArgs {
  const float* o[MAXC];
  int n;
};

__global__ void __launch_bounds__(256) mixed_sum_fwd_kernel(MixArgs a, const float* __restrict__ gate, float* __restrict__ out,
                                                            size_t n4) {
  float g[MAXC];
#pragma unroll
  for (int j = 0; j < MAXC; ++j) g[j] = j < a.n ? gate[j] : 0.f;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  // every candidate's loads of an element are issued before the first is used (the compiler hoists them out of
  // the unrolled loop): n independent 16-byte loads in flight per thread, one pass over each tensor
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
    float4 v[MAXC];
#pragma unroll
    for (int j = 0; j < MAXC; ++j)
      v[j] = (j < a.n && a.o[j]) ? reinterpret_cast<const float4*>(a.o[j])[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int j = 0; j < MAXC; ++j) { acc.x += g[j] * v[j].x; acc.y += g[j] * v[j].y; acc.z += g[j] * v[j].z; acc.w += g[j] * v[j].w; }
    reinterpret_cast<float4*>(out)[i] = acc;
  }
}

// partial inner products <dout, o_j> of this workgroup's slice -> part[blockIdx.x][MAXC]; d_active = gate[active] * dout
__global__ void __launch_bounds__(256) mixed_sum_bwd_kernel(MixArgs a, const float* __restrict__ gate, const float* __restrict__ dout,
                                                            float* __restrict__ d_active, int active, float* __restrict__ part,
                                                            size_t n4) {
  __shared__ float red[4][MAXC];
  float s[MAXC];
#pragma unroll
  for (int j = 0; j < MAXC; ++j) s[j] = 0.f;
  const float ga = d_active ? gate[active] : 0.f;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
    const float4 d = reinterpret_cast<const float4*>(dout)[i];
    float4 v[MAXC];
#pragma unroll
    for (int j = 0; j < MAXC; ++j)
      v[j] = (j < a.n && a.o[j]) ? reinterpret_cast<const float4*>(a.o[j])[i] : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int j = 0; j < MAXC; ++j) s[j] += (d.x * v[j].x + d.y * v[j].y) + (d.z * v[j].z + d.w * v[j].w);
    if (d_active) reinterpret_cast<float4*>(d_active)[i] = make_float4(ga * d.x, ga * d.y, ga * d.z, ga * d.w);
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int j = 0; j < MAXC; ++j) {
    const float t = wave_sum(s[j]);
    if (lane == 0) red[wave][j] = t;
  }
  __syncthreads();
  if (threadIdx.x < MAXC)
    part[(size_t)blockIdx.x * MAXC + threadIdx.x] = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
}

// dgate[j] += sum over workgroups, in a fixed order (bitwise reproducible): 256 threads = 8 candidates x 32 strided
// partial sums, then a fixed-order tree through LDS.  (A single thread per candidate walking all 2048 partials was a
// chain of 2048 dependent loads: 105 us per node, a fifth of the architecture step.)
__global__ void __launch_bounds__(256) mixed_sum_reduce_kernel(const float* __restrict__ part, int nwg, int n, float* __restrict__ dgate) {
  __shared__ float red[32][MAXC + 1];
  const int j = threadIdx.x & (MAXC - 1), g = threadIdx.x / MAXC;   // MAXC = 8: 32 groups
  float t0 = 0.f, t1 = 0.f, t2 = 0.f, t3 = 0.f;
  int b = g;
  for (; b + 96 < nwg; b += 128) {
    t0 += part[(size_t)b * MAXC + j];
    t1 += part[(size_t)(b + 32) * MAXC + j];
    t2 += part[(size_t)(b + 64) * MAXC + j];
    t3 += part[(size_t)(b + 96) * MAXC + j];
  }
  for (; b < nwg; b += 32) t0 += part[(size_t)b * MAXC + j];
  red[g][j] = (t0 + t1) + (t2 + t3);
  __syncthreads();
  if (threadIdx.x < n) {
    float t = 0.f;
#pragma unroll
    for (int i = 0; i < 32; ++i) t += red[i][threadIdx.x];
    dgate[threadIdx.x] += t;
  }
}

// The same reduction for MANY nodes in one launch (the backbone chain of the architecture step defers its 30 nodes'
// reductions to the end of its backward: one workgroup per node instead of 30 one-workgroup launches of ~5 us each).
struct MixReduceJobs {
  const float* part[MMNAS_MIX_REDUCE_MAX];
  float* dgate[MMNAS_MIX_REDUCE_MAX];
  int nwg[MMNAS_MIX_REDUCE_MAX];
  int n[MMNAS_MIX_REDUCE_MAX];
};
__global__ void __launch_bounds__(256) mixed_sum_reduce_many_kernel(const MixReduceJobs jobs) {
  __shared__ float red[32][MAXC + 1];
  const float* __restrict__ part = jobs.part[blockIdx.x];
  float* __restrict__ dgate = jobs.dgate[blockIdx.x];
  const int nwg = jobs.nwg[blockIdx.x], n = jobs.n[blockIdx.x];
  const int j = threadIdx.x & (MAXC - 1), g = threadIdx.x / MAXC;
  float t0 = 0.f, t1 = 0.f, t2 = 0.f, t3 = 0.f;
  int b = g;
  for (; b + 96 < nwg; b += 128) {
    t0 += part[(size_t)b * MAXC + j];
    t1 += part[(size_t)(b + 32) * MAXC + j];
    t2 += part[(size_t)(b + 64) * MAXC + j];
    t3 += part[(size_t)(b + 96) * MAXC + j];
  }
  for (; b < nwg; b += 32) t0 += part[(size_t)b * MAXC + j];
  red[g][j] = (t0 + t1) + (t2 + t3);
  __syncthreads();
  if (threadIdx.x < n) {
    float t = 0.f;
#pragma unroll
    for (int i = 0; i < 32; ++i) t += red[i][threadIdx.x];
    dgate[threadIdx.x] += t;
  }
}

// ---- node epilogue of the architecture step: every candidate's LayerNorm AND the gated sum in one pass ----
// A supernet node in modes 'full' / 'two' evaluates n candidates on the same input; each ends in its own LayerNorm
// (modules.py:52-56, wrapper :266-268) and the node's output is sum_j gate_j LN_j(z_j) (mixed.py:59-68).  As separate
// launches that is n LayerNorm kernels (read z_j, write y_j) plus the gated sum (read every y_j, write out): 2n + 1
// passes over [M, d] and n + 1 launches per node, 30 nodes per step.  Here: one wave per row reads the n pre-LayerNorm
// rows, normalises each in registers and writes only the node output -- n + 1 passes, one launch; the candidates' own
// outputs y_j are never stored.  The backward needs them once more for the gate gradients <dout, y_j>: it recomputes
// them from z_j the same way.  A candidate without LayerNorm (or one whose kernel normalised already) passes
// ln_a = NULL and its output as z.
struct NodeMixArgs {
  const float* z[MAXC];
  const float* a[MAXC];
  const float* b[MAXC];
  int n;
};

template <int NV>
__global__ void __launch_bounds__(256) node_mix_fwd_kernel(NodeMixArgs p, const float* __restrict__ gate, float* __restrict__ out,
                                                           int M, int d, float eps) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;
  float4 acc[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) acc[i] = make_float4(0.f, 0.f, 0.f, 0.f);
  float4 v[MAXC][NV];
#pragma unroll
  for (int j = 0; j < MAXC; ++j)     // every candidate's row in flight before the first reduction
    if (j < p.n && p.z[j]) {         // (z == NULL: a candidate of the node that was not evaluated -- mode 'two')
      const float* zr = p.z[j] + (size_t)row * d;
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        const int c = (lane + 64 * i) * 4;
        v[j][i] = (c < d) ? *reinterpret_cast<const float4*>(zr + c) : make_float4(0.f, 0.f, 0.f, 0.f);
      }
    }
#pragma unroll
  for (int j = 0; j < MAXC; ++j)
    if (j < p.n && p.z[j]) {
      if (p.a[j]) ln_row_apply<NV>(v[j], p.a[j], p.b[j], lane, d, eps);
      const float g = gate[j];
#pragma unroll
      for (int i = 0; i < NV; ++i) { acc[i].x += g * v[j][i].x; acc[i].y += g * v[j][i].y; acc[i].z += g * v[j][i].z; acc[i].w += g * v[j][i].w; }
    }
  float* o = out + (size_t)row * d;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = (lane + 64 * i) * 4;
    if (c < d) *reinterpret_cast<float4*>(o + c) = acc[i];
  }
}

// part[blockIdx.x][j] = sum over this workgroup's rows of <dout, LN_j(z_j)>; d_active = gate[active] * dout.
// LNB (round 6): the sampled candidate's LayerNorm BACKWARD happens here as well -- its row z_active is already in registers
// for the gate's inner product, and d_active = gate[active] * dout would only be written to be read back by the candidate's
// own ln_bwd launch (8 us + a launch boundary per node of the architecture step).  With LNB the kernel writes dz (gradient
// wrt z_active), dt (the same behind the candidate's output dropout, replayed; NULL: none) and leaves the LayerNorm
// parameter partials [workgroup][3][d] (dln_a, dln_b, column sums of dt) as ln_bwd_kernel (rowops.hip) does -- the same
// expressions (written out here: the last bit differs between the two, ln_rows.h), the same hand-off, the same row -> workgroup
// map (<= 512 workgroups) -- and d_active is not written.
template <int NV, bool LNB>
__global__ void __launch_bounds__(256) node_mix_bwd_kernel(NodeMixArgs p, const float* __restrict__ gate, const float* __restrict__ dout,
                                                           float* __restrict__ d_active, int active, float* __restrict__ part,
                                                           int M, int d, float eps, float* __restrict__ ln_dz, float* __restrict__ ln_dt,
                                                           float* __restrict__ ln_part, DropCfg ln_drop) {
  __shared__ float red[4][MAXC];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float s[MAXC];
#pragma unroll
  for (int j = 0; j < MAXC; ++j) s[j] = 0.f;
  const float ga = (d_active || LNB) ? gate[active] : 0.f;
  float4 acc_a[NV], acc_b[NV], acc_c[NV], lnav[NV], lnbv[NV];
  if (LNB) {
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int c = (lane + 64 * i) * 4;
      acc_a[i] = make_float4(0.f, 0.f, 0.f, 0.f); acc_b[i] = acc_a[i]; acc_c[i] = acc_a[i];
      lnav[i] = (c < d) ? *reinterpret_cast<const float4*>(p.a[active] + c) : acc_a[i];
      lnbv[i] = (c < d) ? *reinterpret_cast<const float4*>(p.b[active] + c) : acc_a[i];
    }
  }
  for (int row = blockIdx.x * 4 + wave; row < M; row += gridDim.x * 4) {
    float4 g4[NV];
    const float* dr = dout + (size_t)row * d;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int c = (lane + 64 * i) * 4;
      g4[i] = (c < d) ? *reinterpret_cast<const float4*>(dr + c) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    float4 v[MAXC][NV];
#pragma unroll
    for (int j = 0; j < MAXC; ++j)
      if (j < p.n && p.z[j]) {
        const float* zr = p.z[j] + (size_t)row * d;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
          const int c = (lane + 64 * i) * 4;
          v[j][i] = (c < d) ? *reinterpret_cast<const float4*>(zr + c) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
      }
    if (d_active && !LNB) {
      float* ar = d_active + (size_t)row * d;
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        const int c = (lane + 64 * i) * 4;
        if (c < d) *reinterpret_cast<float4*>(ar + c) = make_float4(ga * g4[i].x, ga * g4[i].y, ga * g4[i].z, ga * g4[i].w);
      }
    }
#pragma unroll
    for (int j = 0; j < MAXC; ++j)
      if (j < p.n && p.z[j]) {
        if (LNB && j == active) {
          // LayerNorm forward (for the gate's inner product) AND backward of the sampled candidate: ln_fwd / ln_bwd_kernel's
          // arithmetic on the row in registers; g = ga * dout is the gradient of the candidate's output
          float4* vv = v[j];
          float t = 0.f;
#pragma unroll
          for (int i = 0; i < NV; ++i) t += (vv[i].x + vv[i].y) + (vv[i].z + vv[i].w);
          const float mean = wave_sum(t) / (float)d;
          float ss = 0.f, sg = 0.f, sgc = 0.f;
          float4 gy[NV];
#pragma unroll
          for (int i = 0; i < NV; ++i) {
            const int c = (lane + 64 * i) * 4;
            gy[i] = make_float4(ga * g4[i].x, ga * g4[i].y, ga * g4[i].z, ga * g4[i].w);
            if (c < d) {
              vv[i].x -= mean; vv[i].y -= mean; vv[i].z -= mean; vv[i].w -= mean;
              ss += (vv[i].x * vv[i].x + vv[i].y * vv[i].y) + (vv[i].z * vv[i].z + vv[i].w * vv[i].w);
              const float gx = gy[i].x * lnav[i].x, gyy = gy[i].y * lnav[i].y, gz = gy[i].z * lnav[i].z, gw = gy[i].w * lnav[i].w;
              sg += (gx + gyy) + (gz + gw);
              sgc += (gx * vv[i].x + gyy * vv[i].y) + (gz * vv[i].z + gw * vv[i].w);
            }
          }
          ss = wave_sum(ss); sg = wave_sum(sg); sgc = wave_sum(sgc);
          const float sd = sqrtf(ss / (float)(d - 1));
          const float sden = sd + eps;
          const float inv = 1.0f / sden;
          const float mg = sg / (float)d;
          const float k2 = ln_bwd_k2(sgc, (float)(d - 1), 1.0f / (float)(d - 1), sd, sden, inv);
#pragma unroll
          for (int i = 0; i < NV; ++i) {
            const int c = (lane + 64 * i) * 4;
            if (c < d) {
              // the candidate's output row (ln_fwd's expression) for the gate gradient
              s[j] += (g4[i].x * (lnav[i].x * vv[i].x * inv + lnbv[i].x) + g4[i].y * (lnav[i].y * vv[i].y * inv + lnbv[i].y)) +
                      (g4[i].z * (lnav[i].z * vv[i].z * inv + lnbv[i].z) + g4[i].w * (lnav[i].w * vv[i].w * inv + lnbv[i].w));
              float4 o;
              o.x = (gy[i].x * lnav[i].x - mg) * inv - vv[i].x * k2;
              o.y = (gy[i].y * lnav[i].y - mg) * inv - vv[i].y * k2;
              o.z = (gy[i].z * lnav[i].z - mg) * inv - vv[i].z * k2;
              o.w = (gy[i].w * lnav[i].w - mg) * inv - vv[i].w * k2;
              *reinterpret_cast<float4*>(ln_dz + (size_t)row * d + c) = o;
              acc_a[i].x += gy[i].x * vv[i].x * inv; acc_a[i].y += gy[i].y * vv[i].y * inv;
              acc_a[i].z += gy[i].z * vv[i].z * inv; acc_a[i].w += gy[i].w * vv[i].w * inv;
              acc_b[i].x += gy[i].x; acc_b[i].y += gy[i].y; acc_b[i].z += gy[i].z; acc_b[i].w += gy[i].w;
              if (ln_dt) {
                if (ln_drop.thresh) {
                  const uint32_t base = (uint32_t)row * (uint32_t)d + (uint32_t)c;
                  o.x *= drop_mult(ln_drop, base); o.y *= drop_mult(ln_drop, base + 1);
                  o.z *= drop_mult(ln_drop, base + 2); o.w *= drop_mult(ln_drop, base + 3);
                }
                *reinterpret_cast<float4*>(ln_dt + (size_t)row * d + c) = o;
                acc_c[i].x += o.x; acc_c[i].y += o.y; acc_c[i].z += o.z; acc_c[i].w += o.w;
              }
            }
          }
          continue;
        }
        if (p.a[j]) ln_row_apply<NV>(v[j], p.a[j], p.b[j], lane, d, eps);
#pragma unroll
        for (int i = 0; i < NV; ++i)
          s[j] += (g4[i].x * v[j][i].x + g4[i].y * v[j][i].y) + (g4[i].z * v[j][i].z + g4[i].w * v[j][i].w);
      }
  }
#pragma unroll
  for (int j = 0; j < MAXC; ++j) {
    const float t = wave_sum(s[j]);
    if (lane == 0) red[wave][j] = t;
  }
  __syncthreads();
  if (threadIdx.x < MAXC)
    part[(size_t)blockIdx.x * MAXC + threadIdx.x] = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
  if (LNB) {   // the LayerNorm parameter partials of this workgroup: ln_bwd_kernel's reduction (16-byte reads, one row store per wave < 3)
    __shared__ __attribute__((aligned(16))) float lred[3][4][64 * 4];
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int c = (lane + 64 * i) * 4;
      __syncthreads();
      *reinterpret_cast<float4*>(&lred[0][wave][lane * 4]) = acc_a[i];
      *reinterpret_cast<float4*>(&lred[1][wave][lane * 4]) = acc_b[i];
      *reinterpret_cast<float4*>(&lred[2][wave][lane * 4]) = acc_c[i];
      __syncthreads();
      if (wave < 3 && c < d) {
        const f32x4 p0 = *reinterpret_cast<const f32x4*>(&lred[wave][0][lane * 4]);
        const f32x4 p1 = *reinterpret_cast<const f32x4*>(&lred[wave][1][lane * 4]);
        const f32x4 p2 = *reinterpret_cast<const f32x4*>(&lred[wave][2][lane * 4]);
        const f32x4 p3 = *reinterpret_cast<const f32x4*>(&lred[wave][3][lane * 4]);
        *reinterpret_cast<f32x4*>(ln_part + ((size_t)blockIdx.x * 3 + wave) * d + c) = (p0 + p1) + (p2 + p3);
      }
    }
  }
}

// The expected-cost term of the hardware-aware search (ProxylessNAS, section 3.3): with p = softmax(alpha_r) over the whole
// row, E_r = sum_j p_j cost[r, j] and E = sum_r E_r, the regulariser R is weight * (E - ref) / ref ('linear', k = weight / ref)
// or weight * log(E / ref) ('log', k = weight / E), and dR/dalpha[r, j] = k p_j (cost[r, j] - E_r) on every live column.
struct AlphaCost {
  const float* cost;   // [rows, width], 0 in the padding columns
  float* stats;        // nullable: E_r per row, then E, then R
  float weight, ref;
  int form;            // 0 linear, 1 log
};

// E_r of one row (padding columns hold -inf: exp = 0)
__device__ __forceinline__ float alpha_row_expected_cost(const float* __restrict__ a, const float* __restrict__ c, int width) {
  float mx = -INFINITY;
  for (int i = 0; i < width; ++i) mx = fmaxf(mx, a[i]);
  float den = 0.f;
  for (int i = 0; i < width; ++i) den += expf(a[i] - mx);
  float e = 0.f;
  for (int i = 0; i < width; ++i) e += (expf(a[i] - mx) / den) * c[i];
  return e;
}

// Pass 1 of the cost kernels, one 256-thread workgroup: thread t takes the rows t, t + 256, ... in that order, the waves' sums
// (lane permutations) meet in LDS and every thread adds the four in one fixed order -- no atomics, the same bits on every call.
// Returns k (see AlphaCost); thread 0 stores E and R.  The barrier inside also separates every read of the old alphas (the
// total is needed before any alpha moves: 'log' divides by it) from the first store of pass 2.
__device__ __forceinline__ float alpha_cost_scale(const float* __restrict__ prob, int rows, int width, const AlphaCost& ac) {
  __shared__ float red[4];
  float part = 0.f;
  for (int r = threadIdx.x; r < rows; r += 256) {
    const float e = alpha_row_expected_cost(prob + (size_t)r * width, ac.cost + (size_t)r * width, width);
    if (ac.stats) ac.stats[r] = e;
    part += e;
  }
  part = wave_sum(part);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = part;
  __syncthreads();
  const float E = (red[0] + red[1]) + (red[2] + red[3]);
  float k = 0.f, R = 0.f;
  if (ac.form == 0) {
    k = ac.weight / ac.ref;
    R = ac.weight * (E - ac.ref) / ac.ref;
  } else if (E > 0.f) {                                     // (E <= 0: every positive-cost candidate underflowed -- no term)
    k = ac.weight / E;
    R = ac.weight * logf(E / ac.ref);
  }
  if (ac.stats && threadIdx.x == 0) {
    ac.stats[rows] = E;
    ac.stats[rows + 1] = R;
  }
  return k;
}

// one node (row) of the 'full'-mode architecture gradient + Adam; COST: plus k p_i (cost_i - E_r)
template <bool COST>
__device__ __forceinline__ void alpha_full_row(float* __restrict__ prob, const float* __restrict__ gate_grad, float* __restrict__ m,
                                               float* __restrict__ v, float* __restrict__ prob_grad, int r, int width, float lr,
                                               float b1, float b2, float omb1, float omb2, float eps, float c1, float c2s, float wd,
                                               const float* __restrict__ cost, float k) {
  float* a = prob + (size_t)r * width;
  const float* g = gate_grad + (size_t)r * width;
  float mx = -INFINITY;
  for (int i = 0; i < width; ++i) mx = fmaxf(mx, a[i]);
  float den = 0.f;
  for (int i = 0; i < width; ++i) den += expf(a[i] - mx);   // padding columns hold -inf: exp = 0
  float dot = 0.f;
  for (int i = 0; i < width; ++i) dot += g[i] * (expf(a[i] - mx) / den);
  float er = 0.f;
  if (COST)
    for (int i = 0; i < width; ++i) er += (expf(a[i] - mx) / den) * cost[(size_t)r * width + i];
  for (int i = 0; i < width; ++i) {
    const float p = expf(a[i] - mx) / den;
    float grad = p * (g[i] - dot);                          // sum_j g_j p_j (delta_ij - p_i), mixed.py:194-198
    if (COST) grad += k * p * (cost[(size_t)r * width + i] - er);
    if (prob_grad) prob_grad[(size_t)r * width + i] = grad;
    if (p == 0.f && !(a[i] > -INFINITY)) continue;          // padding column: stays -inf
    if (wd != 0.f) grad += wd * a[i];                       // torch Adam's weight_decay (ALPHA_WEIGHT_DECAY): p.grad itself stays as it is
    const size_t o = (size_t)r * width + i;
    const float mi = b1 * m[o] + omb1 * grad;
    const float vi = b2 * v[o] + omb2 * grad * grad;
    m[o] = mi; v[o] = vi;
    a[i] -= (lr / c1) * mi / (sqrtf(vi) / c2s + eps);
  }
}

// one thread per node (row): 'full'-mode architecture gradient + Adam
__global__ void alpha_full_step_kernel(float* __restrict__ prob, const float* __restrict__ gate_grad, float* __restrict__ m,
                                       float* __restrict__ v, float* __restrict__ prob_grad, int rows, int width, float lr,
                                       float b1, float b2, float omb1, float omb2, float eps, float c1, float c2s, float wd) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= rows) return;
  alpha_full_row<false>(prob, gate_grad, m, v, prob_grad, r, width, lr, b1, b2, omb1, omb2, eps, c1, c2s, wd, nullptr, 0.f);
}

// the same with the expected-cost term: ONE workgroup of 256 threads walks the rows (alpha_cost_scale says why)
__global__ __launch_bounds__(256) void alpha_full_step_cost_kernel(float* __restrict__ prob, const float* __restrict__ gate_grad,
                                                                   float* __restrict__ m, float* __restrict__ v,
                                                                   float* __restrict__ prob_grad, int rows, int width, float lr,
                                                                   float b1, float b2, float omb1, float omb2, float eps, float c1,
                                                                   float c2s, float wd, AlphaCost ac) {
  const float k = alpha_cost_scale(prob, rows, width, ac);
  for (int r = threadIdx.x; r < rows; r += 256)
    alpha_full_row<true>(prob, gate_grad, m, v, prob_grad, r, width, lr, b1, b2, omb1, omb2, eps, c1, c2s, wd, ac.cost, k);
}

// one thread per node (row): 'two'-mode architecture gradient over the sampled pair + Adam over the row + the pair's
// mass-preserving rescale (mixed.py:179-208, search_vqa.py:330-335).  The pairs travel in the kernel arguments.
constexpr int ALPHA_TWO_MAX_ROWS = 128;                    // mmnas_onehot_rows' limit: 1 KB of kernel arguments
struct AlphaPairArgs { int ij[ALPHA_TWO_MAX_ROWS * 2]; };   // (active, inactive) per row

// COST: k p_i (cost_i - E_r), p the softmax over the WHOLE row, joins the pair gradient on every live column (the regulariser
// reaches all paths, the binary-gate gradient the sampled two)
template <bool COST>
__device__ __forceinline__ void alpha_two_row(float* __restrict__ prob, const float* __restrict__ gate_grad, float* __restrict__ m,
                                              float* __restrict__ v, float* __restrict__ prob_grad, int r, int width, float lr,
                                              float b1, float b2, float omb1, float omb2, float eps, float c1, float c2s, float wd,
                                              int pi, int pj, const float* __restrict__ cost, float k) {
  float* a = prob + (size_t)r * width;
  const float* g = gate_grad + (size_t)r * width;
  const float oi = a[pi], oj = a[pj];                       // the pair's logits before Adam
  const float mx = fmaxf(oi, oj);
  const float ei = expf(oi - mx), ej = expf(oj - mx);
  const float den = ei + ej;
  const float si = ei / den, sj = ej / den;                 // softmax over the pair only (mixed.py:181)
  const float gpi = g[pi] * si, gpj = g[pj] * sj;
  const float dot = gpi + gpj;
  const float gi = gpi - si * dot, gj = gpj - sj * dot;     // sum_k g_k p_k (delta_ik - p_i) over the pair (mixed.py:182-186)
  float rmx = -INFINITY, rden = 0.f, er = 0.f;
  if (COST) {
    for (int i = 0; i < width; ++i) rmx = fmaxf(rmx, a[i]);
    for (int i = 0; i < width; ++i) rden += expf(a[i] - rmx);
    for (int i = 0; i < width; ++i) er += (expf(a[i] - rmx) / rden) * cost[(size_t)r * width + i];
  }
  for (int i = 0; i < width; ++i) {
    float grad = i == pi ? gi : (i == pj ? gj : 0.f);
    const size_t o = (size_t)r * width + i;
    const float ai = a[i];
    if (COST) grad += k * (expf(ai - rmx) / rden) * (cost[o] - er);
    if (prob_grad) prob_grad[o] = grad;
    if (!(ai > -INFINITY)) continue;                        // padding column: stays -inf, its moments untouched
    if (wd != 0.f) grad += wd * ai;                         // torch Adam's weight_decay: p.grad itself stays as it is
    const float mi = b1 * m[o] + omb1 * grad;               // omb = 1 - beta, formed on the host (adam_coef)
    const float vi = b2 * v[o] + omb2 * grad * grad;
    m[o] = mi; v[o] = vi;
    a[i] = ai - (lr / c1) * mi / (sqrtf(vi) / c2s + eps);
  }
  // rescale_updated_arch_param (mixed.py:200-208): offset = logsumexp(new pair) - logsumexp(old pair), in double as the
  // reference's math.log / math.exp; the differences of the maxima and of the logs are taken apart, so nothing cancels
  const float ni = a[pi], nj = a[pj];
  const float nmx = fmaxf(ni, nj);
  const double nden = exp((double)ni - (double)nmx) + exp((double)nj - (double)nmx);
  const double oden = exp((double)oi - (double)mx) + exp((double)oj - (double)mx);
  const double off = ((double)nmx - (double)mx) + log(nden / oden);
  a[pi] = (float)((double)ni - off);
  a[pj] = (float)((double)nj - off);
}

__global__ void alpha_two_step_kernel(float* __restrict__ prob, const float* __restrict__ gate_grad, float* __restrict__ m,
                                      float* __restrict__ v, float* __restrict__ prob_grad, int rows, int width, float lr,
                                      float b1, float b2, float omb1, float omb2, float eps, float c1, float c2s, float wd,
                                      AlphaPairArgs pa) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= rows) return;
  alpha_two_row<false>(prob, gate_grad, m, v, prob_grad, r, width, lr, b1, b2, omb1, omb2, eps, c1, c2s, wd, pa.ij[2 * r],
                       pa.ij[2 * r + 1], nullptr, 0.f);   // (checked on the host: 0 <= pi != pj < width)
}

// the same with the expected-cost term: one workgroup of 256 threads (rows <= ALPHA_TWO_MAX_ROWS: a single pass each)
__global__ __launch_bounds__(256) void alpha_two_step_cost_kernel(float* __restrict__ prob, const float* __restrict__ gate_grad,
                                                                  float* __restrict__ m, float* __restrict__ v,
                                                                  float* __restrict__ prob_grad, int rows, int width, float lr,
                                                                  float b1, float b2, float omb1, float omb2, float eps, float c1,
                                                                  float c2s, float wd, AlphaPairArgs pa, AlphaCost ac) {
  const float k = alpha_cost_scale(prob, rows, width, ac);
  for (int r = threadIdx.x; r < rows; r += 256)
    alpha_two_row<true>(prob, gate_grad, m, v, prob_grad, r, width, lr, b1, b2, omb1, omb2, eps, c1, c2s, wd, pa.ij[2 * r],
                        pa.ij[2 * r + 1], ac.cost, k);
}

// The REINFORCE architecture update (ProxylessNAS section 3.3.2, MnasNet's reward): M sampled architectures a_i (one candidate
// per row), their task rewards Q_i on the device, an optional price C_i = sum_r cost[r, a_ir] of each, a moving-average baseline.
// The sampled indices travel in the kernel arguments, one byte each.
constexpr int ALPHA_REINFORCE_MAX_CHOICES = 3072;          // M * rows: 3 KB of the 4 KB argument block (300 x 4, 128 x 16, ...)
constexpr int ALPHA_REINFORCE_MAX_SAMPLES = 256;           // M: thread i prices sample i
struct AlphaChoiceArgs { unsigned char a[ALPHA_REINFORCE_MAX_CHOICES]; };   // [M, rows]

struct AlphaReinforce {
  const float* quality;  // [M]
  const float* cost;     // nullable (also when cost_weight == 0): R_i = Q_i
  float* baseline;       // (value, initialised)
  float* stats;          // nullable: R_0 .. R_{M-1}, mean R, baseline used, baseline after
  int* err;
  double decay, omd;     // baseline_decay and 1 - baseline_decay, formed on the host from the decimal the caller wrote
  float weight, ref;
  int form;              // 0 mul, 1 add
  int M;
};

// one row of the REINFORCE gradient + Adam.  sA: A_i = R_i - b in LDS, in double; sum_a their sum, samples ascending.  The sum
// over the samples that chose a column runs in double in the same order: where every sample chose one column it IS sum_a, bit
// for bit, and the column's gradient -(1 - p) sum_a / M is as small as sum_a is (the first update: rounding noise of 1e-17,
// which Adam's eps = 1e-8 still swallows; float sums would leave 1e-9 there and Adam would step by it).  The row arithmetic (softmax over the
// live columns, the Adam body) is alpha_full_row's text; it is written out again here and not shared through a helper, so that
// the four existing alpha kernels keep their instruction streams, registers and bits exactly.
__device__ __forceinline__ void alpha_reinforce_row(float* __restrict__ prob, float* __restrict__ m, float* __restrict__ v,
                                                    float* __restrict__ prob_grad, int r, int rows, int width, int M,
                                                    const double* sA, double sum_a, const AlphaChoiceArgs& ch, float lr, float b1,
                                                    float b2, float omb1, float omb2, float eps, float c1, float c2s, float wd) {
  float* a = prob + (size_t)r * width;
  float mx = -INFINITY;
  for (int i = 0; i < width; ++i) mx = fmaxf(mx, a[i]);
  float den = 0.f;
  for (int i = 0; i < width; ++i) den += expf(a[i] - mx);   // padding columns hold -inf: exp = 0
  for (int i = 0; i < width; ++i) {
    const float ai = a[i];
    const float p = expf(ai - mx) / den;
    double hit = 0.0;                                       // sum of A_k over the samples that chose column i, k ascending
    for (int k = 0; k < M; ++k)
      if ((int)ch.a[k * rows + r] == i) hit += sA[k];
    float grad = (float)(-(hit - (double)p * sum_a) / (double)M);
    const size_t o = (size_t)r * width + i;
    if (prob_grad) prob_grad[o] = grad;
    if (!(ai > -INFINITY)) continue;                        // padding column: stays -inf, its moments untouched
    if (wd != 0.f) grad += wd * ai;                         // torch Adam's weight_decay: prob_grad keeps the undecayed gradient
    const float mi = b1 * m[o] + omb1 * grad;
    const float vi = b2 * v[o] + omb2 * grad * grad;
    m[o] = mi; v[o] = vi;
    a[i] = ai - (lr / c1) * mi / (sqrtf(vi) / c2s + eps);
  }
}

// ONE workgroup of 256 threads.  Thread i < M prices sample i (rows ascending, in double) and forms R_i; a non-finite Q_i or R_i ends the
// kernel with *err = 1 before anything is written.  Every thread then forms mean R, b and sum_i A_i in double, samples
// ascending (no atomics, no cross-lane sums: the same bits on every call), thread 0 moves the baseline, and the threads walk
// the rows r, r + 256, ...  The baseline is read by everyone before the barrier and written by thread 0 after it.
__global__ __launch_bounds__(256) void alpha_reinforce_step_kernel(float* __restrict__ prob, float* __restrict__ m,
                                                                   float* __restrict__ v, float* __restrict__ prob_grad, int rows,
                                                                   int width, float lr, float b1, float b2, float omb1, float omb2,
                                                                   float eps, float c1, float c2s, float wd, AlphaReinforce ar,
                                                                   AlphaChoiceArgs ch) {
  __shared__ float sR[ALPHA_REINFORCE_MAX_SAMPLES];
  __shared__ double sA[ALPHA_REINFORCE_MAX_SAMPLES];
  __shared__ int bad;
  const int t = threadIdx.x, M = ar.M;
  if (t == 0) bad = 0;
  __syncthreads();
  if (t < M) {
    const float q = ar.quality[t];
    float R = q;
    if (ar.cost) {
      double C = 0.0;                                       // the price and the reward in double, R_i rounded once: A_i = R_i - b
      for (int r = 0; r < rows; ++r) C += (double)ar.cost[(size_t)r * width + ch.a[t * rows + r]];      // cancels, and M values cost nothing
      if (C > 0.0) {
        const double ratio = C / (double)ar.ref, w = (double)ar.weight;
        R = (float)(ar.form == 0 ? (double)q * pow(ratio, w) : (double)q + w * log(ratio));
      }
    }
    sR[t] = R;
    if (!(fabsf(q) < INFINITY) || !(fabsf(R) < INFINITY)) bad = 1;      // (every writer stores the same value)
  }
  __syncthreads();
  if (bad) {
    if (t == 0) *ar.err = 1;
    return;
  }
  double sum_r = 0.0;
  for (int i = 0; i < M; ++i) sum_r += (double)sR[i];
  const double rbar = sum_r / (double)M;
  const float b_old = ar.baseline[0];
  const bool init = ar.baseline[1] != 0.f;
  const double b = init ? (double)b_old : rbar;
  double sum_a = 0.0;
  for (int i = 0; i < M; ++i) sum_a += (double)sR[i] - b;
  if (t < M) sA[t] = (double)sR[t] - b;
  __syncthreads();
  if (t == 0) {
    const float b_new = init ? (float)(ar.decay * (double)b_old + ar.omd * rbar) : (float)rbar;
    ar.baseline[0] = b_new;
    ar.baseline[1] = 1.f;
    if (ar.stats) {
      for (int i = 0; i < M; ++i) ar.stats[i] = sR[i];
      ar.stats[M] = (float)rbar;
      ar.stats[M + 1] = (float)b;
      ar.stats[M + 2] = b_new;
    }
  }
  for (int r = t; r < rows; r += 256)
    alpha_reinforce_row(prob, m, v, prob_grad, r, rows, width, M, sA, sum_a, ch, lr, b1, b2, omb1, omb2, eps, c1, c2s, wd);
}

}  // namespace mmnas

using namespace mmnas;

static int mix_grid(size_t n4) {
  const size_t b = (n4 + 255) / 256;
  return (int)(b < 1 ? 1 : (b > 2048 ? 2048 : b));
}

extern "C" size_t mmnas_mixed_sum_ws_floats(void) { return (size_t)2048 * MAXC; }

extern "C" int mmnas_mixed_sum_fwd(const float* const* outs_host, int n, const float* gate, float* out, size_t count,
                                   void* stream) {
  MMNAS_REQUIRE(outs_host && gate && out, MMNAS_E_ARG, "mmnas_mixed_sum_fwd: null pointer");
  MMNAS_REQUIRE(n >= 1 && n <= MAXC, MMNAS_E_SHAPE, "mmnas_mixed_sum_fwd: 1..%d candidates, got %d", MAXC, n);
  MMNAS_REQUIRE(count % 4 == 0, MMNAS_E_SHAPE, "mmnas_mixed_sum_fwd: element count must be a multiple of 4");
  MixArgs a;
  a.n = n;
  for (int j = 0; j < MAXC; ++j) {
    a.o[j] = j < n ? outs_host[j] : nullptr;
    MMNAS_REQUIRE(((uintptr_t)a.o[j] & 15) == 0, MMNAS_E_ARG, "mmnas_mixed_sum_fwd: candidate %d unaligned", j);
  }
  if (count == 0) return MMNAS_OK;
  ProfScope ps(MMNAS_K_ROWOPS, 2.0 * n * count, 4.0 * (n + 1) * count, (hipStream_t)stream, "mixed_sum_fwd");
  MMNAS_LAUNCH(mixed_sum_fwd_kernel, dim3(mix_grid(count / 4)), dim3(256), 0, (hipStream_t)stream, a, gate, out, count / 4);
  return check_launch("mixed_sum_fwd");
}

extern "C" int mmnas_mixed_sum_bwd(const float* const* outs_host, int n, const float* gate, const float* dout,
                                   float* d_active, int active, float* dgate, float* ws, size_t count, void* stream) {
  MMNAS_REQUIRE(outs_host && gate && dout && dgate && ws, MMNAS_E_ARG, "mmnas_mixed_sum_bwd: null pointer");
  MMNAS_REQUIRE(n >= 1 && n <= MAXC, MMNAS_E_SHAPE, "mmnas_mixed_sum_bwd: 1..%d candidates, got %d", MAXC, n);
  MMNAS_REQUIRE(count % 4 == 0, MMNAS_E_SHAPE, "mmnas_mixed_sum_bwd: element count must be a multiple of 4");
  MMNAS_REQUIRE(!d_active || (active >= 0 && active < n), MMNAS_E_ARG, "mmnas_mixed_sum_bwd: active index out of range");
  MixArgs a;
  a.n = n;
  for (int j = 0; j < MAXC; ++j) a.o[j] = j < n ? outs_host[j] : nullptr;
  if (count == 0) return MMNAS_OK;
  const int g = mix_grid(count / 4);
  ProfScope ps(MMNAS_K_ROWOPS, 2.0 * n * count, 4.0 * (n + 2) * count, (hipStream_t)stream, "mixed_sum_bwd");
  MMNAS_LAUNCH(mixed_sum_bwd_kernel, dim3(g), dim3(256), 0, (hipStream_t)stream, a, gate, dout, d_active, active, ws, count / 4);
  MMNAS_LAUNCH(mixed_sum_reduce_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const float*)ws, g, n, dgate);
  return check_launch("mixed_sum_bwd");
}

extern "C" int mmnas_alpha_full_step_wd(float* prob, const float* gate_grad, float* m, float* v, float* prob_grad, int rows,
                                        int width, float lr, float beta1, float beta2, float eps, float weight_decay, int step,
                                        void* stream) {
  MMNAS_REQUIRE(prob && gate_grad && m && v && step >= 1 && rows >= 0 && width >= 1, MMNAS_E_ARG, "mmnas_alpha_full_step / mmnas_alpha_full_step_wd: bad arguments");
  if (rows == 0) return MMNAS_OK;
  const AdamCoef k = adam_coef(beta1, beta2, step);
  MMNAS_LAUNCH(alpha_full_step_kernel, dim3(cdiv(rows, 64)), dim3(64), 0, (hipStream_t)stream, prob, gate_grad, m, v, prob_grad,
               rows, width, lr, beta1, beta2, k.omb1, k.omb2, eps, k.c1, k.c2s, weight_decay);
  return check_launch("alpha_full_step");
}

extern "C" int mmnas_alpha_full_step(float* prob, const float* gate_grad, float* m, float* v, float* prob_grad, int rows,
                                     int width, float lr, float beta1, float beta2, float eps, int step, void* stream) {
  return mmnas_alpha_full_step_wd(prob, gate_grad, m, v, prob_grad, rows, width, lr, beta1, beta2, eps, 0.f, step, stream);
}

extern "C" int mmnas_alpha_two_step(float* prob, const float* gate_grad, float* m, float* v, float* prob_grad, int rows,
                                    int width, const int* pair_host, float lr, float beta1, float beta2, float eps,
                                    float weight_decay, int step, void* stream) {
  MMNAS_REQUIRE(rows >= 0 && rows <= ALPHA_TWO_MAX_ROWS, MMNAS_E_SHAPE, "mmnas_alpha_two_step: rows=%d (0..%d)", rows, ALPHA_TWO_MAX_ROWS);
  MMNAS_REQUIRE(step >= 1 && width >= 2, MMNAS_E_ARG, "mmnas_alpha_two_step: step=%d (>= 1) width=%d (>= 2)", step, width);
  if (rows == 0) return MMNAS_OK;
  MMNAS_REQUIRE(prob && gate_grad && m && v && pair_host, MMNAS_E_ARG, "mmnas_alpha_two_step: null pointer");
  AlphaPairArgs pa;
  memset(&pa, 0, sizeof(pa));
  for (int r = 0; r < rows; ++r) {
    const int i = pair_host[2 * r], j = pair_host[2 * r + 1];
    MMNAS_REQUIRE(i >= 0 && i < width && j >= 0 && j < width && i != j, MMNAS_E_ARG,
                  "mmnas_alpha_two_step: row %d: pair (%d, %d) must be two different columns of 0..%d", r, i, j, width - 1);
    pa.ij[2 * r] = i;
    pa.ij[2 * r + 1] = j;
  }
  const AdamCoef k = adam_coef(beta1, beta2, step);
  MMNAS_LAUNCH(alpha_two_step_kernel, dim3(cdiv(rows, 64)), dim3(64), 0, (hipStream_t)stream, prob, gate_grad, m, v, prob_grad,
               rows, width, lr, beta1, beta2, k.omb1, k.omb2, eps, k.c1, k.c2s, weight_decay, pa);
  return check_launch("alpha_two_step");
}

// The cost entries: what both check before anything else (the coefficients: adam_coef, as every Adam entry).
static int alpha_cost_args(const char* who, const float* prob, const float* gate_grad, const float* m, const float* v,
                           const float* cost, int width, int min_width, float cost_weight, float cost_ref, int cost_form, int step) {
  MMNAS_REQUIRE(step >= 1 && width >= min_width, MMNAS_E_ARG, "%s: step=%d (>= 1) width=%d (>= %d)", who, step, width, min_width);
  MMNAS_REQUIRE(cost_form == 0 || cost_form == 1, MMNAS_E_ARG, "%s: cost_form=%d (0 linear, 1 log)", who, cost_form);
  MMNAS_REQUIRE(std::isfinite(cost_ref) && cost_ref > 0.f, MMNAS_E_ARG, "%s: cost_ref=%g must be finite and positive", who, (double)cost_ref);
  MMNAS_REQUIRE(std::isfinite(cost_weight) && cost_weight >= 0.f, MMNAS_E_ARG, "%s: cost_weight=%g must be finite and not negative", who,
                (double)cost_weight);
  MMNAS_REQUIRE(prob && gate_grad && m && v && cost, MMNAS_E_ARG, "%s: null pointer", who);
  return MMNAS_OK;
}

extern "C" int mmnas_alpha_full_step_cost(float* prob, const float* gate_grad, float* m, float* v, float* prob_grad,
                                          const float* cost, float* stats, int rows, int width, float lr, float beta1, float beta2,
                                          float eps, float weight_decay, float cost_weight, float cost_ref, int cost_form, int step,
                                          void* stream) {
  MMNAS_REQUIRE(rows >= 0, MMNAS_E_ARG, "mmnas_alpha_full_step_cost: rows=%d", rows);
  const int rc = alpha_cost_args("mmnas_alpha_full_step_cost", prob, gate_grad, m, v, cost, width, 1, cost_weight, cost_ref, cost_form, step);
  if (rc != MMNAS_OK) return rc;
  const AdamCoef k = adam_coef(beta1, beta2, step);
  const AlphaCost ac{cost, stats, cost_weight, cost_ref, cost_form};
  MMNAS_LAUNCH(alpha_full_step_cost_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, prob, gate_grad, m, v, prob_grad, rows, width,
               lr, beta1, beta2, k.omb1, k.omb2, eps, k.c1, k.c2s, weight_decay, ac);
  return check_launch("alpha_full_step_cost");
}

extern "C" int mmnas_alpha_two_step_cost(float* prob, const float* gate_grad, float* m, float* v, float* prob_grad,
                                         const float* cost, float* stats, int rows, int width, const int* pair_host, float lr,
                                         float beta1, float beta2, float eps, float weight_decay, float cost_weight, float cost_ref,
                                         int cost_form, int step, void* stream) {
  MMNAS_REQUIRE(rows >= 0 && rows <= ALPHA_TWO_MAX_ROWS, MMNAS_E_SHAPE, "mmnas_alpha_two_step_cost: rows=%d (0..%d)", rows, ALPHA_TWO_MAX_ROWS);
  const int rc = alpha_cost_args("mmnas_alpha_two_step_cost", prob, gate_grad, m, v, cost, width, 2, cost_weight, cost_ref, cost_form, step);
  if (rc != MMNAS_OK) return rc;
  MMNAS_REQUIRE(pair_host, MMNAS_E_ARG, "mmnas_alpha_two_step_cost: null pointer");
  AlphaPairArgs pa;
  memset(&pa, 0, sizeof(pa));
  for (int r = 0; r < rows; ++r) {
    const int i = pair_host[2 * r], j = pair_host[2 * r + 1];
    MMNAS_REQUIRE(i >= 0 && i < width && j >= 0 && j < width && i != j, MMNAS_E_ARG,
                  "mmnas_alpha_two_step_cost: row %d: pair (%d, %d) must be two different columns of 0..%d", r, i, j, width - 1);
    pa.ij[2 * r] = i;
    pa.ij[2 * r + 1] = j;
  }
  const AdamCoef k = adam_coef(beta1, beta2, step);
  const AlphaCost ac{cost, stats, cost_weight, cost_ref, cost_form};
  MMNAS_LAUNCH(alpha_two_step_cost_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, prob, gate_grad, m, v, prob_grad, rows, width,
               lr, beta1, beta2, k.omb1, k.omb2, eps, k.c1, k.c2s, weight_decay, pa, ac);
  return check_launch("alpha_two_step_cost");
}

extern "C" int mmnas_alpha_reinforce_step(float* prob, float* m, float* v, float* prob_grad, int rows, int width,
                                          const unsigned char* choice_host, const int* n_choices_host, int M, const float* quality,
                                          const float* cost, float cost_weight, float cost_ref, int reward_form, float* baseline,
                                          float baseline_decay, float* stats, int* err, float lr, float beta1, float beta2,
                                          float eps, float weight_decay, int step, void* stream) {
  const char* who = "mmnas_alpha_reinforce_step";
  MMNAS_REQUIRE(rows >= 0 && M >= 1 && step >= 1 && width >= 1, MMNAS_E_ARG, "%s: rows=%d (>= 0) M=%d (>= 1) step=%d (>= 1) width=%d (>= 1)",
                who, rows, M, step, width);
  MMNAS_REQUIRE(reward_form == 0 || reward_form == 1, MMNAS_E_ARG, "%s: reward_form=%d (0 mul, 1 add)", who, reward_form);
  MMNAS_REQUIRE(std::isfinite(cost_ref) && cost_ref > 0.f, MMNAS_E_ARG, "%s: cost_ref=%g must be finite and positive", who, (double)cost_ref);
  MMNAS_REQUIRE(std::isfinite(cost_weight), MMNAS_E_ARG, "%s: cost_weight=%g must be finite", who, (double)cost_weight);
  MMNAS_REQUIRE(baseline_decay >= 0.f && baseline_decay < 1.f, MMNAS_E_ARG, "%s: baseline_decay=%g outside [0, 1)", who, (double)baseline_decay);
  MMNAS_REQUIRE(prob && m && v && choice_host && n_choices_host && quality && baseline && err, MMNAS_E_ARG, "%s: null pointer", who);
  MMNAS_REQUIRE(M <= ALPHA_REINFORCE_MAX_SAMPLES && width <= 256 && (long)M * rows <= ALPHA_REINFORCE_MAX_CHOICES, MMNAS_E_SHAPE,
                "%s: M=%d (<= %d) width=%d (<= 256) M * rows=%ld (<= %d: the indices travel in the kernel arguments)", who, M,
                ALPHA_REINFORCE_MAX_SAMPLES, width, (long)M * rows, ALPHA_REINFORCE_MAX_CHOICES);
  for (int r = 0; r < rows; ++r)
    MMNAS_REQUIRE(n_choices_host[r] >= 1 && n_choices_host[r] <= width, MMNAS_E_ARG, "%s: row %d has %d live columns of %d", who, r,
                  n_choices_host[r], width);
  AlphaChoiceArgs ch;
  memset(&ch, 0, sizeof(ch));
  for (int i = 0; i < M; ++i)
    for (int r = 0; r < rows; ++r) {
      const int a = choice_host[(size_t)i * rows + r];
      MMNAS_REQUIRE(a < n_choices_host[r], MMNAS_E_ARG, "%s: sample %d, row %d: candidate %d outside 0..%d", who, i, r, a,
                    n_choices_host[r] - 1);
      ch.a[i * rows + r] = (unsigned char)a;
    }
  const AdamCoef k = adam_coef(beta1, beta2, step);
  const double decay = decimal_of(baseline_decay);
  AlphaReinforce ar;
  ar.quality = quality;
  ar.cost = cost_weight != 0.f ? cost : nullptr;
  ar.baseline = baseline; ar.stats = stats; ar.err = err;
  ar.decay = decay; ar.omd = 1.0 - decay;
  ar.weight = cost_weight; ar.ref = cost_ref; ar.form = reward_form; ar.M = M;
  MMNAS_LAUNCH(alpha_reinforce_step_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, prob, m, v, prob_grad, rows, width, lr, beta1,
               beta2, k.omb1, k.omb2, eps, k.c1, k.c2s, weight_decay, ar, ch);
  return check_launch("alpha_reinforce_step");
}


namespace mmnas {
static int node_args(NodeMixArgs& a, const float* const* z, const float* const* ln_a, const float* const* ln_b, int n, int d, const char* who) {
  MMNAS_REQUIRE(z && n >= 1 && n <= MAXC, MMNAS_E_SHAPE, "%s: 1..%d candidates, got %d", who, MAXC, n);
  MMNAS_REQUIRE(d >= 4 && d % 4 == 0 && d <= 1024, MMNAS_E_SHAPE, "%s: d=%d (multiple of 4, <= 1024)", who, d);
  memset(&a, 0, sizeof(a));
  a.n = n;
  for (int j = 0; j < n; ++j) {
    a.z[j] = z[j];
    a.a[j] = ln_a ? ln_a[j] : nullptr;
    a.b[j] = ln_b ? ln_b[j] : nullptr;
    MMNAS_REQUIRE(((uintptr_t)a.z[j] & 15) == 0, MMNAS_E_ARG, "%s: candidate %d: unaligned input", who, j);   // (NULL: not evaluated)
    MMNAS_REQUIRE(!a.a[j] || (a.b[j] && (((uintptr_t)a.a[j] | (uintptr_t)a.b[j]) & 15) == 0), MMNAS_E_ARG, "%s: candidate %d: LayerNorm parameters", who, j);
    if (d < 2) MMNAS_REQUIRE(!a.a[j], MMNAS_E_SHAPE, "%s: LayerNorm needs d >= 2", who);
  }
  return MMNAS_OK;
}
}  // namespace mmnas

extern "C" int mmnas_node_mix_fwd(const float* const* z, const float* const* ln_a, const float* const* ln_b, int n, const float* gate,
                                  float* out, int M, int d, float eps, void* stream) {
  NodeMixArgs a;
  int rc = node_args(a, z, ln_a, ln_b, n, d, "mmnas_node_mix_fwd");
  if (rc) return rc;
  MMNAS_REQUIRE(gate && out && M >= 0, MMNAS_E_ARG, "mmnas_node_mix_fwd: null pointer");
  if (M == 0) return MMNAS_OK;
  hipStream_t st = (hipStream_t)stream;
  ProfScope ps(MMNAS_K_ROWOPS, (2.0 * n + 8.0 * n) * M * d, 4.0 * (n + 1) * M * d, st, "node_mix_fwd");
  const dim3 grid(cdiv(M, 4)), block(256);
  if (d <= 256) MMNAS_LAUNCH((node_mix_fwd_kernel<1>), grid, block, 0, st, a, gate, out, M, d, eps);
  else if (d <= 512) MMNAS_LAUNCH((node_mix_fwd_kernel<2>), grid, block, 0, st, a, gate, out, M, d, eps);
  else MMNAS_LAUNCH((node_mix_fwd_kernel<4>), grid, block, 0, st, a, gate, out, M, d, eps);
  return check_launch("node_mix_fwd");
}

namespace mmnas {
// reduce == false: the partial sums stay in ws[0 .. *nwg_out * MAXC) for mixed_reduce_many()
int mixed_reduce_many(const float* const* parts, float* const* dgates, const int* nwg, const int* n, int count, hipStream_t st) {
  for (int i0 = 0; i0 < count; i0 += MMNAS_MIX_REDUCE_MAX) {
    MixReduceJobs jobs;
    const int c = count - i0 < MMNAS_MIX_REDUCE_MAX ? count - i0 : MMNAS_MIX_REDUCE_MAX;
    for (int i = 0; i < c; ++i) { jobs.part[i] = parts[i0 + i]; jobs.dgate[i] = dgates[i0 + i]; jobs.nwg[i] = nwg[i0 + i]; jobs.n[i] = n[i0 + i]; }
    ProfScope ps(MMNAS_K_ROWOPS, 0.0, 0.0, st, "mixed_reduce_many");
    MMNAS_LAUNCH(mixed_sum_reduce_many_kernel, dim3(c), dim3(256), 0, st, jobs);
  }
  return check_launch("mixed_reduce_many");
}
}  // namespace mmnas

extern "C" int mmnas_node_mix_bwd(const float* const* z, const float* const* ln_a, const float* const* ln_b, int n, const float* gate,
                                  const float* dout, float* d_active, int active, float* dgate, float* ws, int M, int d, float eps,
                                  void* stream) {
  return mmnas::node_mix_bwd_impl(z, ln_a, ln_b, n, gate, dout, d_active, active, dgate, ws, M, d, eps, (hipStream_t)stream, true, nullptr);
}

// mmnas_node_mix_bwd with the sampled candidate's LayerNorm backward inside the same launch, as the mixed chain runs it
// (ops.hip: chain backward): dz / dt / the LayerNorm parameter gradients instead of d_active.
extern "C" int mmnas_node_mix_bwd_ln(const float* const* z, const float* const* ln_a, const float* const* ln_b, int n, const float* gate,
                                     const float* dout, int active, float* dgate, float* ws, float* dz, float* dt, float* dln_a,
                                     float* dln_b, float* dcol, float* lnws, float drop_p, uint64_t seed, uint32_t site, int M, int d,
                                     float eps, void* stream) {
  MMNAS_REQUIRE(dz && lnws && ln_a && ln_b, MMNAS_E_ARG, "mmnas_node_mix_bwd_ln: null pointer");
  MMNAS_REQUIRE(dcol == nullptr || dt != nullptr, MMNAS_E_ARG, "mmnas_node_mix_bwd_ln: dcol needs dt");
  mmnas::NodeLnBwd lnb;
  lnb.dz = dz; lnb.dt = dt; lnb.part = lnws;
  lnb.drop = mmnas::make_drop(dt ? drop_p : 0.f, seed, site);
  int nwg = 0;
  const int rc = mmnas::node_mix_bwd_impl(z, ln_a, ln_b, n, gate, dout, nullptr, active, dgate, ws, M, d, eps, (hipStream_t)stream, true, &nwg, &lnb);
  if (rc || nwg == 0) return rc;
  mmnas::AuxReduce aux;
  aux.part = lnws; aux.nrows = nwg; aux.d = d;
  aux.out[0] = dln_a; aux.out[1] = dln_b; aux.out[2] = dcol;
  return mmnas::launch_aux_reduce(aux, (hipStream_t)stream);
}

int mmnas::node_mix_bwd_impl(const float* const* z, const float* const* ln_a, const float* const* ln_b, int n, const float* gate,
                             const float* dout, float* d_active, int active, float* dgate, float* ws, int M, int d, float eps,
                             hipStream_t stream, bool reduce, int* nwg_out, const NodeLnBwd* lnb) {
  NodeMixArgs a;
  int rc = node_args(a, z, ln_a, ln_b, n, d, "mmnas_node_mix_bwd");
  if (rc) return rc;
  MMNAS_REQUIRE(gate && dout && dgate && ws && M >= 0, MMNAS_E_ARG, "mmnas_node_mix_bwd: null pointer");
  MMNAS_REQUIRE(!d_active || (active >= 0 && active < n), MMNAS_E_ARG, "mmnas_node_mix_bwd: active index out of range");
  if (nwg_out) *nwg_out = 0;
  if (M == 0) return MMNAS_OK;
  hipStream_t st = stream;
  const bool fuse = lnb && lnb->dz;
  if (fuse) MMNAS_REQUIRE(active >= 0 && active < n && z[active] && ln_a[active] && ln_b[active] && lnb->part && d <= 256, MMNAS_E_ARG,
                          "mmnas_node_mix_bwd: the fused LayerNorm backward needs a normalised active candidate (d <= 256)");
  int g = cdiv(M, 4);
  if (g > 2048) g = 2048;
  if (fuse && g > 512) g = 512;      // ln_bwd_kernel's row -> workgroup map: the partial rows fit mmnas_layernorm_bwd_ws_floats
  if (nwg_out) *nwg_out = g;
  ProfScope ps(MMNAS_K_ROWOPS, (2.0 * n + 8.0 * n) * M * d + (fuse ? 16.0 * M * d : 0.0), 4.0 * (n + 2 + (fuse ? 1 : 0)) * M * d, st, "node_mix_bwd");
  const dim3 grid(g), block(256);
  float* const ndz = fuse ? lnb->dz : nullptr; float* const ndt = fuse ? lnb->dt : nullptr; float* const npart = fuse ? lnb->part : nullptr;
  const DropCfg ndrop = fuse ? lnb->drop : make_drop(0.f, 0, 0);
  // (d <= 256 only: the two-chunk instantiation <2, true> crashes this compiler's machine copy propagation, as a [2][NV] row
  //  array did in rowops.hip; the supernet -- the one user of mixed chains -- is 256 wide)
  if (fuse) MMNAS_LAUNCH((node_mix_bwd_kernel<1, true>), grid, block, 0, st, a, gate, dout, d_active, active, ws, M, d, eps, ndz, ndt, npart, ndrop);
  else if (d <= 256) MMNAS_LAUNCH((node_mix_bwd_kernel<1, false>), grid, block, 0, st, a, gate, dout, d_active, active, ws, M, d, eps, ndz, ndt, npart, ndrop);
  else if (d <= 512) MMNAS_LAUNCH((node_mix_bwd_kernel<2, false>), grid, block, 0, st, a, gate, dout, d_active, active, ws, M, d, eps, ndz, ndt, npart, ndrop);
  else MMNAS_LAUNCH((node_mix_bwd_kernel<4, false>), grid, block, 0, st, a, gate, dout, d_active, active, ws, M, d, eps, ndz, ndt, npart, ndrop);
  if (reduce) MMNAS_LAUNCH(mixed_sum_reduce_kernel, dim3(1), dim3(256), 0, st, (const float*)ws, g, n, dgate);
  return check_launch("node_mix_bwd");
}
