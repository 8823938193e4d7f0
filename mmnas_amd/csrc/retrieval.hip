// Retrieval scoring of the ITM network outside the training step (train_itm.py:437-546 evaluation, :299-363 hard-negative
// mining; mmnas_amd/retrieval.py drives these):
//   * mmnas_mha_core_fwd_indexed -- the guided operators' attention cores over a per-caption K / V cache (kernel in
//     attention.hip: a compile-time variant of the <= 64-key forward body);
//   * mmnas_itm_pair_head        -- z = LN(xflat[cap_idx[p]] + yflat[p]); logit = z . Wp + bp; score = sigmoid(logit)
//     (full_itm.py:109-112), one wave per pair, the score written straight into the score matrix when asked;
//   * mmnas_rank_matrix          -- the i2t / t2i ranks of train_itm.py:505-546 as counts of strictly greater scores;
//   * mmnas_row_topk             -- the per-anchor argsort of train_itm.py:317-318 (ties: lower position first).
#include "common.h"

namespace mmnas {

// ------------------------------------------------------------------------------------------
// pair head: block 256 = 4 waves = 4 pairs; lane holds columns lane + 64 i
// ------------------------------------------------------------------------------------------
constexpr int HEAD_MAXD = 2048;
constexpr int HEAD_PER_LANE = HEAD_MAXD / 64;

__global__ void __launch_bounds__(256) itm_pair_head_kernel(const float* __restrict__ xflat, const int* __restrict__ cap_idx,
                                                            const float* __restrict__ yflat, const float* __restrict__ ln_a,
                                                            const float* __restrict__ ln_b, const float* __restrict__ Wp,
                                                            const float* __restrict__ bp, float* __restrict__ logits,
                                                            float* __restrict__ scores, const int* __restrict__ img_row,
                                                            const int* __restrict__ cap_col, long ld, int P, int D, float eps) {
  const int lane = threadIdx.x & 63;
  const int p = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (p >= P) return;   // wave-uniform
  const float* xr = xflat + (size_t)cap_idx[p] * D;
  const float* yr = yflat + (size_t)p * D;
  float z[HEAD_PER_LANE];
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < HEAD_PER_LANE; ++i) {
    const int j = lane + 64 * i;
    z[i] = j < D ? xr[j] + yr[j] : 0.f;
    s += z[i];
  }
  const float mean = wave_sum(s) / (float)D;
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < HEAD_PER_LANE; ++i) {
    const int j = lane + 64 * i;
    const float c = j < D ? z[i] - mean : 0.f;
    z[i] = c;
    q += c * c;
  }
  // LayerNorm of modules.py:44-56: Bessel-corrected std, eps added to the std
  const float inv = 1.0f / (sqrtf(wave_sum(q) / (float)(D - 1)) + eps);
  float dot = 0.f;
#pragma unroll
  for (int i = 0; i < HEAD_PER_LANE; ++i) {
    const int j = lane + 64 * i;
    if (j < D) dot += (ln_a[j] * (z[i] * inv) + ln_b[j]) * Wp[j];
  }
  const float logit = wave_sum(dot) + bp[0];
  if (lane == 0) {
    if (logits) logits[p] = logit;
    if (scores) {
      const float sc = 1.0f / (1.0f + expf(-logit));
      if (img_row) scores[(size_t)img_row[p] * ld + cap_col[p]] = sc;
      else scores[p] = sc;
    }
  }
}

// ------------------------------------------------------------------------------------------
// ranks.  i2t (row pass): one workgroup per image row, coalesced over the row.  t2i (column pass): a thread per caption column,
// a workgroup per (256 columns, 64 rows): consecutive threads read consecutive columns of a row; the row chunks add their
// counts with integer atomics (exact, order-free) into the zeroed outputs.
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) rank_rows_kernel(const float* __restrict__ S, int Nc, long ld, int G, int* __restrict__ rank,
                                                        int* __restrict__ tie, int* __restrict__ nan_flag) {
  __shared__ int cnt[3];
  const int i = blockIdx.x, tid = threadIdx.x;
  if (tid < 3) cnt[tid] = 0;
  __syncthreads();
  const float* row = S + (size_t)i * ld;
  float t = row[(size_t)G * i];
  for (int g = 1; g < G; ++g) t = fmaxf(t, row[(size_t)G * i + g]);
  int gt = 0, eq = 0, nan = 0;
  for (int k = tid; k < Nc; k += 256) {
    const float v = row[k];
    gt += v > t;
    eq += (v == t) && (k < G * i || k >= G * (i + 1));
    nan |= v != v;
  }
  if (gt) atomicAdd(&cnt[0], gt);
  if (eq) atomicAdd(&cnt[1], eq);
  if (nan) atomicOr(&cnt[2], 1);
  __syncthreads();
  if (tid == 0) {
    rank[i] = cnt[0];
    tie[i] = cnt[1];
    if (cnt[2] || t != t) atomicOr(nan_flag, 1);
  }
}

constexpr int RANK_COL_ROWS = 64;

__global__ void __launch_bounds__(256) rank_cols_kernel(const float* __restrict__ S, int Ni, int Nc, long ld, int G,
                                                        int* __restrict__ rank, int* __restrict__ tie) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= Nc) return;
  const int own = j / G;
  const float t = S[(size_t)own * ld + j];
  const int r0 = blockIdx.y * RANK_COL_ROWS, r1 = min(Ni, r0 + RANK_COL_ROWS);
  int gt = 0, eq = 0;
#pragma unroll 8
  for (int i = r0; i < r1; ++i) {
    const float v = S[(size_t)i * ld + j];
    gt += v > t;
    eq += (v == t) && i != own;
  }
  if (gt) atomicAdd(rank + j, gt);
  if (eq) atomicAdd(tie + j, eq);
}

// ------------------------------------------------------------------------------------------
// row top-k: one wave per row, the row in LDS; element c goes to slot #{c' : s[c'] > s[c] or (s[c'] == s[c] and c' < c)}
// (every lane reads the same LDS word in a step: a broadcast)
// ------------------------------------------------------------------------------------------
constexpr int TOPK_MAXC = 1024;

__global__ void __launch_bounds__(256) row_topk_kernel(const float* __restrict__ S, int N, int C, long ld, int k, int* __restrict__ out,
                                                       int* __restrict__ nan_flag) {
  __shared__ float rows[4][TOPK_MAXC];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int r = blockIdx.x * 4 + w;
  if (r >= N) return;   // wave-uniform; no workgroup barrier below
  float* row = rows[w];
  int nan = 0;
  for (int c = lane; c < C; c += 64) {
    const float v = S[(size_t)r * ld + c];
    row[c] = v;
    nan |= v != v;
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  if (nan && nan_flag) atomicOr(nan_flag, 1);
  for (int c = lane; c < C; c += 64) {
    const float v = row[c];
    int pos = 0;
    for (int c2 = 0; c2 < C; ++c2) {
      const float u = row[c2];
      pos += (u > v) || (u == v && c2 < c);
    }
    if (pos < k) out[(size_t)r * k + pos] = c;
  }
}

}  // namespace mmnas

using namespace mmnas;

extern "C" int mmnas_mha_core_fwd_indexed(const mmnas_mha_desc* d, const int* kv_idx, void* stream) {
  return mha_core_fwd_indexed(d, kv_idx, (hipStream_t)stream);
}

extern "C" int mmnas_itm_pair_head(const float* xflat, const int* cap_idx, const float* yflat, const float* ln_a, const float* ln_b,
                                   const float* Wp, const float* bp, float* logits, float* scores, const int* img_row,
                                   const int* cap_col, long ld, int P, int D, float eps, void* stream) {
  MMNAS_REQUIRE(P >= 0 && D >= 2 && D <= HEAD_MAXD, MMNAS_E_SHAPE, "itm_pair_head: P=%d D=%d (2 <= D <= %d)", P, D, HEAD_MAXD);
  MMNAS_REQUIRE(xflat && cap_idx && yflat && ln_a && ln_b && Wp && bp, MMNAS_E_ARG, "itm_pair_head: null input");
  MMNAS_REQUIRE(logits || scores, MMNAS_E_ARG, "itm_pair_head: neither logits nor scores requested");
  MMNAS_REQUIRE(!img_row == !cap_col, MMNAS_E_ARG, "itm_pair_head: img_row and cap_col go together");
  MMNAS_REQUIRE(!img_row || (scores && ld > 0), MMNAS_E_ARG, "itm_pair_head: matrix placement needs scores and ld > 0");
  if (P == 0) return MMNAS_OK;
  hipStream_t st = (hipStream_t)stream;
  MMNAS_LAUNCH(itm_pair_head_kernel, dim3(cdiv(P, 4)), dim3(256), 0, st, xflat, cap_idx, yflat, ln_a, ln_b, Wp, bp, logits, scores,
               img_row, cap_col, ld, P, D, eps);
  return check_launch("itm_pair_head");
}

extern "C" int mmnas_rank_matrix(const float* S, int Ni, int Nc, long ld, int* i2t_rank, int* i2t_tie, int* t2i_rank, int* t2i_tie,
                                 int* nan_flag, void* stream) {
  MMNAS_REQUIRE(Ni > 0 && Nc > 0 && Nc % Ni == 0, MMNAS_E_SHAPE, "rank_matrix: Nc=%d must be a positive multiple of Ni=%d", Nc, Ni);
  MMNAS_REQUIRE(ld >= Nc, MMNAS_E_SHAPE, "rank_matrix: ld=%ld < Nc=%d", ld, Nc);
  MMNAS_REQUIRE(S && i2t_rank && i2t_tie && t2i_rank && t2i_tie && nan_flag, MMNAS_E_ARG, "rank_matrix: null pointer");
  hipStream_t st = (hipStream_t)stream;
  const int G = Nc / Ni;
  if (hipMemsetAsync(t2i_rank, 0, sizeof(int) * (size_t)Nc, st) != hipSuccess ||
      hipMemsetAsync(t2i_tie, 0, sizeof(int) * (size_t)Nc, st) != hipSuccess ||
      hipMemsetAsync(nan_flag, 0, sizeof(int), st) != hipSuccess)
    return check_launch("rank_matrix (memset)");
  MMNAS_LAUNCH(rank_rows_kernel, dim3(Ni), dim3(256), 0, st, S, Nc, ld, G, i2t_rank, i2t_tie, nan_flag);
  MMNAS_LAUNCH(rank_cols_kernel, dim3(cdiv(Nc, 256), cdiv(Ni, RANK_COL_ROWS)), dim3(256), 0, st, S, Ni, Nc, ld, G, t2i_rank, t2i_tie);
  return check_launch("rank_matrix");
}

extern "C" int mmnas_row_topk(const float* S, int N, int C, long ld, int k, int* out, int* nan_flag, void* stream) {
  MMNAS_REQUIRE(N >= 0 && C > 0 && C <= TOPK_MAXC, MMNAS_E_SHAPE, "row_topk: C=%d candidates (1 <= C <= %d)", C, TOPK_MAXC);
  MMNAS_REQUIRE(k > 0 && k <= C, MMNAS_E_SHAPE, "row_topk: k=%d outside 1..C=%d", k, C);
  MMNAS_REQUIRE(ld >= C, MMNAS_E_SHAPE, "row_topk: ld=%ld < C=%d", ld, C);
  MMNAS_REQUIRE(S && out, MMNAS_E_ARG, "row_topk: null pointer");
  hipStream_t st = (hipStream_t)stream;
  if (nan_flag && hipMemsetAsync(nan_flag, 0, sizeof(int), st) != hipSuccess) return check_launch("row_topk (memset)");
  if (N == 0) return MMNAS_OK;
  MMNAS_LAUNCH(row_topk_kernel, dim3(cdiv(N, 4)), dim3(256), 0, st, S, N, C, ld, k, out, nan_flag);
  return check_launch("row_topk");
}
