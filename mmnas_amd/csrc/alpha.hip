// The architecture-parameter updates of the search, every node (row of the [rows, width] alpha block) in one launch:
//   * 'full' mode: dL/dalpha from dL/dgate (mixed.py:171-198) followed by the Adam step of alpha_optim (search_vqa.py:194,331-332);
//   * 'two' mode: the gradient over the sampled pair, the same Adam step and the pair's rescale (mixed.py:179-208,
//     search_vqa.py:330-335);
//   * both with the expected-cost term of a hardware-aware search, and the REINFORCE update over sampled architectures.
// What the rows share -- the softmax statistics, the expected cost, the Adam element update -- is written once below.
#include <math.h>
#include <string.h>
#include "common.h"

namespace mmnas {

// lr, the betas, eps and weight decay as the caller gave them; 1 - beta and the bias corrections from adam_coef
struct AlphaAdam { float lr, b1, b2, omb1, omb2, eps, c1, c2s, wd; };

// torch Adam on one element: moves the moments at o, returns the new alpha (grad: weight decay already added).  Every product
// is rounded before it is added (no fused multiply-add): the bits do not depend on which product the compiler would fuse.
__device__ __forceinline__ float alpha_adam_elem(float ai, float* __restrict__ m, float* __restrict__ v, size_t o, float grad,
                                                 const AlphaAdam& h) {
#pragma clang fp contract(off)
  const float mi = h.b1 * m[o] + h.omb1 * grad;             // omb = 1 - beta, formed on the host (adam_coef)
  const float vi = h.b2 * v[o] + h.omb2 * grad * grad;
  m[o] = mi; v[o] = vi;
  return ai - (h.lr / h.c1) * mi / (sqrtf(vi) / h.c2s + h.eps);
}

// softmax statistics of one row: p_i = expf(a[i] - mx) / den (padding columns hold -inf: exp = 0)
__device__ __forceinline__ void alpha_row_max_den(const float* __restrict__ a, int width, float& mx, float& den) {
  mx = -INFINITY;
  for (int i = 0; i < width; ++i) mx = fmaxf(mx, a[i]);
  den = 0.f;
  for (int i = 0; i < width; ++i) den += expf(a[i] - mx);
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

// E_r of one row from its softmax statistics; without them: from the row alone
__device__ __forceinline__ float alpha_row_expected_cost(const float* __restrict__ a, const float* __restrict__ c, int width, float mx,
                                                         float den) {
  float e = 0.f;
  for (int i = 0; i < width; ++i) e += (expf(a[i] - mx) / den) * c[i];
  return e;
}
__device__ __forceinline__ float alpha_row_expected_cost(const float* __restrict__ a, const float* __restrict__ c, int width) {
  float mx, den;
  alpha_row_max_den(a, width, mx, den);
  return alpha_row_expected_cost(a, c, width, mx, den);
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
                                               float* __restrict__ v, float* __restrict__ prob_grad, int r, int width,
                                               const AlphaAdam& h, const float* __restrict__ cost, float k) {
  float* a = prob + (size_t)r * width;
  const float* g = gate_grad + (size_t)r * width;
  float mx, den;
  alpha_row_max_den(a, width, mx, den);
  float dot = 0.f;
  for (int i = 0; i < width; ++i) dot += g[i] * (expf(a[i] - mx) / den);
  float er = 0.f;
  if (COST) er = alpha_row_expected_cost(a, cost + (size_t)r * width, width, mx, den);
  for (int i = 0; i < width; ++i) {
    const float p = expf(a[i] - mx) / den;
    float grad = p * (g[i] - dot);                          // sum_j g_j p_j (delta_ij - p_i), mixed.py:194-198
    if (COST) grad += k * p * (cost[(size_t)r * width + i] - er);
    if (prob_grad) prob_grad[(size_t)r * width + i] = grad;
    if (p == 0.f && !(a[i] > -INFINITY)) continue;          // padding column: stays -inf
    if (h.wd != 0.f) grad += h.wd * a[i];                   // torch Adam's weight_decay (ALPHA_WEIGHT_DECAY): p.grad itself stays as it is
    a[i] = alpha_adam_elem(a[i], m, v, (size_t)r * width + i, grad, h);
  }
}

// one thread per node (row): 'full'-mode architecture gradient + Adam
__global__ void alpha_full_step_kernel(float* __restrict__ prob, const float* __restrict__ gate_grad, float* __restrict__ m,
                                       float* __restrict__ v, float* __restrict__ prob_grad, int rows, int width, AlphaAdam h) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= rows) return;
  alpha_full_row<false>(prob, gate_grad, m, v, prob_grad, r, width, h, nullptr, 0.f);
}

// the same with the expected-cost term: ONE workgroup of 256 threads walks the rows (alpha_cost_scale says why)
__global__ __launch_bounds__(256) void alpha_full_step_cost_kernel(float* __restrict__ prob, const float* __restrict__ gate_grad,
                                                                   float* __restrict__ m, float* __restrict__ v,
                                                                   float* __restrict__ prob_grad, int rows, int width, AlphaAdam h,
                                                                   AlphaCost ac) {
  const float k = alpha_cost_scale(prob, rows, width, ac);
  for (int r = threadIdx.x; r < rows; r += 256) alpha_full_row<true>(prob, gate_grad, m, v, prob_grad, r, width, h, ac.cost, k);
}

// one thread per node (row): 'two'-mode architecture gradient over the sampled pair + Adam over the row + the pair's
// mass-preserving rescale (mixed.py:179-208, search_vqa.py:330-335).  The pairs travel in the kernel arguments.
constexpr int ALPHA_TWO_MAX_ROWS = 128;                    // mmnas_onehot_rows' limit: 1 KB of kernel arguments
struct AlphaPairArgs { int ij[ALPHA_TWO_MAX_ROWS * 2]; };   // (active, inactive) per row

// COST: k p_i (cost_i - E_r), p the softmax over the WHOLE row, joins the pair gradient on every live column (the regulariser
// reaches all paths, the binary-gate gradient the sampled two)
template <bool COST>
__device__ __forceinline__ void alpha_two_row(float* __restrict__ prob, const float* __restrict__ gate_grad, float* __restrict__ m,
                                              float* __restrict__ v, float* __restrict__ prob_grad, int r, int width,
                                              const AlphaAdam& h, int pi, int pj, const float* __restrict__ cost, float k) {
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
    alpha_row_max_den(a, width, rmx, rden);
    er = alpha_row_expected_cost(a, cost + (size_t)r * width, width, rmx, rden);
  }
  for (int i = 0; i < width; ++i) {
    float grad = i == pi ? gi : (i == pj ? gj : 0.f);
    const size_t o = (size_t)r * width + i;
    const float ai = a[i];
    if (COST) grad += k * (expf(ai - rmx) / rden) * (cost[o] - er);
    if (prob_grad) prob_grad[o] = grad;
    if (!(ai > -INFINITY)) continue;                        // padding column: stays -inf, its moments untouched
    if (h.wd != 0.f) grad += h.wd * ai;                     // torch Adam's weight_decay: p.grad itself stays as it is
    a[i] = alpha_adam_elem(ai, m, v, o, grad, h);
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
                                      float* __restrict__ v, float* __restrict__ prob_grad, int rows, int width, AlphaAdam h,
                                      AlphaPairArgs pa) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= rows) return;
  alpha_two_row<false>(prob, gate_grad, m, v, prob_grad, r, width, h, pa.ij[2 * r], pa.ij[2 * r + 1], nullptr,
                       0.f);                                // (checked on the host: 0 <= pi != pj < width)
}

// the same with the expected-cost term: one workgroup of 256 threads (rows <= ALPHA_TWO_MAX_ROWS: a single pass each)
__global__ __launch_bounds__(256) void alpha_two_step_cost_kernel(float* __restrict__ prob, const float* __restrict__ gate_grad,
                                                                  float* __restrict__ m, float* __restrict__ v,
                                                                  float* __restrict__ prob_grad, int rows, int width, AlphaAdam h,
                                                                  AlphaPairArgs pa, AlphaCost ac) {
  const float k = alpha_cost_scale(prob, rows, width, ac);
  for (int r = threadIdx.x; r < rows; r += 256)
    alpha_two_row<true>(prob, gate_grad, m, v, prob_grad, r, width, h, pa.ij[2 * r], pa.ij[2 * r + 1], ac.cost, k);
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
// which Adam's eps = 1e-8 still swallows; float sums would leave 1e-9 there and Adam would step by it).
__device__ __forceinline__ void alpha_reinforce_row(float* __restrict__ prob, float* __restrict__ m, float* __restrict__ v,
                                                    float* __restrict__ prob_grad, int r, int rows, int width, int M,
                                                    const double* sA, double sum_a, const AlphaChoiceArgs& ch, const AlphaAdam& h) {
  float* a = prob + (size_t)r * width;
  float mx, den;
  alpha_row_max_den(a, width, mx, den);
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
    if (h.wd != 0.f) grad += h.wd * ai;                     // torch Adam's weight_decay: prob_grad keeps the undecayed gradient
    a[i] = alpha_adam_elem(ai, m, v, o, grad, h);
  }
}

// ONE workgroup of 256 threads.  Thread i < M prices sample i (rows ascending, in double) and forms R_i; a non-finite Q_i or R_i ends the
// kernel with *err = 1 before anything is written.  Every thread then forms mean R, b and sum_i A_i in double, samples
// ascending (no atomics, no cross-lane sums: the same bits on every call), thread 0 moves the baseline, and the threads walk
// the rows r, r + 256, ...  The baseline is read by everyone before the barrier and written by thread 0 after it.
__global__ __launch_bounds__(256) void alpha_reinforce_step_kernel(float* __restrict__ prob, float* __restrict__ m,
                                                                   float* __restrict__ v, float* __restrict__ prob_grad, int rows,
                                                                   int width, AlphaAdam h, AlphaReinforce ar, AlphaChoiceArgs ch) {
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
  for (int r = t; r < rows; r += 256) alpha_reinforce_row(prob, m, v, prob_grad, r, rows, width, M, sA, sum_a, ch, h);
}

}  // namespace mmnas

using namespace mmnas;

static AlphaAdam alpha_adam(float lr, float beta1, float beta2, float eps, float weight_decay, int step) {
  const AdamCoef k = adam_coef(beta1, beta2, step);
  return AlphaAdam{lr, beta1, beta2, k.omb1, k.omb2, eps, k.c1, k.c2s, weight_decay};
}

// the 'two' entries: every pair is two different columns of the block
static int alpha_pair_args(const char* who, AlphaPairArgs& pa, const int* pair_host, int rows, int width) {
  memset(&pa, 0, sizeof(pa));
  for (int r = 0; r < rows; ++r) {
    const int i = pair_host[2 * r], j = pair_host[2 * r + 1];
    MMNAS_REQUIRE(i >= 0 && i < width && j >= 0 && j < width && i != j, MMNAS_E_ARG,
                  "%s: row %d: pair (%d, %d) must be two different columns of 0..%d", who, r, i, j, width - 1);
    pa.ij[2 * r] = i;
    pa.ij[2 * r + 1] = j;
  }
  return MMNAS_OK;
}

// The cost and REINFORCE entries: the scalars all three check before their pointers.  form_name / forms: what the entry calls
// its form and the two values; any_sign: REINFORCE's weight is an exponent or a factor of a log and may be negative.
static int alpha_cost_args(const char* who, int width, int min_width, int step, const char* form_name, const char* forms, int form,
                           float cost_ref, float cost_weight, bool any_sign) {
  MMNAS_REQUIRE(step >= 1 && width >= min_width, MMNAS_E_ARG, "%s: step=%d (>= 1) width=%d (>= %d)", who, step, width, min_width);
  MMNAS_REQUIRE(form == 0 || form == 1, MMNAS_E_ARG, "%s: %s=%d (%s)", who, form_name, form, forms);
  MMNAS_REQUIRE(std::isfinite(cost_ref) && cost_ref > 0.f, MMNAS_E_ARG, "%s: cost_ref=%g must be finite and positive", who, (double)cost_ref);
  MMNAS_REQUIRE(std::isfinite(cost_weight) && (any_sign || cost_weight >= 0.f), MMNAS_E_ARG, "%s: cost_weight=%g must be finite%s", who,
                (double)cost_weight, any_sign ? "" : " and not negative");
  return MMNAS_OK;
}

extern "C" int mmnas_alpha_full_step_wd(float* prob, const float* gate_grad, float* m, float* v, float* prob_grad, int rows,
                                        int width, float lr, float beta1, float beta2, float eps, float weight_decay, int step,
                                        void* stream) {
  MMNAS_REQUIRE(prob && gate_grad && m && v && step >= 1 && rows >= 0 && width >= 1, MMNAS_E_ARG, "mmnas_alpha_full_step / mmnas_alpha_full_step_wd: bad arguments");
  if (rows == 0) return MMNAS_OK;
  MMNAS_LAUNCH(alpha_full_step_kernel, dim3(cdiv(rows, 64)), dim3(64), 0, (hipStream_t)stream, prob, gate_grad, m, v, prob_grad,
               rows, width, alpha_adam(lr, beta1, beta2, eps, weight_decay, step));
  return check_launch("alpha_full_step");
}

extern "C" int mmnas_alpha_full_step(float* prob, const float* gate_grad, float* m, float* v, float* prob_grad, int rows,
                                     int width, float lr, float beta1, float beta2, float eps, int step, void* stream) {
  return mmnas_alpha_full_step_wd(prob, gate_grad, m, v, prob_grad, rows, width, lr, beta1, beta2, eps, 0.f, step, stream);
}

extern "C" int mmnas_alpha_two_step(float* prob, const float* gate_grad, float* m, float* v, float* prob_grad, int rows,
                                    int width, const int* pair_host, float lr, float beta1, float beta2, float eps,
                                    float weight_decay, int step, void* stream) {
  const char* who = "mmnas_alpha_two_step";
  MMNAS_REQUIRE(rows >= 0 && rows <= ALPHA_TWO_MAX_ROWS, MMNAS_E_SHAPE, "%s: rows=%d (0..%d)", who, rows, ALPHA_TWO_MAX_ROWS);
  MMNAS_REQUIRE(step >= 1 && width >= 2, MMNAS_E_ARG, "%s: step=%d (>= 1) width=%d (>= 2)", who, step, width);
  if (rows == 0) return MMNAS_OK;
  MMNAS_REQUIRE(prob && gate_grad && m && v && pair_host, MMNAS_E_ARG, "%s: null pointer", who);
  AlphaPairArgs pa;
  if (const int rc = alpha_pair_args(who, pa, pair_host, rows, width)) return rc;
  MMNAS_LAUNCH(alpha_two_step_kernel, dim3(cdiv(rows, 64)), dim3(64), 0, (hipStream_t)stream, prob, gate_grad, m, v, prob_grad,
               rows, width, alpha_adam(lr, beta1, beta2, eps, weight_decay, step), pa);
  return check_launch("alpha_two_step");
}

extern "C" int mmnas_alpha_full_step_cost(float* prob, const float* gate_grad, float* m, float* v, float* prob_grad,
                                          const float* cost, float* stats, int rows, int width, float lr, float beta1, float beta2,
                                          float eps, float weight_decay, float cost_weight, float cost_ref, int cost_form, int step,
                                          void* stream) {
  const char* who = "mmnas_alpha_full_step_cost";
  MMNAS_REQUIRE(rows >= 0, MMNAS_E_ARG, "%s: rows=%d", who, rows);
  if (const int rc = alpha_cost_args(who, width, 1, step, "cost_form", "0 linear, 1 log", cost_form, cost_ref, cost_weight, false)) return rc;
  MMNAS_REQUIRE(prob && gate_grad && m && v && cost, MMNAS_E_ARG, "%s: null pointer", who);
  const AlphaCost ac{cost, stats, cost_weight, cost_ref, cost_form};
  MMNAS_LAUNCH(alpha_full_step_cost_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, prob, gate_grad, m, v, prob_grad, rows, width,
               alpha_adam(lr, beta1, beta2, eps, weight_decay, step), ac);
  return check_launch("alpha_full_step_cost");
}

extern "C" int mmnas_alpha_two_step_cost(float* prob, const float* gate_grad, float* m, float* v, float* prob_grad,
                                         const float* cost, float* stats, int rows, int width, const int* pair_host, float lr,
                                         float beta1, float beta2, float eps, float weight_decay, float cost_weight, float cost_ref,
                                         int cost_form, int step, void* stream) {
  const char* who = "mmnas_alpha_two_step_cost";
  MMNAS_REQUIRE(rows >= 0 && rows <= ALPHA_TWO_MAX_ROWS, MMNAS_E_SHAPE, "%s: rows=%d (0..%d)", who, rows, ALPHA_TWO_MAX_ROWS);
  if (const int rc = alpha_cost_args(who, width, 2, step, "cost_form", "0 linear, 1 log", cost_form, cost_ref, cost_weight, false)) return rc;
  MMNAS_REQUIRE(prob && gate_grad && m && v && cost && pair_host, MMNAS_E_ARG, "%s: null pointer", who);
  AlphaPairArgs pa;
  if (const int rc = alpha_pair_args(who, pa, pair_host, rows, width)) return rc;
  const AlphaCost ac{cost, stats, cost_weight, cost_ref, cost_form};
  MMNAS_LAUNCH(alpha_two_step_cost_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, prob, gate_grad, m, v, prob_grad, rows, width,
               alpha_adam(lr, beta1, beta2, eps, weight_decay, step), pa, ac);
  return check_launch("alpha_two_step_cost");
}

extern "C" int mmnas_alpha_reinforce_step(float* prob, float* m, float* v, float* prob_grad, int rows, int width,
                                          const unsigned char* choice_host, const int* n_choices_host, int M, const float* quality,
                                          const float* cost, float cost_weight, float cost_ref, int reward_form, float* baseline,
                                          float baseline_decay, float* stats, int* err, float lr, float beta1, float beta2,
                                          float eps, float weight_decay, int step, void* stream) {
  const char* who = "mmnas_alpha_reinforce_step";
  MMNAS_REQUIRE(rows >= 0 && M >= 1, MMNAS_E_ARG, "%s: rows=%d (>= 0) M=%d (>= 1)", who, rows, M);
  if (const int rc = alpha_cost_args(who, width, 1, step, "reward_form", "0 mul, 1 add", reward_form, cost_ref, cost_weight, true)) return rc;
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
  const double decay = decimal_of(baseline_decay);
  const AlphaReinforce ar{quality, cost_weight != 0.f ? cost : nullptr, baseline, stats, err, decay, 1.0 - decay, cost_weight, cost_ref,
                          reward_form, M};
  MMNAS_LAUNCH(alpha_reinforce_step_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, prob, m, v, prob_grad, rows, width,
               alpha_adam(lr, beta1, beta2, eps, weight_decay, step), ar, ch);
  return check_launch("alpha_reinforce_step");
}
