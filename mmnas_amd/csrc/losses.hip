// The task losses of train_vgd / train_itm as one launch per direction; mmnas_amd/losses.py drives these:
//   * mmnas_vgd_loss_fwd         -- train_vgd.py:320-334 (REDUCTION = 'sum'): KLDiv or BCE-with-logits on the region scores +
//     LOSS_LAMBDA * SmoothL1 on the masked box targets, each over its LOSS_AVG denominator;
//   * mmnas_itm_triplet_loss_fwd -- mmnas/utils/itm_loss.py:4-24 (BCE_Loss: labels 1 / 0 / 0, the positive term twice) and
//     :27-37 (Margin_Loss: hinge with margin 0.2);
//   * mmnas_loss_grad_scale      -- the backward of both: the forward launch already wrote every gradient for an upstream
//     gradient of 1, this multiplies them by the upstream scalar (a device value).
// The problems are tiny (at most 64 x 100 x 4 floats), so each forward is ONE workgroup striding over the elements: per-thread
// partial sums in float64, a shuffle reduction per wave, the waves' sums through LDS, every thread adding them in the same order.
// No atomics: the same inputs give the same bits on every call.  The VGD gradients need the mask sums, so that kernel walks its
// inputs twice (the second pass hits the cache).

#include "common.h"

namespace mmnas {

constexpr int LOSS_THREADS = 1024;
constexpr int LOSS_WAVES = LOSS_THREADS / 64;

// Sums of NV values over the workgroup, returned to every thread.  red: NV * LOSS_WAVES doubles of LDS.
template <int NV>
__device__ __forceinline__ void block_sum(double (&v)[NV], double* red) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < NV; ++k) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v[k] += __shfl_xor(v[k], off);
  }
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < NV; ++k) red[k * LOSS_WAVES + w] = v[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < LOSS_WAVES; ++j) s += red[k * LOSS_WAVES + j];
    v[k] = s;
  }
}

// SmoothL1 (beta = 1) of one difference: value and derivative
__device__ __forceinline__ double smooth_l1(double d, double* g) {
  const double a = fabs(d);
  if (a < 1.0) {
    *g = d;
    return 0.5 * d * d;
  }
  *g = d > 0.0 ? 1.0 : -1.0;   // (a NaN difference: the value below is NaN, and so is the loss)
  return a - 0.5;
}

// ------------------------------------------------------------------------------------------
// VGD loss.  n = B * S regions; smask holds n values (smask_full) or B (one per sample); bmask 4 n values (bmask_full) or n.
// The products with the masks are float32 products, as the reference forms them before the loss functions see them.
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(LOSS_THREADS) vgd_loss_kernel(const float* __restrict__ ps, const float4* __restrict__ pr,
                                                                const float* __restrict__ sc, const float4* __restrict__ bb,
                                                                const float* __restrict__ smask, const float* __restrict__ bmask,
                                                                int B, int S, int smask_full, int bmask_full, int bce, int loss_avg,
                                                                double batch_size, double lam, float* __restrict__ loss,
                                                                float* __restrict__ parts, float* __restrict__ dps,
                                                                float4* __restrict__ dpr) {
  __shared__ double red[4 * LOSS_WAVES];
  const int n = B * S;
  const int tid = threadIdx.x;
  double v[4] = {0.0, 0.0, 0.0, 0.0};   // score term, box term, sum of scores_mask, sum of bbox_mask (each as given)
  for (int i = tid; i < n; i += LOSS_THREADS) {
    const float m = smask_full ? smask[i] : smask[i / S];
    if (smask_full) v[2] += (double)m;
    const float p = ps[i], t = sc[i];
    if (bce) {   // max(x, 0) - x t + log1p(exp(-|x|)); the mask does not enter
      const double x = p;
      v[0] += fmax(x, 0.0) - x * (double)t + log1p(exp(-fabs(x)));
    } else {     // xlogy(t m, t m) - t m * (p m): a zero target contributes nothing
      const float tm = t * m, pm = p * m;
      const double td = tm;
      v[0] += (tm == 0.f ? 0.0 : td * log(td)) - td * (double)pm;
    }
    const float4 q = pr[i], g = bb[i];
    float4 k;
    if (bmask_full) {
      k = reinterpret_cast<const float4*>(bmask)[i];
      v[3] += ((double)k.x + (double)k.y) + ((double)k.z + (double)k.w);
    } else {
      const float b1 = bmask[i];
      k = make_float4(b1, b1, b1, b1);
      v[3] += (double)b1;
    }
    double unused;
    v[1] += (smooth_l1((double)(q.x * k.x) - (double)(g.x * k.x), &unused) + smooth_l1((double)(q.y * k.y) - (double)(g.y * k.y), &unused)) +
            (smooth_l1((double)(q.z * k.z) - (double)(g.z * k.z), &unused) + smooth_l1((double)(q.w * k.w) - (double)(g.w * k.w), &unused));
  }
  if (!smask_full) {
    for (int b = tid; b < B; b += LOSS_THREADS) v[2] += (double)smask[b];
  }
  block_sum<4>(v, red);
  // LOSS_AVG: the score term over the mask's sum (kld) or BATCH_SIZE (bce), the box term over its mask's sum; an empty mask
  // is the reference's own 0 / 0
  const double den_s = loss_avg ? (bce ? batch_size : v[2]) : 1.0;
  const double den_r = loss_avg ? v[3] : 1.0;
  if (tid == 0) {
    const double ls = v[0] / den_s, lr = v[1] / den_r;
    loss[0] = (float)(ls + lam * lr);
    parts[0] = (float)ls;
    parts[1] = (float)lr;
    parts[2] = (float)v[2];
    parts[3] = (float)v[3];
  }
  if (!dps) return;   // no gradient wanted (uniform)
  for (int i = tid; i < n; i += LOSS_THREADS) {
    if (bce) {
      const double x = ps[i];
      dps[i] = (float)((1.0 / (1.0 + exp(-x)) - (double)sc[i]) / den_s);
    } else {
      const float m = smask_full ? smask[i] : smask[i / S];
      dps[i] = (float)(-((double)(sc[i] * m) * (double)m) / den_s);
    }
    const float4 q = pr[i], g = bb[i];
    float4 k;
    if (bmask_full) {
      k = reinterpret_cast<const float4*>(bmask)[i];
    } else {
      const float b1 = bmask[i];
      k = make_float4(b1, b1, b1, b1);
    }
    double d[4];
    smooth_l1((double)(q.x * k.x) - (double)(g.x * k.x), &d[0]);
    smooth_l1((double)(q.y * k.y) - (double)(g.y * k.y), &d[1]);
    smooth_l1((double)(q.z * k.z) - (double)(g.z * k.z), &d[2]);
    smooth_l1((double)(q.w * k.w) - (double)(g.w * k.w), &d[3]);
    const double c = lam / den_r;
    dpr[i] = make_float4((float)(d[0] * (double)k.x * c), (float)(d[1] * (double)k.y * c), (float)(d[2] * (double)k.z * c),
                         (float)(d[3] * (double)k.w * c));
  }
}

// ------------------------------------------------------------------------------------------
// ITM triplet losses over n scores per role.  grads (nullable) [3, n]: d loss / d (pos, negc, negi).
//   bce:    -max(log s, -100) for the label 1, -max(log(1 - s), -100) for the label 0 (torch.nn.BCELoss's clamp); the backward
//           is torch's binary_cross_entropy_backward: (s - label) / max((1 - s) s, 1e-12).
//   margin: max(0, (margin + s_neg) - s_pos), float32 as the reference forms it; clamp(min=0) passes the gradient at >= 0.
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ double bce_term(double s, int label, double* g) {
  const double arg = label ? s : 1.0 - s;
  *g = (s - (double)label) / fmax((1.0 - s) * s, 1e-12);
  return -fmax(log(arg), -100.0);
}

__global__ void __launch_bounds__(LOSS_THREADS) itm_triplet_loss_kernel(const float* __restrict__ sp, const float* __restrict__ sc,
                                                                        const float* __restrict__ si, long n, int margin_mode,
                                                                        float margin, int mean, float* __restrict__ loss,
                                                                        float* __restrict__ grads) {
  __shared__ double red[LOSS_WAVES];
  const double scale = mean ? 1.0 / (double)n : 1.0;
  double v[1] = {0.0};
  for (long i = threadIdx.x; i < n; i += LOSS_THREADS) {
    double gp, gc, gi;
    if (margin_mode) {
      const float cc = (margin + sc[i]) - sp[i], ci = (margin + si[i]) - sp[i];
      v[0] += (double)(cc > 0.f ? cc : (cc != cc ? cc : 0.f)) + (double)(ci > 0.f ? ci : (ci != ci ? ci : 0.f));
      gc = cc >= 0.f ? 1.0 : 0.0;
      gi = ci >= 0.f ? 1.0 : 0.0;
      gp = -(gc + gi);
    } else {
      const double lp = bce_term(sp[i], 1, &gp), lc = bce_term(sc[i], 0, &gc), ln = bce_term(si[i], 0, &gi);
      v[0] += (lp + lc) + (lp + ln);
      gp *= 2.0;   // the positive term enters twice
    }
    if (grads) {
      grads[i] = (float)(gp * scale);
      grads[n + i] = (float)(gc * scale);
      grads[2 * n + i] = (float)(gi * scale);
    }
  }
  block_sum<1>(v, red);
  if (threadIdx.x == 0) loss[0] = (float)(v[0] * scale);
}

__global__ void __launch_bounds__(256) loss_grad_scale_kernel(const float* __restrict__ saved, const float* __restrict__ go,
                                                              float* __restrict__ out, size_t n) {
  const float g = go[0];
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) out[i] = g * saved[i];
}

}  // namespace mmnas

using namespace mmnas;

static bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

extern "C" int mmnas_vgd_loss_fwd(const float* pred_scores, const float* pred_reg, const float* scores, const float* bbox,
                                  const float* scores_mask, const float* bbox_mask, int B, int S, int smask_full, int bmask_full,
                                  int mode, int loss_avg, double batch_size, double lam, float* loss, float* parts,
                                  float* dpred_scores, float* dpred_reg, void* stream) {
  MMNAS_REQUIRE(B >= 1 && S >= 1 && (long)B * S <= (1L << 28), MMNAS_E_SHAPE, "vgd_loss_fwd: B=%d S=%d (B, S >= 1, B*S <= 2^28)", B, S);
  MMNAS_REQUIRE(mode == 0 || mode == 1, MMNAS_E_ARG, "vgd_loss_fwd: mode %d (0 = kld, 1 = bce)", mode);
  MMNAS_REQUIRE(pred_scores && pred_reg && scores && bbox && scores_mask && bbox_mask && loss && parts, MMNAS_E_ARG,
                "vgd_loss_fwd: null pointer");
  MMNAS_REQUIRE((dpred_scores == nullptr) == (dpred_reg == nullptr), MMNAS_E_ARG,
                "vgd_loss_fwd: dpred_scores and dpred_reg are given together or not at all");
  MMNAS_REQUIRE(aligned16(pred_reg) && aligned16(bbox) && (!bmask_full || aligned16(bbox_mask)) && aligned16(dpred_reg), MMNAS_E_ARG,
                "vgd_loss_fwd: pred_reg, bbox, a full bbox_mask and dpred_reg must be 16-byte aligned");
  MMNAS_LAUNCH(vgd_loss_kernel, dim3(1), dim3(LOSS_THREADS), 0, (hipStream_t)stream, pred_scores, (const float4*)pred_reg, scores,
               (const float4*)bbox, scores_mask, bbox_mask, B, S, smask_full ? 1 : 0, bmask_full ? 1 : 0, mode, loss_avg ? 1 : 0,
               batch_size, lam, loss, parts, dpred_scores, (float4*)dpred_reg);
  return check_launch("vgd_loss_fwd");
}

extern "C" int mmnas_itm_triplet_loss_fwd(const float* scores_pos, const float* scores_negc, const float* scores_negi, long n, int mode,
                                          float margin, int mean, float* loss, float* grads, void* stream) {
  MMNAS_REQUIRE(n >= 0 && n <= (1L << 28), MMNAS_E_SHAPE, "itm_triplet_loss_fwd: n=%ld (0 <= n <= 2^28)", n);
  MMNAS_REQUIRE(mode == 0 || mode == 1, MMNAS_E_ARG, "itm_triplet_loss_fwd: mode %d (0 = bce, 1 = margin)", mode);
  MMNAS_REQUIRE(loss && (n == 0 || (scores_pos && scores_negc && scores_negi)), MMNAS_E_ARG, "itm_triplet_loss_fwd: null pointer");
  MMNAS_LAUNCH(itm_triplet_loss_kernel, dim3(1), dim3(LOSS_THREADS), 0, (hipStream_t)stream, scores_pos, scores_negc, scores_negi, n,
               mode, margin, mean ? 1 : 0, loss, grads);
  return check_launch("itm_triplet_loss_fwd");
}

extern "C" int mmnas_loss_grad_scale(const float* saved, const float* go, float* out, size_t n, void* stream) {
  MMNAS_REQUIRE(n <= ((size_t)1 << 31), MMNAS_E_SHAPE, "loss_grad_scale: n=%zu (n <= 2^31)", n);
  if (n == 0) return MMNAS_OK;
  MMNAS_REQUIRE(saved && go && out, MMNAS_E_ARG, "loss_grad_scale: null pointer");
  MMNAS_LAUNCH(loss_grad_scale_kernel, dim3(cdiv((long)n, 256) < 64 ? cdiv((long)n, 256) : 64), dim3(256), 0, (hipStream_t)stream,
               saved, go, out, n);
  return check_launch("loss_grad_scale");
}
