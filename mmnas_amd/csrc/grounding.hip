// Visual grounding (configs[3], train_vgd) outside the training step; mmnas_amd/grounding.py drives these:
//   * mmnas_vgd_targets -- the loader's per-sample training targets (load_data_vgd.py:228-282 get_sigmoid_score /
//     proc_bbox_label, bbox_transform.py:10-27 bbox_transform, overlaps.py bbox_overlaps) for a whole batch;
//   * mmnas_vgd_ground  -- one evaluation batch of train_vgd.py:436-453: argmax region, bbox_transform_inv of that row only
//     (bbox_transform.py:29-63), clip_boxes (:65-78), IoU with the ground truth, hit = IoU >= threshold.
// One wave per sample, four samples per 256-thread workgroup, the lanes striding over the S regions.
//
// Numerics restate the reference's host arithmetic operation for operation, so FP contraction is off for this file: a fused
// multiply-add would round once where numpy rounds twice.
#pragma clang fp contract(off)

#include "common.h"

namespace mmnas {

constexpr int VGD_MAXS = 1024;
constexpr int VGD_ERR_NONFINITE = 1, VGD_ERR_NOBJ = 2;

struct VgdNorm {
  double mean[4], std[4];
  int on;
};

// Python's min / max on two floats: min(a, b) = b if b < a else a (max likewise)
__device__ __forceinline__ double py_min(double a, double b) { return b < a ? b : a; }
__device__ __forceinline__ double py_max(double a, double b) { return b > a ? b : a; }
// np.minimum / np.maximum of float32: a NaN first operand propagates
__device__ __forceinline__ float np_min(float a, float b) { return (a <= b || a != a) ? a : b; }
__device__ __forceinline__ float np_max(float a, float b) { return (a >= b || a != a) ? a : b; }

// overlaps.py bbox_overlaps for one box b against one query box q, in its order and with its +1 convention (strict iw / ih tests)
__device__ __forceinline__ double vgd_iou(double b0, double b1, double b2, double b3, double q0, double q1, double q2, double q3) {
  const double box_area = (q2 - q0 + 1.0) * (q3 - q1 + 1.0);
  const double iw = py_min(b2, q2) - py_max(b0, q0) + 1.0;
  if (!(iw > 0.0)) return 0.0;
  const double ih = py_min(b3, q3) - py_max(b1, q1) + 1.0;
  if (!(ih > 0.0)) return 0.0;
  const double ua = (b2 - b0 + 1.0) * (b3 - b1 + 1.0) + box_area - iw * ih;
  return iw * ih / ua;
}

// numpy's float32 pairwise sum (an add.reduce over a contiguous array): blocks of <= 128 elements in 8 strided partial sums,
// combined ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)), then the tail in order; longer arrays split at n/2 rounded down to a multiple
// of 8.  Five levels cover n <= 1024 (1024 -> 519 -> 263 -> 135 -> 71).
__device__ float pw_leaf(const float* a, int n) {
  if (n < 8) {
    float r = -0.0f;
    for (int i = 0; i < n; ++i) r += a[i];
    return r;
  }
  float r[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) r[j] = a[j];
  int i = 8;
  for (; i < n - n % 8; i += 8) {
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] += a[i + j];
  }
  float res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
  for (; i < n; ++i) res += a[i];
  return res;
}

template <int D>
__device__ float pw_sum(const float* a, int n) {
  if constexpr (D == 0) {
    return pw_leaf(a, n);
  } else {
    if (n <= 128) return pw_leaf(a, n);
    int n2 = n / 2;
    n2 -= n2 % 8;
    return pw_sum<D - 1>(a, n2) + pw_sum<D - 1>(a + n2, n - n2);
  }
}

__device__ __forceinline__ bool finite4(float a, float b, float c, float d) {
  return isfinite(a) && isfinite(b) && isfinite(c) && isfinite(d);
}

// ------------------------------------------------------------------------------------------
// targets: lane holds rows lane + 64 i (i < 16); the un-normalised scores go through LDS for the pairwise sum (lane 0)
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) vgd_targets_kernel(const float* __restrict__ bbox, const int* __restrict__ nobj,
                                                          const double* __restrict__ gt, int B, int S, double thr, int bce,
                                                          VgdNorm nrm, float* __restrict__ scores, float* __restrict__ scores_mask,
                                                          float* __restrict__ transformed, float* __restrict__ bbox_mask,
                                                          int* __restrict__ err) {
  __shared__ float srow[4][VGD_MAXS];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int b = blockIdx.x * 4 + w;
  if (b >= B) return;   // wave-uniform; no workgroup barrier below
  float* row = srow[w];
  int n = nobj[b];
  int bad = 0;
  if (n < 1 || n > S) {   // the sample's outputs are all zero
    bad |= VGD_ERR_NOBJ;
    n = 0;
  }
  const double q0 = gt[4 * (size_t)b], q1 = gt[4 * (size_t)b + 1], q2 = gt[4 * (size_t)b + 2], q3 = gt[4 * (size_t)b + 3];
  if (!(isfinite(q0) && isfinite(q1) && isfinite(q2) && isfinite(q3))) bad |= VGD_ERR_NONFINITE;
  // bbox_transform's ground-truth side (float64)
  const double gw = q2 - q0 + 1.0, gh = q3 - q1 + 1.0;
  const double gcx = q0 + 0.5 * gw, gcy = q1 + 0.5 * gh;
  unsigned ge_bits = 0;   // bit i: row lane + 64 i has overlap >= thr
  int any_ge = 0, any_nan = 0;
  for (int r = lane, i = 0; r < S; r += 64, ++i) {
    const size_t o = (size_t)b * S + r;
    float s = 0.f;
    float t[4] = {0.f, 0.f, 0.f, 0.f};
    if (r < n) {
      const float p0 = bbox[4 * o], p1 = bbox[4 * o + 1], p2 = bbox[4 * o + 2], p3 = bbox[4 * o + 3];
      if (!finite4(p0, p1, p2, p3)) bad |= VGD_ERR_NONFINITE;
      const double ov = vgd_iou(p0, p1, p2, p3, q0, q1, q2, q3);
      any_nan |= ov != ov;
      if (ov >= thr) {
        any_ge = 1;
        ge_bits |= 1u << i;
        // kld: the overlap stored into the float32 score array; bce: get_sigmoid_score's steps
        s = bce ? (ov < 0.6 ? 0.8f : ov < 0.7 ? 0.9f : 1.0f) : (float)ov;
      }
      // bbox_transform: the proposal side in float32 (a float32 array + 1.0), the rest in float64, one rounding at the end
      const float ew = p2 - p0 + 1.0f, eh = p3 - p1 + 1.0f;
      const float ecx = p0 + 0.5f * ew, ecy = p1 + 0.5f * eh;
      double d[4];
      d[0] = (gcx - (double)ecx) / (double)ew;
      d[1] = (gcy - (double)ecy) / (double)eh;
      d[2] = log(gw / (double)ew);
      d[3] = log(gh / (double)eh);
#pragma unroll
      for (int k = 0; k < 4; ++k) t[k] = (float)(nrm.on ? (d[k] - nrm.mean[k]) / nrm.std[k] : d[k]);
    }
    row[r] = s;
#pragma unroll
    for (int k = 0; k < 4; ++k) transformed[4 * o + k] = t[k];
  }
  // overlaps.max() >= thr (a NaN overlap makes the maximum NaN: no target)
  const bool on = __ballot(any_ge) != 0 && __ballot(any_nan) == 0;
  float tot = 1.0f;
  if (on && !bce) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    float sum = 0.f;
    if (lane == 0) sum = pw_sum<5>(row, S);
    tot = __shfl(sum, 0) + 1e-8f;   // scores / (scores.sum() + 1e-8), float32
  }
  for (int r = lane, i = 0; r < S; r += 64, ++i) {
    const size_t o = (size_t)b * S + r;
    const bool m = on && ((ge_bits >> i) & 1u);
    const float s = row[r];   // (written by this lane)
    scores[o] = on ? (bce ? s : s / tot) : 0.f;
    bbox_mask[o] = m ? 1.f : 0.f;
  }
  if (lane == 0) {
    scores_mask[b] = on ? 1.f : 0.f;
  }
  bad = __ballot(bad & VGD_ERR_NONFINITE) ? (bad | VGD_ERR_NONFINITE) : bad;
  if (lane == 0 && bad) atomicOr(err, bad);
}

// ------------------------------------------------------------------------------------------
// evaluation: argmax over the S scores (ties: the lowest index, as np.argmax), then lane 0 decodes, clips and scores that row
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) vgd_ground_kernel(const float* __restrict__ ps, const float* __restrict__ reg,
                                                         const float* __restrict__ bbox, const float* __restrict__ img_shape,
                                                         const float* __restrict__ gt, int B, int S, double thr,
                                                         long long* __restrict__ idx_out, float* __restrict__ box_out,
                                                         double* __restrict__ iou_out, unsigned char* __restrict__ hit_out,
                                                         unsigned long long* __restrict__ counts, int* __restrict__ err) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int b = blockIdx.x * 4 + w;
  if (b >= B) return;   // wave-uniform
  float best = 0.f;
  int bi = S;   // S = none yet
  int bad = 0;
  for (int r = lane; r < S; r += 64) {
    const size_t o = (size_t)b * S + r;
    const float v = ps[o];
    if (!isfinite(v) || !finite4(reg[4 * o], reg[4 * o + 1], reg[4 * o + 2], reg[4 * o + 3])) bad = 1;
    if (bi == S || v > best) {
      best = v;
      bi = r;
    }
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const float ob = __shfl_xor(best, off);
    const int oi = __shfl_xor(bi, off);
    if (oi < S && (bi == S || ob > best || (ob == best && oi < bi))) {
      best = ob;
      bi = oi;
    }
  }
  const bool any_bad = __ballot(bad) != 0;
  if (lane != 0) return;
  const size_t o = (size_t)b * S + bi;
  // bbox_transform_inv of one row, all in float32
  const float b0 = bbox[4 * o], b1 = bbox[4 * o + 1], b2 = bbox[4 * o + 2], b3 = bbox[4 * o + 3];
  const float dx = reg[4 * o], dy = reg[4 * o + 1], dw = reg[4 * o + 2], dh = reg[4 * o + 3];
  const float wd = b2 - b0 + 1.0f, ht = b3 - b1 + 1.0f;
  const float cx = b0 + 0.5f * wd, cy = b1 + 0.5f * ht;
  const float pcx = dx * wd + cx, pcy = dy * ht + cy;
  const float pw = expf(dw) * wd, ph = expf(dh) * ht;
  // clip_boxes: x to [0, w - 1], y to [0, h - 1] (img_shape = (h, w))
  const float xm = img_shape[2 * (size_t)b + 1] - 1.0f, ym = img_shape[2 * (size_t)b] - 1.0f;
  const float x1 = np_max(np_min(pcx - 0.5f * pw, xm), 0.f);
  const float y1 = np_max(np_min(pcy - 0.5f * ph, ym), 0.f);
  const float x2 = np_max(np_min(pcx + 0.5f * pw, xm), 0.f);
  const float y2 = np_max(np_min(pcy + 0.5f * ph, ym), 0.f);
  const double iou = vgd_iou(x1, y1, x2, y2, gt[4 * (size_t)b], gt[4 * (size_t)b + 1], gt[4 * (size_t)b + 2], gt[4 * (size_t)b + 3]);
  const int hit = iou >= thr;
  idx_out[b] = bi;
  box_out[4 * (size_t)b] = x1;
  box_out[4 * (size_t)b + 1] = y1;
  box_out[4 * (size_t)b + 2] = x2;
  box_out[4 * (size_t)b + 3] = y2;
  iou_out[b] = iou;
  hit_out[b] = (unsigned char)hit;
  if (counts) {
    if (hit) atomicAdd(counts, 1ull);
    atomicAdd(counts + 1, 1ull);
  }
  if (any_bad) atomicOr(err, VGD_ERR_NONFINITE);
}

}  // namespace mmnas

using namespace mmnas;

extern "C" int mmnas_vgd_targets(const float* bbox, const int* nobj, const double* gt, int B, int S, double thr, int mode,
                                 const double* norm, float* scores, float* scores_mask, float* transformed, float* bbox_mask,
                                 int* err_flag, void* stream) {
  MMNAS_REQUIRE(B >= 0 && S >= 1 && S <= VGD_MAXS, MMNAS_E_SHAPE, "vgd_targets: B=%d S=%d (B >= 0, 1 <= S <= %d)", B, S, VGD_MAXS);
  MMNAS_REQUIRE(mode == 0 || mode == 1, MMNAS_E_ARG, "vgd_targets: mode %d (0 = kld, 1 = bce)", mode);
  MMNAS_REQUIRE(bbox && nobj && gt && scores && scores_mask && transformed && bbox_mask && err_flag, MMNAS_E_ARG,
                "vgd_targets: null pointer");
  VgdNorm nrm = {};
  if (norm) {
    for (int k = 0; k < 4; ++k) {
      nrm.mean[k] = norm[k];
      nrm.std[k] = norm[4 + k];
    }
    nrm.on = 1;
  }
  if (B == 0) return MMNAS_OK;
  MMNAS_LAUNCH(vgd_targets_kernel, dim3(cdiv(B, 4)), dim3(256), 0, (hipStream_t)stream, bbox, nobj, gt, B, S, thr, mode, nrm,
               scores, scores_mask, transformed, bbox_mask, err_flag);
  return check_launch("vgd_targets");
}

extern "C" int mmnas_vgd_ground(const float* pred_scores, const float* pred_reg, const float* bbox, const float* img_shape,
                                const float* gt, int B, int S, double thr, long long* idx, float* box, double* iou,
                                unsigned char* hit, long long* counts, int* err_flag, void* stream) {
  MMNAS_REQUIRE(B >= 0 && S >= 1 && S <= VGD_MAXS, MMNAS_E_SHAPE, "vgd_ground: B=%d S=%d (B >= 0, 1 <= S <= %d)", B, S, VGD_MAXS);
  MMNAS_REQUIRE(pred_scores && pred_reg && bbox && img_shape && gt && idx && box && iou && hit && err_flag, MMNAS_E_ARG,
                "vgd_ground: null pointer");
  if (B == 0) return MMNAS_OK;
  MMNAS_LAUNCH(vgd_ground_kernel, dim3(cdiv(B, 4)), dim3(256), 0, (hipStream_t)stream, pred_scores, pred_reg, bbox, img_shape, gt,
               B, S, thr, idx, box, iou, hit, (unsigned long long*)counts, err_flag);
  return check_launch("vgd_ground");
}
