// VQA (configs[0] / [1], search_vqa / train_vqa) outside the training step; mmnas_amd/answering.py drives these:
//   * mmnas_vqa_answer         -- one evaluation batch of train_vqa.py:379-393: per row the argmax answer (np.argmax's rule),
//     then that answer's VQAEval credit for the row's question, looked up in the CSR table AnswerCredit builds on the host;
//   * mmnas_vqa_accuracy       -- the sums of VQAEval.setAccuracy (vqaEval.py:143-146) as exact integers, by answer type and
//     by question type;
//   * mmnas_vqa_answer_targets -- the loader's soft answer targets (load_data_vqa.py:299-333 proc_ans / get_score) for a batch
//     of answer-index lists;
//   * mmnas_vqa_soft_accuracy  -- those targets' score of the predicted answer, target[b, argmax logits[b]], and its batch
//     mean as a device scalar: the reward of a REINFORCE architecture step (harness.SearchLoop(arch_mode='reinforce')).
// The argmax and the targets run one wave per row, four rows per 256-thread workgroup.  Logit rows are 4-byte aligned only
// (3129 floats), so every load is a single dword.
#include "common.h"

namespace mmnas {

constexpr int VQA_MAX_TYPES = 256, VQA_MAX_N = 64;
constexpr int VQA_ERR_NAN = 1, VQA_ERR_INDEX = 2;

// (v, i) comes before (bv, bi) in np.argmax's order: NaN above every number (the first NaN wins), then the larger value, then
// the lower index.  bi < 0: nothing yet.
__device__ __forceinline__ bool vqa_before(float v, int i, float bv, int bi) {
  if (bi < 0) return true;
  const bool vn = v != v, bn = bv != bv;
  if (vn || bn) return vn && (!bn || i < bi);
  return v > bv || (v == bv && i < bi);
}

// ------------------------------------------------------------------------------------------
// argmax + credit: lanes stride over the A logits of row b, a butterfly over (value, index) pairs, then the lanes scan the
// <= n table entries of the row's question for the predicted column
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) vqa_answer_kernel(const float* __restrict__ logits, int B, int A, long ld,
                                                         const int* __restrict__ slot_idx, long slot_base, int slot_step,
                                                         int nslots, const int* __restrict__ qmap, const int* __restrict__ row_ptr,
                                                         const int* __restrict__ col, const int* __restrict__ kval, int nq,
                                                         long long* __restrict__ pred, int* __restrict__ credit,
                                                         int* __restrict__ count, int* __restrict__ err) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int b = blockIdx.x * 4 + w;
  if (b >= B) return;   // wave-uniform; no workgroup barrier below
  int bad = 0;
  const long slot = slot_idx ? (long)slot_idx[b] : slot_base + (long)slot_step * b;
  if (slot == -1) return;   // skipped row
  if (slot < -1 || slot >= nslots) {   // >= nslots: the sampler's wrap-around padding; out of range when given explicitly
    if ((slot_idx || slot < -1) && lane == 0) atomicOr(err, VQA_ERR_INDEX);
    return;
  }
  const float* row = logits + (size_t)b * ld;
  float bv = 0.f;
  int bi = -1;
#pragma unroll 4
  for (int c = lane; c < A; c += 64) {
    const float v = row[c];
    if (vqa_before(v, c, bv, bi)) {
      bv = v;
      bi = c;
    }
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const float ov = __shfl_xor(bv, off);
    const int oi = __shfl_xor(bi, off);
    if (oi >= 0 && vqa_before(ov, oi, bv, bi)) {
      bv = ov;
      bi = oi;
    }
  }
  if (bv != bv) bad |= VQA_ERR_NAN;   // NaN ranks first: the row holds one iff its maximum is NaN
  int k = -1;
  if (credit) {
    const int q = qmap ? qmap[slot] : (int)slot;
    if (q < -1 || q >= nq) bad |= VQA_ERR_INDEX;
    if (q >= 0 && q < nq) {
      k = 0;
      const int e0 = row_ptr[q], e1 = row_ptr[q + 1];
      for (int e = e0 + lane; e < e1; e += 64) {
        const unsigned long long hit = __ballot(col[e] == bi);
        if (hit) {
          k = __shfl(kval[e], __ffsll((long long)hit) - 1);
          break;
        }
      }
    }
  }
  if (lane != 0) return;
  pred[slot] = bi;
  if (credit) credit[slot] = k;
  if (count) atomicAdd(count + slot, 1);
  if (bad) atomicOr(err, bad);
}

// ------------------------------------------------------------------------------------------
// accuracy: LDS histograms (credit sum, count) per answer type and per question type, then one global 64-bit atomic per
// non-empty bin and workgroup.  Integer adds: the totals do not depend on the order.
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) vqa_accuracy_kernel(const int* __restrict__ credit, const int* __restrict__ qmap,
                                                           const int* __restrict__ ans_type, const int* __restrict__ ques_type,
                                                           int N, int nq, int n_at, int n_qt, unsigned long long* __restrict__ totals,
                                                           int* __restrict__ err) {
  __shared__ unsigned int h[4][VQA_MAX_TYPES];   // answer-type sum, count, question-type sum, count
  for (int i = threadIdx.x; i < 4 * VQA_MAX_TYPES; i += 256) h[i / VQA_MAX_TYPES][i % VQA_MAX_TYPES] = 0u;
  __syncthreads();
  int bad = 0;
  for (long p = (long)blockIdx.x * 256 + threadIdx.x; p < N; p += (long)gridDim.x * 256) {
    const int q = qmap ? qmap[p] : (int)p;
    if (q < 0 || q >= nq) {
      bad = 1;
      continue;
    }
    const int a = ans_type[q], t = ques_type[q], c = credit[p];
    if (a < 0 || a >= n_at || t < 0 || t >= n_qt || c < 0) {
      bad = 1;
      continue;
    }
    atomicAdd(&h[0][a], (unsigned)c);
    atomicAdd(&h[1][a], 1u);
    atomicAdd(&h[2][t], (unsigned)c);
    atomicAdd(&h[3][t], 1u);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < n_at; i += 256) {
    if (h[1][i]) {
      atomicAdd(totals + i, (unsigned long long)h[0][i]);
      atomicAdd(totals + n_at + i, (unsigned long long)h[1][i]);
    }
  }
  for (int i = threadIdx.x; i < n_qt; i += 256) {
    if (h[3][i]) {
      atomicAdd(totals + 2 * n_at + i, (unsigned long long)h[2][i]);
      atomicAdd(totals + 2 * n_at + n_qt + i, (unsigned long long)h[3][i]);
    }
  }
  if (bad) atomicOr(err, VQA_ERR_INDEX);
}

// ------------------------------------------------------------------------------------------
// soft targets: the row's n answer indices go to LDS; every lane counts each of its columns among them and writes the score,
// zeros included (the whole [A] row is written)
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) vqa_answer_targets_kernel(const int* __restrict__ ans_ix, int B, int n, int A,
                                                                 float* __restrict__ out, int* __restrict__ err) {
  __shared__ int sidx[4][VQA_MAX_N];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int b = blockIdx.x * 4 + w;
  if (b >= B) return;   // wave-uniform
  int bad = 0;
  if (lane < n) {
    int v = ans_ix[(size_t)b * n + lane];
    if (v < -1 || v >= A) {
      bad = 1;
      v = -1;
    }
    sidx[w][lane] = v;
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  float* o = out + (size_t)b * A;
  for (int c = lane; c < A; c += 64) {
    int cnt = 0;
    for (int j = 0; j < n; ++j) cnt += sidx[w][j] == c;
    // get_score: 0 / .3 / .6 / .9 / 1 (the float32 values of the loader's Python floats)
    o[c] = cnt == 0 ? 0.0f : cnt == 1 ? 0.3f : cnt == 2 ? 0.6f : cnt == 3 ? 0.9f : 1.0f;
  }
  if (__ballot(bad) && lane == 0) atomicOr(err, VQA_ERR_INDEX);
}

// ------------------------------------------------------------------------------------------
// soft accuracy: target[b, argmax_a logits[b, a]] per row and its mean.  ONE workgroup: wave w takes the rows w, w + 4, ... in
// that order and adds their scores in double; the four sums meet in LDS as (s0 + s1) + (s2 + s3).  No atomics: the NaN flag is
// a plain store of 1.
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) vqa_soft_accuracy_kernel(const float* __restrict__ logits, long ld, const float* __restrict__ target,
                                                                long ldt, int B, int A, float* __restrict__ per_row,
                                                                float* __restrict__ out, int* __restrict__ nan_flag) {
  __shared__ double part[4];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  double sum = 0.0;
  bool nan = false;
  for (int b = w; b < B; b += 4) {
    const float* row = logits + (size_t)b * ld;
    float bv = 0.f;
    int bi = -1;
#pragma unroll 4
    for (int c = lane; c < A; c += 64) {
      const float v = row[c];
      if (vqa_before(v, c, bv, bi)) {
        bv = v;
        bi = c;
      }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      const float ov = __shfl_xor(bv, off);
      const int oi = __shfl_xor(bi, off);
      if (oi >= 0 && vqa_before(ov, oi, bv, bi)) {
        bv = ov;
        bi = oi;
      }
    }
    nan |= bv != bv;                       // NaN ranks first: the row holds one iff its maximum is NaN
    const float s = target[(size_t)b * ldt + bi];   // (A >= 1: every wave ends with 0 <= bi < A)
    if (per_row && lane == 0) per_row[b] = s;
    sum += (double)s;
  }
  if (lane == 0) {
    part[w] = sum;
    if (nan) *nan_flag = 1;
  }
  __syncthreads();
  if (threadIdx.x == 0) out[0] = (float)(((part[0] + part[1]) + (part[2] + part[3])) / (double)B);
}

}  // namespace mmnas

using namespace mmnas;

extern "C" int mmnas_vqa_answer(const float* logits, int B, int A, long ld, const int* slot_idx, long slot_base, int slot_step,
                                int nslots, const int* qmap, const int* row_ptr, const int* col, const int* kval, int nq,
                                long long* pred, int* credit, int* count, int* err_flag, void* stream) {
  MMNAS_REQUIRE(B >= 0 && A >= 1 && ld >= A && nslots >= 0 && nq >= 0, MMNAS_E_SHAPE,
                "vqa_answer: B=%d A=%d ld=%ld nslots=%d nq=%d (B >= 0, 1 <= A <= ld, nslots, nq >= 0)", B, A, ld, nslots, nq);
  MMNAS_REQUIRE(logits && pred && err_flag, MMNAS_E_ARG, "vqa_answer: null pointer");
  MMNAS_REQUIRE(!credit || (row_ptr && col && kval), MMNAS_E_ARG, "vqa_answer: credit needs row_ptr, col and k");
  if (B == 0) return MMNAS_OK;
  MMNAS_LAUNCH(vqa_answer_kernel, dim3(cdiv(B, 4)), dim3(256), 0, (hipStream_t)stream, logits, B, A, ld, slot_idx, slot_base,
               slot_step, nslots, qmap, row_ptr, col, kval, nq, pred, credit, count, err_flag);
  return check_launch("vqa_answer");
}

extern "C" int mmnas_vqa_accuracy(const int* credit, const int* qmap, const int* ans_type, const int* ques_type, int N, int nq,
                                  int n_at, int n_qt, long long* totals, int* err_flag, void* stream) {
  MMNAS_REQUIRE(N >= 0 && N <= (1 << 28) && nq >= 0 && n_at >= 1 && n_at <= VQA_MAX_TYPES && n_qt >= 1 && n_qt <= VQA_MAX_TYPES,
                MMNAS_E_SHAPE, "vqa_accuracy: N=%d nq=%d types %d / %d (0 <= N <= 2^28, 1 <= types <= %d)", N, nq, n_at, n_qt,
                VQA_MAX_TYPES);
  MMNAS_REQUIRE(credit && ans_type && ques_type && totals && err_flag, MMNAS_E_ARG, "vqa_accuracy: null pointer");
  if (N == 0) return MMNAS_OK;
  MMNAS_LAUNCH(vqa_accuracy_kernel, dim3(cdiv(N, 256) < 1024 ? cdiv(N, 256) : 1024), dim3(256), 0, (hipStream_t)stream, credit,
               qmap, ans_type, ques_type, N, nq, n_at, n_qt, (unsigned long long*)totals, err_flag);
  return check_launch("vqa_accuracy");
}

extern "C" int mmnas_vqa_answer_targets(const int* ans_ix, int B, int n, int A, float* out, int* err_flag, void* stream) {
  MMNAS_REQUIRE(B >= 0 && n >= 1 && n <= VQA_MAX_N && A >= 1, MMNAS_E_SHAPE,
                "vqa_answer_targets: B=%d n=%d A=%d (B >= 0, 1 <= n <= %d, A >= 1)", B, n, A, VQA_MAX_N);
  MMNAS_REQUIRE(ans_ix && out && err_flag, MMNAS_E_ARG, "vqa_answer_targets: null pointer");
  if (B == 0) return MMNAS_OK;
  MMNAS_LAUNCH(vqa_answer_targets_kernel, dim3(cdiv(B, 4)), dim3(256), 0, (hipStream_t)stream, ans_ix, B, n, A, out, err_flag);
  return check_launch("vqa_answer_targets");
}

extern "C" int mmnas_vqa_soft_accuracy(const float* logits, long ld_logits, const float* target, long ld_target, int B, int A,
                                       float* per_row, float* out, int* nan_flag, void* stream) {
  MMNAS_REQUIRE(B >= 1 && A >= 1 && ld_logits >= A && ld_target >= A, MMNAS_E_SHAPE,
                "vqa_soft_accuracy: B=%d A=%d ld %ld / %ld (B >= 1, 1 <= A <= ld)", B, A, ld_logits, ld_target);
  MMNAS_REQUIRE(logits && target && out && nan_flag, MMNAS_E_ARG, "vqa_soft_accuracy: null pointer");
  MMNAS_LAUNCH(vqa_soft_accuracy_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, logits, ld_logits, target, ld_target, B, A, per_row,
               out, nan_flag);
  return check_launch("vqa_soft_accuracy");
}
