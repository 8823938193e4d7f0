// The grounding head behind attfc_y (full_vgd.py:105-114; hygr_vgd.py carries the same lines) as one native call per direction;
// ops.GroundingHeadFn drives these:
//   xy = LayerNorm(x_pooled[:, None, :] + y)      modules.py:44-56: unbiased std, eps added to the std
//   scores = proj_scores(xy)[..., 0]  (+ log_softmax over the regions in 'kld' mode);   reg = proj_reg(xy)
//   * mmnas_vgd_head_fwd -- one workgroup per sample, one wave per region row: the row is read once (16-byte loads), normalised
//     in registers and dotted with the five projection rows; no [B,S,F] tensor is written.  The sample's S scores meet in LDS,
//     where the same workgroup takes their log_softmax.
//   * mmnas_vgd_head_bwd -- workgroups of VH_ROWS region rows of one sample.  The normalised row is recomputed from the saved
//     input and the two saved statistics per row.  With dp = (dscore behind the log_softmax, dreg) the five sums
//         A_k[j] = sum_rows dp_k * xhat_j        and        D_k = sum_rows dp_k
//     carry every parameter gradient:  dW_k = a * A_k + b * D_k,  da = sum_k W_k * A_k,  db = sum_k W_k * D_k,  dbias_k = D_k.
//     Each workgroup leaves its A_k, D_k and its share of dxp = sum_s dyf in the workspace; a second (small) launch of the same
//     call adds the partials in a fixed order and forms the gradients.  No floating-point atomics: the same inputs give the
//     same bits on every call.

#include "common.h"
#include "ln_rows.h"

namespace mmnas {

// forward workgroup: 16 waves (one row each per sweep, the S <= 1024 scores one per thread); 8 waves above F = 1024, where a
// row's registers need the larger budget (two scores per thread)
__host__ __device__ constexpr int vh_fwd_threads(int NV) { return NV <= 4 ? 1024 : 512; }
constexpr int VH_BWD_THREADS = 256;
constexpr int VH_BWD_WAVES = VH_BWD_THREADS / 64;
constexpr int VH_ROWS = 16;            // region rows of one backward workgroup
constexpr int VH_MAX_S = 1024, VH_MIN_F = 8, VH_MAX_F = 2048;
constexpr int VH_PART = 6;             // partial rows per backward workgroup: A_0 .. A_4, dxp share
constexpr int VH_RED_THREADS = 1024;   // reduction: 16 columns x 64 slices

static inline int vh_groups(int S) { return cdiv(S, VH_ROWS); }

__device__ __forceinline__ float sum4(float4 v) { return (v.x + v.y) + (v.z + v.w); }
__device__ __forceinline__ float dot4(float4 a, float4 b) { return (a.x * b.x + a.y * b.y) + (a.z * b.z + a.w * b.w); }
__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void fma4(float4& acc, float s, float4 v) {
  acc.x += s * v.x; acc.y += s * v.y; acc.z += s * v.z; acc.w += s * v.w;
}

// ------------------------------------------------------------------------------------------
// forward: grid B, lane l of a wave holds columns (l + 64 i) * 4 .. + 3, i < NV
// ------------------------------------------------------------------------------------------
template <int NV>
__global__ void __launch_bounds__(vh_fwd_threads(NV)) vgd_head_fwd_kernel(
    const float* __restrict__ yf, const float* __restrict__ xp, const float* __restrict__ a, const float* __restrict__ b,
    const float* __restrict__ Ws, const float* __restrict__ bs, const float* __restrict__ Wr, const float* __restrict__ br,
    float* __restrict__ scores, float* __restrict__ reg, float* __restrict__ mean_out, float* __restrict__ rstd_out, int S, int F,
    float eps, int logsm) {
  constexpr int THREADS = vh_fwd_threads(NV), WAVES = THREADS / 64, PER = VH_MAX_S / THREADS;
  __shared__ float sc[VH_MAX_S];
  __shared__ float red[WAVES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const size_t sample = blockIdx.x;
  float4 xv[NV];   // the pooled language row: the same for every region of the sample
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = (lane + 64 * i) * 4;
    xv[i] = (c < F) ? ld4(xp + sample * F + c) : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  for (int s = wave; s < S; s += WAVES) {
    const size_t row = sample * S + s;
    const float* yr = yf + row * F;
    float4 v[NV];
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int c = (lane + 64 * i) * 4;
      v[i] = (c < F) ? ld4(yr + c) : make_float4(0.f, 0.f, 0.f, 0.f);
      v[i].x += xv[i].x; v[i].y += xv[i].y; v[i].z += xv[i].z; v[i].w += xv[i].w;
      sum += sum4(v[i]);
    }
    const float mean = wave_sum(sum) / (float)F;
    float ss = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int c = (lane + 64 * i) * 4;
      if (c < F) {
        v[i].x -= mean; v[i].y -= mean; v[i].z -= mean; v[i].w -= mean;
        ss += dot4(v[i], v[i]);
      }
    }
    const float sd = sqrtf(wave_sum(ss) / (float)(F - 1));
    const float inv = 1.0f / (sd + eps);
    float p0 = 0.f, p1 = 0.f, p2 = 0.f, p3 = 0.f, p4 = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int c = (lane + 64 * i) * 4;
      if (c < F) {
        const float4 av = ld4(a + c), bv = ld4(b + c);
        float4 n;   // the normalised row, as ln_fwd_kernel forms it
        n.x = av.x * v[i].x * inv + bv.x; n.y = av.y * v[i].y * inv + bv.y;
        n.z = av.z * v[i].z * inv + bv.z; n.w = av.w * v[i].w * inv + bv.w;
        p0 += dot4(n, ld4(Ws + c));
        p1 += dot4(n, ld4(Wr + c));
        p2 += dot4(n, ld4(Wr + (size_t)F + c));
        p3 += dot4(n, ld4(Wr + 2 * (size_t)F + c));
        p4 += dot4(n, ld4(Wr + 3 * (size_t)F + c));
      }
    }
    p0 = wave_sum(p0); p1 = wave_sum(p1); p2 = wave_sum(p2); p3 = wave_sum(p3); p4 = wave_sum(p4);
    if (lane == 0) {
      sc[s] = p0 + bs[0];
      *reinterpret_cast<float4*>(reg + row * 4) = make_float4(p1 + br[0], p2 + br[1], p3 + br[2], p4 + br[3]);
      if (mean_out) {
        mean_out[row] = mean;
        rstd_out[row] = inv;
      }
    }
  }
  __syncthreads();
  float x[PER];
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    const int t = threadIdx.x + j * THREADS;
    x[j] = t < S ? sc[t] : -__builtin_inff();
  }
  if (!logsm) {
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      const int t = threadIdx.x + j * THREADS;
      if (t < S) scores[sample * S + t] = x[j];
    }
    return;
  }
  // log_softmax over the S scores (torch: x - max - log(sum(exp(x - max)))); every thread adds the waves' values in one order
  float m = x[0];
#pragma unroll
  for (int j = 1; j < PER; ++j) m = fmaxf(m, x[j]);
  m = wave_max(m);
  if (lane == 0) red[wave] = m;
  __syncthreads();
  m = red[0];
#pragma unroll
  for (int j = 1; j < WAVES; ++j) m = fmaxf(m, red[j]);
  __syncthreads();
  float e = 0.f;
#pragma unroll
  for (int j = 0; j < PER; ++j) e += (threadIdx.x + j * THREADS < S) ? expf(x[j] - m) : 0.f;
  e = wave_sum(e);
  if (lane == 0) red[wave] = e;
  __syncthreads();
  float tot = 0.f;
#pragma unroll
  for (int j = 0; j < WAVES; ++j) tot += red[j];
  const float lt = logf(tot);
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    const int t = threadIdx.x + j * THREADS;
    if (t < S) scores[sample * S + t] = (x[j] - m) - lt;
  }
}

// ------------------------------------------------------------------------------------------
// backward: grid (groups of VH_ROWS rows, B); part [B * G][VH_PART][F], dpart [B * G][8]
// dx of the LayerNorm: (g - mean(g)) / s - c * sum(g c) / ((F-1) sd s^2),  g = dn * a,  c = x - mean,  s = sd + eps  (rowops.hip)
// ------------------------------------------------------------------------------------------
template <int NV>
__global__ void __launch_bounds__(VH_BWD_THREADS) vgd_head_bwd_kernel(
    const float* __restrict__ dscores, const float* __restrict__ dreg, const float* __restrict__ yf, const float* __restrict__ xp,
    const float* __restrict__ a, const float* __restrict__ Ws, const float* __restrict__ Wr, const float* __restrict__ scores,
    const float* __restrict__ mean_in, const float* __restrict__ rstd_in, float* __restrict__ dyf, float* __restrict__ part,
    float* __restrict__ dpart, int S, int F, float eps, int logsm) {
  __shared__ __attribute__((aligned(16))) float red[VH_PART][VH_BWD_WAVES][64 * 4];   // [which][wave][lane * 4 + j], reused per i
  __shared__ float tsum[VH_BWD_WAVES];
  __shared__ float dsum[VH_BWD_WAVES][8];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const size_t sample = blockIdx.y;
  const int G = gridDim.x;
  const size_t wg = sample * G + blockIdx.x;
  // log_softmax backward: ds = dscores - exp(scores) * sum_s dscores; the sum over the sample's S regions, one order for all
  float T = 0.f;
  if (logsm) {
    float t = 0.f;
    for (int s = threadIdx.x; s < S; s += VH_BWD_THREADS) t += dscores[sample * S + s];
    t = wave_sum(t);
    if (lane == 0) tsum[wave] = t;
    __syncthreads();
    T = (tsum[0] + tsum[1]) + (tsum[2] + tsum[3]);
  }
  float4 A0[NV], A1[NV], A2[NV], A3[NV], A4[NV], AX[NV], xv[NV], av[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = (lane + 64 * i) * 4;
    A0[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    A1[i] = A0[i]; A2[i] = A0[i]; A3[i] = A0[i]; A4[i] = A0[i]; AX[i] = A0[i];
    xv[i] = (c < F) ? ld4(xp + sample * F + c) : A0[i];
    av[i] = (c < F) ? ld4(a + c) : A0[i];
  }
  float D0 = 0.f, D1 = 0.f, D2 = 0.f, D3 = 0.f, D4 = 0.f;
  const int s0 = blockIdx.x * VH_ROWS;
  const int s1 = min(S, s0 + VH_ROWS);
  for (int s = s0 + wave; s < s1; s += VH_BWD_WAVES) {
    const size_t row = sample * S + s;
    float d0 = dscores[row];
    if (logsm) d0 -= expf(scores[row]) * T;
    const float4 dr = ld4(dreg + row * 4);
    const float mean = mean_in[row], inv = rstd_in[row];
    const float sden = 1.0f / inv, sd = sden - eps;
    const float* yr = yf + row * F;
    float4 cv[NV], g[NV];
    float sg = 0.f, sgc = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int c = (lane + 64 * i) * 4;
      if (c < F) {
        const float4 y = ld4(yr + c);
        cv[i].x = (xv[i].x + y.x) - mean; cv[i].y = (xv[i].y + y.y) - mean;
        cv[i].z = (xv[i].z + y.z) - mean; cv[i].w = (xv[i].w + y.w) - mean;
        const float4 w0 = ld4(Ws + c), w1 = ld4(Wr + c), w2 = ld4(Wr + (size_t)F + c), w3 = ld4(Wr + 2 * (size_t)F + c),
                     w4 = ld4(Wr + 3 * (size_t)F + c);
        // gradient wrt the normalised row, times a
        g[i].x = (d0 * w0.x + dr.x * w1.x + dr.y * w2.x + dr.z * w3.x + dr.w * w4.x) * av[i].x;
        g[i].y = (d0 * w0.y + dr.x * w1.y + dr.y * w2.y + dr.z * w3.y + dr.w * w4.y) * av[i].y;
        g[i].z = (d0 * w0.z + dr.x * w1.z + dr.y * w2.z + dr.z * w3.z + dr.w * w4.z) * av[i].z;
        g[i].w = (d0 * w0.w + dr.x * w1.w + dr.y * w2.w + dr.z * w3.w + dr.w * w4.w) * av[i].w;
        sg += sum4(g[i]);
        sgc += dot4(g[i], cv[i]);
      } else {
        cv[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        g[i] = cv[i];
      }
    }
    sg = wave_sum(sg); sgc = wave_sum(sgc);
    const float mg = sg / (float)F;
    // sd is recovered from 1 / (sd + eps), so it is not exactly 0 on a constant row.  That needs no flag from the forward:
    // there cv == 0 exactly, so sgc == 0 and the term is 0 whichever way ln_bwd_k2 decides.  A row whose recovered sd is not
    // above 0 although its sd is (an estimate: sd within a few units in the last place of eps, ~1e-13) loses a term that is
    // at most sd / (sd + eps), about 2e-7, of the first one.
    const float k2 = ln_bwd_k2(sgc, (float)(F - 1), 1.0f / (float)(F - 1), sd, sden, inv);
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int c = (lane + 64 * i) * 4;
      if (c < F) {
        float4 o;
        o.x = (g[i].x - mg) * inv - cv[i].x * k2; o.y = (g[i].y - mg) * inv - cv[i].y * k2;
        o.z = (g[i].z - mg) * inv - cv[i].z * k2; o.w = (g[i].w - mg) * inv - cv[i].w * k2;
        *reinterpret_cast<float4*>(dyf + row * F + c) = o;
        AX[i].x += o.x; AX[i].y += o.y; AX[i].z += o.z; AX[i].w += o.w;
        const float4 xh = make_float4(cv[i].x * inv, cv[i].y * inv, cv[i].z * inv, cv[i].w * inv);
        fma4(A0[i], d0, xh); fma4(A1[i], dr.x, xh); fma4(A2[i], dr.y, xh); fma4(A3[i], dr.z, xh); fma4(A4[i], dr.w, xh);
      }
    }
    D0 += d0; D1 += dr.x; D2 += dr.y; D3 += dr.z; D4 += dr.w;
  }
  // the waves' partial rows meet in LDS as 16-byte rows (ln_bwd_kernel's scheme); wave w adds rows w and w + 4 of the six
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = (lane + 64 * i) * 4;
    __syncthreads();
    *reinterpret_cast<float4*>(&red[0][wave][lane * 4]) = A0[i];
    *reinterpret_cast<float4*>(&red[1][wave][lane * 4]) = A1[i];
    *reinterpret_cast<float4*>(&red[2][wave][lane * 4]) = A2[i];
    *reinterpret_cast<float4*>(&red[3][wave][lane * 4]) = A3[i];
    *reinterpret_cast<float4*>(&red[4][wave][lane * 4]) = A4[i];
    *reinterpret_cast<float4*>(&red[5][wave][lane * 4]) = AX[i];
    __syncthreads();
    for (int which = wave; which < VH_PART; which += VH_BWD_WAVES) {
      if (c < F) {
        const f32x4 q0 = *reinterpret_cast<const f32x4*>(&red[which][0][lane * 4]);
        const f32x4 q1 = *reinterpret_cast<const f32x4*>(&red[which][1][lane * 4]);
        const f32x4 q2 = *reinterpret_cast<const f32x4*>(&red[which][2][lane * 4]);
        const f32x4 q3 = *reinterpret_cast<const f32x4*>(&red[which][3][lane * 4]);
        *reinterpret_cast<f32x4*>(part + (wg * VH_PART + which) * F + c) = (q0 + q1) + (q2 + q3);
      }
    }
  }
  if (lane == 0) {
    dsum[wave][0] = D0; dsum[wave][1] = D1; dsum[wave][2] = D2; dsum[wave][3] = D3; dsum[wave][4] = D4;
  }
  __syncthreads();
  if (threadIdx.x < 8) {
    const int k = threadIdx.x;
    dpart[wg * 8 + k] = k < 5 ? (dsum[0][k] + dsum[1][k]) + (dsum[2][k] + dsum[3][k]) : 0.f;
  }
}

// The fixed-order sums over the workgroups' partials.  grid (ceil(F / 16), 1 + B), block = 16 columns x 64 slices.
//   y == 0:  A_k = sum over all P = B * G partials, D_k likewise -> dWs, dWr, dln_a, dln_b (columns of this block), dbs, dbr
//   y == 1 + b:  dxp[b] = sum over the G partials of sample b (G <= 64: one per slice)
__global__ void __launch_bounds__(VH_RED_THREADS) vgd_head_bwd_reduce_kernel(
    const float* __restrict__ part, const float* __restrict__ dpart, const float* __restrict__ a, const float* __restrict__ b,
    const float* __restrict__ Ws, const float* __restrict__ Wr, float* __restrict__ dxp, float* __restrict__ da,
    float* __restrict__ db, float* __restrict__ dWs, float* __restrict__ dbs, float* __restrict__ dWr, float* __restrict__ dbr,
    int P, int G, int F) {
  __shared__ float red[5][64][17];
  __shared__ float dred[5][VH_RED_THREADS / 64];
  const int cl = threadIdx.x & 15, sl = threadIdx.x >> 4;
  const int c = blockIdx.x * 16 + cl;
  if (blockIdx.y > 0) {
    const size_t sample = blockIdx.y - 1;
    red[0][sl][cl] = (c < F && sl < G) ? part[((sample * G + sl) * VH_PART + 5) * F + c] : 0.f;
    __syncthreads();
    if (sl == 0 && c < F) {
      float t = 0.f;
      for (int i = 0; i < G; ++i) t += red[0][i][cl];
      dxp[sample * F + c] = t;
    }
    return;
  }
  float acc[5] = {0.f, 0.f, 0.f, 0.f, 0.f}, d[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
  if (c < F) {
    for (size_t p = sl; p < (size_t)P; p += 64) {
#pragma unroll
      for (int k = 0; k < 5; ++k) acc[k] += part[(p * VH_PART + k) * F + c];
    }
  }
  for (size_t p = threadIdx.x; p < (size_t)P; p += VH_RED_THREADS) {
#pragma unroll
    for (int k = 0; k < 5; ++k) d[k] += dpart[p * 8 + k];
  }
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    red[k][sl][cl] = acc[k];
    d[k] = wave_sum(d[k]);
    if ((threadIdx.x & 63) == 0) dred[k][threadIdx.x >> 6] = d[k];
  }
  __syncthreads();
  if (sl != 0) return;
  float D[5];
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    float t = 0.f;
#pragma unroll
    for (int j = 0; j < VH_RED_THREADS / 64; ++j) t += dred[k][j];
    D[k] = t;
  }
  if (blockIdx.x == 0 && cl == 0) {
    dbs[0] = D[0];
    dbr[0] = D[1]; dbr[1] = D[2]; dbr[2] = D[3]; dbr[3] = D[4];
  }
  if (c >= F) return;
  float A[5];
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    float t = 0.f;
#pragma unroll 8
    for (int i = 0; i < 64; ++i) t += red[k][i][cl];
    A[k] = t;
  }
  const float ac = a[c], bc = b[c];
  float ga = 0.f, gb = 0.f;
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    const float w = k == 0 ? Ws[c] : Wr[(size_t)(k - 1) * F + c];
    ga += w * A[k];
    gb += w * D[k];
    (k == 0 ? dWs : dWr + (size_t)(k - 1) * F)[c] = ac * A[k] + bc * D[k];
  }
  da[c] = ga;
  db[c] = gb;
}

}  // namespace mmnas

using namespace mmnas;

static bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

extern "C" int mmnas_vgd_head_supported(int S, int F) {
  return S >= 1 && S <= VH_MAX_S && F >= VH_MIN_F && F <= VH_MAX_F && F % 4 == 0;
}

extern "C" size_t mmnas_vgd_head_bwd_ws_floats(int B, int S, int F) {
  if (B < 1 || !mmnas_vgd_head_supported(S, F)) return 0;
  return (size_t)B * vh_groups(S) * ((size_t)VH_PART * F + 8);
}

static int vh_check(const char* what, int B, int S, int F) {
  MMNAS_REQUIRE(mmnas_vgd_head_supported(S, F), MMNAS_E_SHAPE, "%s: S=%d F=%d (1 <= S <= %d, %d <= F <= %d, F %% 4 == 0)", what, S, F,
                VH_MAX_S, VH_MIN_F, VH_MAX_F);
  MMNAS_REQUIRE(B >= 1 && B <= 32768, MMNAS_E_SHAPE, "%s: B=%d (1 <= B <= 32768)", what, B);
  return MMNAS_OK;
}

extern "C" int mmnas_vgd_head_fwd(const float* yf, const float* xp, const float* ln_a, const float* ln_b, const float* Ws,
                                  const float* bs, const float* Wr, const float* br, float* scores, float* reg, float* mean,
                                  float* rstd, int B, int S, int F, float eps, int log_softmax, void* stream) {
  if (int rc = vh_check("vgd_head_fwd", B, S, F)) return rc;
  MMNAS_REQUIRE(yf && xp && ln_a && ln_b && Ws && bs && Wr && br && scores && reg, MMNAS_E_ARG, "vgd_head_fwd: null pointer");
  MMNAS_REQUIRE((mean == nullptr) == (rstd == nullptr), MMNAS_E_ARG, "vgd_head_fwd: mean and rstd are given together or not at all");
  MMNAS_REQUIRE(aligned16(yf) && aligned16(xp) && aligned16(ln_a) && aligned16(ln_b) && aligned16(Ws) && aligned16(Wr) && aligned16(reg),
                MMNAS_E_ARG, "vgd_head_fwd: yf, xp, ln_a, ln_b, Ws, Wr and reg must be 16-byte aligned");
  const int nv = cdiv(F, 256);
#define VHF(NV)                                                                                                                \
  MMNAS_LAUNCH(vgd_head_fwd_kernel<NV>, dim3(B), dim3(vh_fwd_threads(NV)), 0, (hipStream_t)stream, yf, xp, ln_a, ln_b, Ws, bs, Wr, br, \
               scores, reg, mean, rstd, S, F, eps, log_softmax ? 1 : 0)
  if (nv <= 1) VHF(1);
  else if (nv <= 2) VHF(2);
  else if (nv <= 4) VHF(4);
  else VHF(8);
#undef VHF
  return check_launch("vgd_head_fwd");
}

extern "C" int mmnas_vgd_head_bwd(const float* dscores, const float* dreg, const float* yf, const float* xp, const float* ln_a,
                                  const float* ln_b, const float* Ws, const float* Wr, const float* scores, const float* mean,
                                  const float* rstd, float* dyf, float* dxp, float* dln_a, float* dln_b, float* dWs, float* dbs,
                                  float* dWr, float* dbr, float* ws, int B, int S, int F, float eps, int log_softmax, void* stream) {
  if (int rc = vh_check("vgd_head_bwd", B, S, F)) return rc;
  MMNAS_REQUIRE(dscores && dreg && yf && xp && ln_a && ln_b && Ws && Wr && mean && rstd && dyf && dxp && dln_a && dln_b && dWs && dbs &&
                    dWr && dbr && ws && (scores || !log_softmax),
                MMNAS_E_ARG, "vgd_head_bwd: null pointer");
  MMNAS_REQUIRE(aligned16(dreg) && aligned16(yf) && aligned16(xp) && aligned16(ln_a) && aligned16(Ws) && aligned16(Wr) && aligned16(dyf) &&
                    aligned16(ws),
                MMNAS_E_ARG, "vgd_head_bwd: dreg, yf, xp, ln_a, Ws, Wr, dyf and ws must be 16-byte aligned");
  const int G = vh_groups(S), P = B * G;
  float* part = ws;
  float* dpart = ws + (size_t)P * VH_PART * F;
  const int nv = cdiv(F, 256);
#define VHB(NV)                                                                                                                  \
  MMNAS_LAUNCH(vgd_head_bwd_kernel<NV>, dim3(G, B), dim3(VH_BWD_THREADS), 0, (hipStream_t)stream, dscores, dreg, yf, xp, ln_a, Ws, \
               Wr, scores, mean, rstd, dyf, part, dpart, S, F, eps, log_softmax ? 1 : 0)
  if (nv <= 1) VHB(1);
  else if (nv <= 2) VHB(2);
  else if (nv <= 4) VHB(4);
  else VHB(8);
#undef VHB
  if (int rc = check_launch("vgd_head_bwd")) return rc;
  MMNAS_LAUNCH(vgd_head_bwd_reduce_kernel, dim3(cdiv(F, 16), 1 + B), dim3(VH_RED_THREADS), 0, (hipStream_t)stream, part, dpart, ln_a,
               ln_b, Ws, Wr, dxp, dln_a, dln_b, dWs, dbs, dWr, dbr, P, G, F);
  return check_launch("vgd_head_bwd (reduction)");
}
