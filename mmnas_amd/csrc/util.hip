// Error plumbing, ABI version, the runtime switches (switches.h), and the small utility kernels of the C ABI:
// dropout-mask materialisation (tests / mask replay), segment pack/unpack for the data-parallel
// gradient exchange, fused Adam / SGD and sum-of-squares for the optimizer step.
#include <stdarg.h>
#include <stdlib.h>
#include <string.h>
#include <mutex>
#include <vector>
#include <algorithm>
#include "common.h"
#include "switches.h"

namespace mmnas {

static thread_local char g_err[512] = "";

void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

int check_launch(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_error("%s: launch failed: %s", what, hipGetErrorString(e));
    return MMNAS_E_LAUNCH;
  }
  return MMNAS_OK;
}

// ---- runtime switches: the definitions of switches.h's table ----
int env_int(const char* name, int dflt) {
  const char* e = getenv(name);
  return e && e[0] ? atoi(e) : dflt;
}

namespace sw {
#define MMNAS_SW_DEFINE(id, var, dflt, kind, policy, help) Switch id = {var, dflt, sw_##kind, sw_##policy, "[" #kind ", " #policy "] " help, 0, 0};
MMNAS_SWITCHES(MMNAS_SW_DEFINE)
#undef MMNAS_SW_DEFINE
}  // namespace sw

#define MMNAS_SW_ADDRESS(id, var, dflt, kind, policy, help) &sw::id,
static Switch* const g_switches[] = {MMNAS_SWITCHES(MMNAS_SW_ADDRESS)};
#undef MMNAS_SW_ADDRESS
constexpr int N_SWITCHES = (int)(sizeof(g_switches) / sizeof(g_switches[0]));

// what the environment says now; *from_env: the variable, not the default, decided
static int sw_parse(const Switch& s, bool* from_env) {
  const char* e = getenv(s.name);
  *from_env = s.kind == sw_presence ? e != nullptr : (e && e[0]);
  switch (s.kind) {
    case sw_presence: case sw_string: return *from_env ? 1 : 0;
    case sw_exact1: return e && e[0] == '1';
    case sw_bool: return (*from_env ? atoi(e) : s.dflt) != 0;
    default: return *from_env ? atoi(e) : s.dflt;
  }
}

int Switch::read() {
  bool from_env;
  const int v = sw_parse(*this, &from_env);
  if (policy != sw_every_call) { value = v; state = from_env ? 2 : 1; }
  return v;
}

int Switch::reload() {
  state = 0;
  return read();
}

int Switch::set(int v) {
  const int prev = get();
  value = v;
  state = 3;
  return prev;
}

int Switch::peek(int* source) const {
  if (state) { *source = state - 1; return value; }
  bool from_env;
  const int v = sw_parse(*this, &from_env);
  *source = (from_env ? MMNAS_SWITCH_ENV : MMNAS_SWITCH_DEFAULT) | (policy == sw_every_call ? 0 : MMNAS_SWITCH_UNREAD);
  return v;
}

// ---- optional per-kernel-class timing with HIP events on the launch stream (bench.py roofline) ----
namespace prof {
struct Rec { hipEvent_t a, b; int kind; double flops, bytes; char tag[96]; };
static std::mutex mu;
static bool enabled = false;
static std::vector<Rec> recs;
static std::vector<hipEvent_t> pool;
static size_t pool_next = 0;

static hipEvent_t get_event() {
  if (pool_next == pool.size()) {
    hipEvent_t e = nullptr;
    if (hipEventCreate(&e) != hipSuccess) e = nullptr;   // (a null event makes the launch carry no timestamp)
    pool.push_back(e);
  }
  return pool[pool_next++];
}
}  // namespace prof

bool prof_enabled() { return prof::enabled; }

double decimal_of(float x) {
  char buf[40];
  for (int digits = 1; digits <= 9; ++digits) {
    snprintf(buf, sizeof(buf), "%.*g", digits, (double)x);
    if (strtof(buf, nullptr) == x) break;
  }
  return strtod(buf, nullptr);
}

AdamCoef adam_coef(float beta1, float beta2, int step) {
  const double b1 = decimal_of(beta1), b2 = decimal_of(beta2);
  AdamCoef k;
  k.c1 = (float)(1.0 - pow(b1, (double)step));
  k.c2s = (float)sqrt(1.0 - pow(b2, (double)step));
  k.omb1 = (float)(1.0 - b1);
  k.omb2 = (float)(1.0 - b2);
  return k;
}

struct ActiveScope { long idx; bool started; };
static thread_local ActiveScope g_active = {-1, false};

ProfScope::ProfScope(int kind, double flops, double bytes, hipStream_t st, const char* tag) : idx_(-1), st_(st) {
  if (!prof::enabled || g_active.idx >= 0) return;  // (scopes do not nest: the outer one keeps the launches)
  std::lock_guard<std::mutex> g(prof::mu);
  prof::Rec r;
  r.a = prof::get_event(); r.b = prof::get_event(); r.kind = kind; r.flops = flops; r.bytes = bytes;
  r.tag[0] = 0;
  if (tag) { strncpy(r.tag, tag, sizeof(r.tag) - 1); r.tag[sizeof(r.tag) - 1] = 0; }
  idx_ = (long)prof::recs.size();
  prof::recs.push_back(r);
  g_active.idx = idx_;
  g_active.started = false;
}

ProfScope::~ProfScope() {
  if (idx_ < 0) return;
  if (!g_active.started) {  // no kernel was launched inside the scope: drop the record
    std::lock_guard<std::mutex> g(prof::mu);
    prof::recs[idx_].kind = -1;
  }
  g_active.idx = -1;
}

ProfEvents prof_launch_events() {
  ProfEvents e = {nullptr, nullptr};
  if (g_active.idx < 0) return e;
  std::lock_guard<std::mutex> g(prof::mu);
  const prof::Rec& r = prof::recs[g_active.idx];
  e.start = g_active.started ? nullptr : r.a;
  e.stop = r.b;
  g_active.started = true;
  return e;
}

__global__ void dropout_mask_kernel(float* out, size_t n, DropCfg c) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    out[i] = c.thresh ? drop_mult(c, (uint32_t)i) : 1.0f;
}

// Gather / scatter of gradient segments (DDP's bucket copies).  One 1-D grid over all segments: segment sizes differ by
// 100x (a candidate's 1 MB of weights beside the 24 MB embedding table), so the work is cut into equal pieces of
// PACK_PIECE floats and each workgroup takes pieces round-robin; a piece never crosses a segment (pieces are counted per
// segment).  (Round 2 launched 64 workgroups per segment: the largest segment set the kernel's duration, 50 us for a
// 24 MB bucket.)
constexpr int PACK_PIECE = 8192;   // floats per piece: 8 float4 per thread
__device__ __forceinline__ void pack_piece(const mmnas_segment s, float* staging, size_t piece, float scale, int direction) {
  float* stg = staging + s.offset;
  const size_t lo = piece * PACK_PIECE, hi = lo + PACK_PIECE < s.n ? lo + PACK_PIECE : s.n;
  if ((((uintptr_t)s.ptr | (uintptr_t)stg) & 15) == 0) {
    float4* p4 = reinterpret_cast<float4*>(s.ptr);
    float4* s4 = reinterpret_cast<float4*>(stg);
    const size_t l4 = lo >> 2, h4 = hi >> 2;
    float4 v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {   // all loads of the piece in flight before the first store
      const size_t i = l4 + threadIdx.x + 256 * k;
      if (i < h4) v[k] = direction == 0 ? p4[i] : s4[i];
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const size_t i = l4 + threadIdx.x + 256 * k;
      if (i < h4) {
        float4 w = v[k];
        w.x *= scale; w.y *= scale; w.z *= scale; w.w *= scale;
        if (direction == 0) s4[i] = w; else p4[i] = w;
      }
    }
    for (size_t i = (h4 << 2) + threadIdx.x; i < hi; i += 256) {
      if (direction == 0) stg[i] = s.ptr[i] * scale; else s.ptr[i] = stg[i] * scale;
    }
  } else {
    for (size_t i = lo + threadIdx.x; i < hi; i += 256) {
      if (direction == 0) stg[i] = s.ptr[i] * scale; else s.ptr[i] = stg[i] * scale;
    }
  }
}

// piece q of the whole table -> (segment, piece inside it); nseg <= 96: a linear walk of per-segment piece counts
template <typename Table>
__device__ __forceinline__ void pack_body(const Table& segs, int nseg, size_t npieces, float* staging, float scale, int direction) {
  if (npieces == 0)   // (table on the device: the launcher could not count)
    for (int k = 0; k < nseg; ++k) npieces += (segs[k].n + PACK_PIECE - 1) / PACK_PIECE;
  for (size_t q = blockIdx.x; q < npieces; q += gridDim.x) {
    size_t rest = q;
    int k = 0;
    for (; k < nseg; ++k) {
      const size_t np = (segs[k].n + PACK_PIECE - 1) / PACK_PIECE;
      if (rest < np) break;
      rest -= np;
    }
    if (k < nseg) pack_piece(segs[k], staging, rest, scale, direction);
  }
}

__global__ void pack_kernel(const mmnas_segment* segs, int nseg, size_t npieces, float* staging, float scale, int direction) {
  pack_body(segs, nseg, npieces, staging, scale, direction);
}

struct PackArgs { mmnas_segment s[96]; };
__global__ void pack_args_kernel(PackArgs a, int nseg, size_t npieces, float* staging, float scale, int direction) {
  pack_body(a.s, nseg, npieces, staging, scale, direction);
}

// omb1 / omb2 = 1 - beta, c1 / c2: all four formed on the host (adam_coef)
__global__ void adam_kernel(float* p, const float* g, float* m, float* v, size_t n, float lr, float b1,
                            float b2, float omb1, float omb2, float eps, float wd, const float* sumsq, float max_norm, float c1,
                            float c2) {
  float gscale = 1.f;
  if (sumsq) gscale = fminf(1.f, max_norm / (sqrtf(*sumsq) + 1e-6f));
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    float gi = g[i] * gscale;
    float pi = p[i];
    if (wd != 0.f) gi += wd * pi;
    const float mi = b1 * m[i] + omb1 * gi;
    const float vi = b2 * v[i] + omb2 * gi * gi;
    m[i] = mi; v[i] = vi;
    // torch.optim.Adam: denom = sqrt(v)/sqrt(1-b2^t) + eps ; p -= lr/(1-b1^t) * m/denom
    p[i] = pi - (lr / c1) * mi / (sqrtf(vi) / c2 + eps);
  }
}

// the same arithmetic on four consecutive elements per thread and pass: 16-byte loads / stores (the scalar form moved
// 4 bytes per lane and instruction: 0.45 ms for the supernet's 37 M parameters where 1.04 GB of traffic is 0.21 ms at 5 TB/s)
__device__ __forceinline__ void adam_one(float& pi, float gi, float& mi, float& vi, float gscale, float lr, float b1, float b2,
                                         float omb1, float omb2, float eps, float wd, float c1, float c2) {
  gi *= gscale;
  if (wd != 0.f) gi += wd * pi;
  mi = b1 * mi + omb1 * gi;
  vi = b2 * vi + omb2 * gi * gi;
  pi = pi - (lr / c1) * mi / (sqrtf(vi) / c2 + eps);
}
__global__ void __launch_bounds__(256) adam4_kernel(float4* __restrict__ p, const float4* __restrict__ g, float4* __restrict__ m,
                                                    float4* __restrict__ v, size_t n4, float lr, float b1, float b2, float omb1,
                                                    float omb2, float eps, float wd, const float* sumsq, float max_norm, float c1,
                                                    float c2) {
  float gscale = 1.f;
  if (sumsq) gscale = fminf(1.f, max_norm / (sqrtf(*sumsq) + 1e-6f));
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
    float4 pi = p[i], mi = m[i], vi = v[i];
    const float4 gi = g[i];
    adam_one(pi.x, gi.x, mi.x, vi.x, gscale, lr, b1, b2, omb1, omb2, eps, wd, c1, c2);
    adam_one(pi.y, gi.y, mi.y, vi.y, gscale, lr, b1, b2, omb1, omb2, eps, wd, c1, c2);
    adam_one(pi.z, gi.z, mi.z, vi.z, gscale, lr, b1, b2, omb1, omb2, eps, wd, c1, c2);
    adam_one(pi.w, gi.w, mi.w, vi.w, gscale, lr, b1, b2, omb1, omb2, eps, wd, c1, c2);
    m[i] = mi; v[i] = vi; p[i] = pi;
  }
}
// torch.optim.SGD (momentum, dampening, nesterov, weight decay) with the clip scale read from the device scalar, in
// torch's order of operations.  `first`: the momentum buffer does not exist yet -- torch's first step sets buf = g'
// (no dampening).  MOM == false neither reads nor writes buf.
template <bool MOM>
__device__ __forceinline__ void sgd_one(float& pi, float gi, float& bi, float gscale, float lr, float mom, float damp, float wd,
                                        bool nesterov, bool first) {
  // (explicit fmaf: each torch statement -- add(p, alpha=wd), mul_(momentum).add_(g', alpha=1 - dampening), add_(buf, alpha=-lr) --
  //  is one rounding of a + alpha * b in ATen; written out so that contraction cannot pick another grouping)
  gi *= gscale;
  if (wd != 0.f) gi = fmaf(wd, pi, gi);
  if (MOM) {
    bi = first ? gi : fmaf(1.f - damp, gi, mom * bi);
    gi = nesterov ? fmaf(mom, bi, gi) : bi;
  }
  pi = fmaf(-lr, gi, pi);
}
template <bool MOM>
__global__ void sgd_kernel(float* p, const float* g, float* buf, size_t n, float lr, float mom, float damp, float wd, int nesterov,
                           int first, const float* sumsq, float max_norm) {
  float gscale = 1.f;
  if (sumsq) gscale = fminf(1.f, max_norm / (sqrtf(*sumsq) + 1e-6f));
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    float pi = p[i], bi = 0.f;
    if (MOM && !first) bi = buf[i];
    sgd_one<MOM>(pi, g[i], bi, gscale, lr, mom, damp, wd, nesterov != 0, first != 0);
    if (MOM) buf[i] = bi;
    p[i] = pi;
  }
}
// four consecutive elements per thread and pass, as adam4_kernel: 20 bytes of traffic per element (12 without momentum)
template <bool MOM>
__global__ void __launch_bounds__(256) sgd4_kernel(float4* __restrict__ p, const float4* __restrict__ g, float4* __restrict__ buf,
                                                   size_t n4, float lr, float mom, float damp, float wd, int nesterov, int first,
                                                   const float* sumsq, float max_norm) {
  float gscale = 1.f;
  if (sumsq) gscale = fminf(1.f, max_norm / (sqrtf(*sumsq) + 1e-6f));
  const bool nest = nesterov != 0, fst = first != 0;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
    float4 pi = p[i], bi = make_float4(0.f, 0.f, 0.f, 0.f);
    const float4 gi = g[i];
    if (MOM && !fst) bi = buf[i];
    sgd_one<MOM>(pi.x, gi.x, bi.x, gscale, lr, mom, damp, wd, nest, fst);
    sgd_one<MOM>(pi.y, gi.y, bi.y, gscale, lr, mom, damp, wd, nest, fst);
    sgd_one<MOM>(pi.z, gi.z, bi.z, gscale, lr, mom, damp, wd, nest, fst);
    sgd_one<MOM>(pi.w, gi.w, bi.w, gscale, lr, mom, damp, wd, nest, fst);
    if (MOM) buf[i] = bi;
    p[i] = pi;
  }
}
// Sum of squares in two stages: every workgroup leaves ONE partial in part[] (sumsq4_kernel over the aligned body, sumsq_kernel
// over a misaligned call or the tail), sumsq_final_kernel adds the partials in double in a fixed order and adds the total to
// *out once.  (Until round 15 every workgroup added its partial to *out with a float atomic: a chain of up to 1024 additions,
// each rounded to the running total's ulp -- 5.9e-7 relative on 1 M elements where a float32 pairwise sum stays under 6e-8 --
// and in an order that changed from run to run.)
constexpr int SUMSQ_MAX_BLOCKS = 1024;                     // per stage-one kernel; part[] holds 2 * SUMSQ_MAX_BLOCKS floats
__global__ void __launch_bounds__(256) sumsq4_kernel(const float4* __restrict__ g, size_t n4, float* __restrict__ part) {
  float s0 = 0.f, s1 = 0.f;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
    const float4 x = g[i];
    s0 += x.x * x.x + x.y * x.y; s1 += x.z * x.z + x.w * x.w;
  }
  float s = wave_sum(s0 + s1);
  __shared__ float red[4];
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ void sumsq_kernel(const float* g, size_t n, float* __restrict__ part) {
  float s = 0.f;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    s += g[i] * g[i];
  s = wave_sum(s);
  __shared__ float red[4];
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// one workgroup: out += sum of part[0 .. nparts) (nparts <= 2 * SUMSQ_MAX_BLOCKS), in double, in a fixed order
__global__ void __launch_bounds__(256) sumsq_final_kernel(const float* __restrict__ part, int nparts, float* out) {
  double s = 0.0;
  for (int i = threadIdx.x; i < nparts; i += 256) s += (double)part[i];
  __shared__ double red[256];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) atomicAdd(out, (float)red[0]);     // (atomic: the word may collect several calls, as before)
}

}  // namespace mmnas

using namespace mmnas;

extern "C" int mmnas_prof_enable(int on) {
  std::lock_guard<std::mutex> g(prof::mu);
  prof::enabled = on != 0;
  prof::recs.clear();
  prof::pool_next = 0;
  return MMNAS_OK;
}

extern "C" int mmnas_prof_collect(mmnas_prof_stat* stats) {
  MMNAS_REQUIRE(stats, MMNAS_E_ARG, "prof_collect: null output");
  std::lock_guard<std::mutex> g(prof::mu);
  for (int k = 0; k < MMNAS_K_COUNT; ++k) { stats[k].ms = 0; stats[k].flops = 0; stats[k].bytes = 0; stats[k].launches = 0; }
  // tuning aid: MMNAS_PROF_DUMP=<file> appends one "kind,tag,ms,flops,bytes" row per bracketed launch
  const char* dump = getenv(sw::prof_dump.name);
  FILE* df = dump && dump[0] ? fopen(dump, "a") : nullptr;
  for (const prof::Rec& r : prof::recs) {
    if (r.kind < 0) continue;
    if (hipEventSynchronize(r.b) != hipSuccess) continue;
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, r.a, r.b) != hipSuccess) continue;
    if (df) fprintf(df, "%d,%s,%.6f,%.0f,%.0f\n", r.kind, r.tag, ms, r.flops, r.bytes);
    mmnas_prof_stat& s = stats[r.kind];
    s.ms += ms; s.flops += r.flops; s.bytes += r.bytes; s.launches += 1;
  }
  if (df) fclose(df);
  prof::recs.clear();
  prof::pool_next = 0;
  return MMNAS_OK;
}

extern "C" int mmnas_abi_version(void) { return MMNAS_ABI_VERSION; }

extern "C" int mmnas_switch_count(void) { return N_SWITCHES; }

extern "C" int mmnas_switch_info(int i, const char** name, const char** help, int* dflt, int* value, int* source) {
  MMNAS_REQUIRE(i >= 0 && i < N_SWITCHES, MMNAS_E_ARG, "mmnas_switch_info: index %d outside 0..%d", i, N_SWITCHES - 1);
  const Switch& s = *g_switches[i];
  int src = 0;
  const int v = s.peek(&src);
  if (name) *name = s.name;
  if (help) *help = s.help;
  if (dflt) *dflt = s.dflt;
  if (value) *value = v;
  if (source) *source = src;
  return MMNAS_OK;
}
extern "C" const char* mmnas_last_error(void) { return g_err; }

extern "C" int mmnas_dropout_mask(float* out, size_t n, float p, uint64_t seed, uint32_t site, void* stream) {
  MMNAS_REQUIRE(out || n == 0, MMNAS_E_ARG, "mmnas_dropout_mask: null output");
  if (n == 0) return MMNAS_OK;
  MMNAS_REQUIRE(n < (1ull << 32), MMNAS_E_SHAPE, "mmnas_dropout_mask: n too large");
  const int blocks = (int)((n + 255) / 256 < 2048 ? (n + 255) / 256 : 2048);
  MMNAS_LAUNCH(dropout_mask_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, out, n,
                     make_drop(p, seed, site));
  return check_launch("dropout_mask");
}

static int pack_grid(size_t npieces) { return (int)(npieces < 2048 ? (npieces ? npieces : 1) : 2048); }

extern "C" int mmnas_pack_segments(const mmnas_segment* segs, int nseg, float* staging, float scale,
                                   int direction, void* stream) {
  if (nseg <= 0) return MMNAS_OK;
  MMNAS_REQUIRE(segs && staging, MMNAS_E_ARG, "mmnas_pack_segments: null pointer");
  // (the table lives on the device: the kernel counts the pieces itself)
  MMNAS_LAUNCH(pack_kernel, dim3(1024), dim3(256), 0, (hipStream_t)stream, segs, nseg, (size_t)0, staging, scale, direction);
  return check_launch("pack_segments");
}

extern "C" int mmnas_pack_segments_host(const mmnas_segment* segs_host, int nseg, float* staging, float scale,
                                        int direction, void* stream) {
  if (nseg <= 0) return MMNAS_OK;
  MMNAS_REQUIRE(segs_host && staging, MMNAS_E_ARG, "mmnas_pack_segments_host: null pointer");
  for (int base = 0; base < nseg; base += 96) {
    const int n = nseg - base < 96 ? nseg - base : 96;
    PackArgs a;
    memset(&a, 0, sizeof(a));
    memcpy(a.s, segs_host + base, (size_t)n * sizeof(mmnas_segment));
    size_t npieces = 0;
    for (int k = 0; k < n; ++k) npieces += (a.s[k].n + PACK_PIECE - 1) / PACK_PIECE;
    MMNAS_LAUNCH(pack_args_kernel, dim3(pack_grid(npieces)), dim3(256), 0, (hipStream_t)stream, a, n, npieces, staging, scale, direction);
  }
  return check_launch("pack_segments_host");
}

// ---- ragged batches: padded [B, S, d] <-> packed [sum n_b, d] rows (sample b: its first n_b = off[b+1] - off[b] rows) ----
namespace mmnas {
template <bool PACK>
__global__ void __launch_bounds__(256) ragged_rows_kernel(const float4* __restrict__ src, float4* __restrict__ dst,
                                                          const int* __restrict__ off, int B, int S, int d4) {
  const size_t n = (size_t)B * S * d4;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    const size_t row = i / d4;
    const int c = (int)(i - row * d4);
    const int b = (int)(row / S), s = (int)(row - (size_t)b * S);
    const int o = off[b], nb = off[b + 1] - o;
    if (PACK) {
      if (s < nb) dst[(size_t)(o + s) * d4 + c] = src[i];
    } else {
      dst[i] = s < nb ? src[(size_t)(o + s) * d4 + c] : make_float4(0.f, 0.f, 0.f, 0.f);   // padding rows: zero
    }
  }
}
}  // namespace mmnas

extern "C" int mmnas_pack_rows(const float* x, const int* off, float* packed, int B, int S, int d, void* stream) {
  MMNAS_REQUIRE(x && off && packed && B > 0 && S > 0 && d > 0 && d % 4 == 0, MMNAS_E_ARG, "pack_rows: bad arguments (d %% 4 == 0)");
  const size_t n = (size_t)B * S * (d / 4);
  MMNAS_LAUNCH((mmnas::ragged_rows_kernel<true>), dim3((unsigned)std::min<size_t>((n + 255) / 256, 4096)), dim3(256), 0, (hipStream_t)stream,
               (const float4*)x, (float4*)packed, off, B, S, d / 4);
  return mmnas::check_launch("pack_rows");
}

extern "C" int mmnas_unpack_rows(const float* packed, const int* off, float* x, int B, int S, int d, void* stream) {
  MMNAS_REQUIRE(x && off && packed && B > 0 && S > 0 && d > 0 && d % 4 == 0, MMNAS_E_ARG, "unpack_rows: bad arguments (d %% 4 == 0)");
  const size_t n = (size_t)B * S * (d / 4);
  MMNAS_LAUNCH((mmnas::ragged_rows_kernel<false>), dim3((unsigned)std::min<size_t>((n + 255) / 256, 4096)), dim3(256), 0, (hipStream_t)stream,
               (const float4*)packed, (float4*)x, off, B, S, d / 4);
  return mmnas::check_launch("unpack_rows");
}

extern "C" int mmnas_adam_step(float* p, const float* g, float* m, float* v, size_t n, float lr, float beta1,
                               float beta2, float eps, float weight_decay, const float* sumsq, float max_norm,
                               int step, void* stream) {
  if (n == 0) return MMNAS_OK;
  MMNAS_REQUIRE(p && g && m && v && step >= 1, MMNAS_E_ARG, "mmnas_adam_step: bad arguments");
  const AdamCoef k = adam_coef(beta1, beta2, step);
  // 16-byte path for the aligned body, the scalar kernel for a misaligned call or the tail (< 4 elements)
  const bool al16 = ((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) == 0);
  const size_t n4 = al16 ? n / 4 : 0, done = 4 * n4;
  if (n4) {
    const int blocks4 = (int)((n4 + 255) / 256 < 4096 ? (n4 + 255) / 256 : 4096);
    MMNAS_LAUNCH(adam4_kernel, dim3(blocks4), dim3(256), 0, (hipStream_t)stream, (float4*)p, (const float4*)g, (float4*)m, (float4*)v, n4,
                 lr, beta1, beta2, k.omb1, k.omb2, eps, weight_decay, sumsq, max_norm, k.c1, k.c2s);
  }
  if (done < n) {
    const size_t r = n - done;
    const int blocks = (int)((r + 255) / 256 < 4096 ? (r + 255) / 256 : 4096);
    MMNAS_LAUNCH(adam_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, p + done, g + done, m + done, v + done, r, lr, beta1,
                 beta2, k.omb1, k.omb2, eps, weight_decay, sumsq, max_norm, k.c1, k.c2s);
  }
  return check_launch("adam_step");
}

extern "C" int mmnas_sgd_step(float* p, const float* g, float* buf, size_t n, float lr, float momentum, float dampening,
                              float weight_decay, int nesterov, int first, const float* sumsq, float max_norm, void* stream) {
  if (n == 0) return MMNAS_OK;
  const bool mom = momentum != 0.f;
  MMNAS_REQUIRE(p && g && (buf || !mom), MMNAS_E_ARG, "mmnas_sgd_step: null pointer (buf may be null only with momentum == 0)");
  MMNAS_REQUIRE(!nesterov || (mom && dampening == 0.f), MMNAS_E_ARG, "mmnas_sgd_step: nesterov needs momentum != 0 and dampening == 0");
  // 16-byte path for the aligned body, the scalar kernel for a misaligned call or the tail (< 4 elements)
  const bool al16 = ((((uintptr_t)p | (uintptr_t)g | (mom ? (uintptr_t)buf : 0)) & 15) == 0);
  const size_t n4 = al16 ? n / 4 : 0, done = 4 * n4;
  hipStream_t st = (hipStream_t)stream;
  if (n4) {
    const int blocks4 = (int)((n4 + 255) / 256 < 4096 ? (n4 + 255) / 256 : 4096);
    if (mom)
      MMNAS_LAUNCH(sgd4_kernel<true>, dim3(blocks4), dim3(256), 0, st, (float4*)p, (const float4*)g, (float4*)buf, n4, lr, momentum,
                   dampening, weight_decay, nesterov, first, sumsq, max_norm);
    else
      MMNAS_LAUNCH(sgd4_kernel<false>, dim3(blocks4), dim3(256), 0, st, (float4*)p, (const float4*)g, (float4*)nullptr, n4, lr, momentum,
                   dampening, weight_decay, nesterov, first, sumsq, max_norm);
  }
  if (done < n) {
    const size_t r = n - done;
    const int blocks = (int)((r + 255) / 256 < 4096 ? (r + 255) / 256 : 4096);
    if (mom)
      MMNAS_LAUNCH(sgd_kernel<true>, dim3(blocks), dim3(256), 0, st, p + done, g + done, buf + done, r, lr, momentum, dampening,
                   weight_decay, nesterov, first, sumsq, max_norm);
    else
      MMNAS_LAUNCH(sgd_kernel<false>, dim3(blocks), dim3(256), 0, st, p + done, g + done, (float*)nullptr, r, lr, momentum, dampening,
                   weight_decay, nesterov, first, sumsq, max_norm);
  }
  return check_launch("sgd_step");
}

// The partials' buffer of mmnas_sumsq: one per stream (calls on one stream are ordered, calls on two streams never share a
// buffer), allocated at the stream's first call and kept for the life of the process.
static float* sumsq_partials(hipStream_t st) {
  static std::mutex mu;
  static std::vector<std::pair<hipStream_t, float*>> table;
  std::lock_guard<std::mutex> g(mu);
  for (const auto& e : table)
    if (e.first == st) return e.second;
  float* p = nullptr;
  if (hipMalloc(&p, (size_t)2 * SUMSQ_MAX_BLOCKS * sizeof(float)) != hipSuccess) return nullptr;
  table.emplace_back(st, p);
  return p;
}

extern "C" int mmnas_sumsq(const float* g, size_t n, float* out, void* stream) {
  if (n == 0) return MMNAS_OK;
  MMNAS_REQUIRE(g && out, MMNAS_E_ARG, "mmnas_sumsq: null pointer");
  hipStream_t st = (hipStream_t)stream;
  float* part = sumsq_partials(st);
  MMNAS_REQUIRE(part, MMNAS_E_LAUNCH, "mmnas_sumsq: no memory for the partial sums");
  const size_t n4 = (((uintptr_t)g & 15) == 0) ? n / 4 : 0, done = 4 * n4;
  int nparts = 0;
  if (n4) {
    const int blocks4 = (int)((n4 + 255) / 256 < (size_t)SUMSQ_MAX_BLOCKS ? (n4 + 255) / 256 : SUMSQ_MAX_BLOCKS);
    MMNAS_LAUNCH(sumsq4_kernel, dim3(blocks4), dim3(256), 0, st, (const float4*)g, n4, part);
    nparts = blocks4;
  }
  if (done < n) {
    const size_t r = n - done;
    const int blocks = (int)((r + 255) / 256 < (size_t)SUMSQ_MAX_BLOCKS ? (r + 255) / 256 : SUMSQ_MAX_BLOCKS);
    MMNAS_LAUNCH(sumsq_kernel, dim3(blocks), dim3(256), 0, st, g + done, r, part + nparts);
    nparts += blocks;
  }
  MMNAS_LAUNCH(sumsq_final_kernel, dim3(1), dim3(256), 0, st, (const float*)part, nparts, out);
  return check_launch("sumsq");
}
