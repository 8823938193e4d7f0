// Operator-level entry points: one call enqueues every kernel of one reference operator forward
// (or backward) on the caller's stream.  Host-side orchestration only -- the arithmetic lives in
// gemm.hip / attention.hip / relbias.hip / rowops.hip.
//
//   attention family (SelfAtt modules.py:260-271, RelSelfAtt :286-298, GuidedAtt :313-325,
//   UniimgAtt :415-428):
//     fwd:  [Q|K|V] = grouped GEMM -> (rel bias) -> attention core -> merge GEMM with fused
//           dropout+residual epilogue -> LayerNorm                            (4-5 launches)
//     bwd:  LN bwd (+dropout replay) -> d(att) GEMM, dWm GEMM -> core bwd (3 launches) ->
//           dW{q,k,v} grouped GEMM -> dx GEMM(s) with fused residual add -> (rel bias bwd)
//   MLP family (FeedForward modules.py:351-362, FeedForward_deep :389-400).
#include <string.h>
#include <functional>
#include <vector>
#include "common.h"

namespace mmnas {

static inline size_t al(size_t n) { return (n + 255) & ~(size_t)255; }
// whether this operator (or the head) drops: training mode with a positive rate
template <class Op> static inline bool drops(const Op* op) { return (op->flags & MMNAS_F_TRAIN) && op->drop_p > 0.f; }

struct Carver {
  char* base; size_t off;
  explicit Carver(void* p) : base((char*)p), off(0) {}
  float* take(size_t nfloats) { float* r = (float*)(base + off); off += al(nfloats * sizeof(float)); return r; }
};

static void gemm_init(mmnas_gemm_desc& g, int layout, int N, int K, int lda, int ldb, int ldc) {
  memset(&g, 0, sizeof(g));
  g.layout = layout; g.ngroups = 1; g.nseg = 1; g.N = N; g.K = K; g.lda = lda; g.ldb = ldb; g.ldc = ldc;
  g.alpha = 1.f; g.gate_scale = 1.f; g.split_k = 1;
}

struct AttLayout {
  size_t Mq, Mk;
  float *Q, *K, *V, *att, *stats, *z, *biasT;       // save
  float *dz, *dt, *datt, *dQ, *dK, *dV, *delta, *dbiasT, *lnws, *relws;  // backward scratch
  size_t save_bytes, ws_bwd_bytes;
};

static AttLayout att_layout(const mmnas_att_op* op) {
  AttLayout L;
  L.Mq = op->q_off ? (size_t)op->Mq : (size_t)op->B * op->Sq;     // (packed rows: the sum of the sequences' lengths)
  L.Mk = op->k_off ? (size_t)op->Mk : (size_t)op->B * op->Sk;
  const bool norm = op->flags & MMNAS_F_NORM, rel = op->flags & MMNAS_F_REL;
  const bool drop = drops(op);
  Carver s(op->save);
  L.Q = s.take(L.Mq * op->di); L.K = s.take(L.Mk * op->di); L.V = s.take(L.Mk * op->di);
  L.att = s.take(L.Mq * op->di);
  L.stats = s.take((size_t)op->B * op->H * op->Sq * 2);
  L.z = norm ? s.take(L.Mq * op->d) : nullptr;
  L.biasT = rel ? s.take((size_t)op->B * op->H * op->Sk * op->Sq) : nullptr;
  L.save_bytes = s.off;
  Carver w(op->ws);
  L.dz = norm ? w.take(L.Mq * op->d) : nullptr;
  L.dt = drop ? w.take(L.Mq * op->d) : nullptr;
  L.datt = w.take(L.Mq * op->di);
  L.dQ = w.take(L.Mq * op->di); L.dK = w.take(L.Mk * op->di); L.dV = w.take(L.Mk * op->di);
  L.delta = w.take((size_t)op->B * op->H * op->Sq);
  L.dbiasT = rel ? w.take((size_t)op->B * op->H * op->Sk * op->Sq) : nullptr;
  L.lnws = norm ? w.take(mmnas_layernorm_bwd_ws_floats((int)L.Mq, op->d)) : nullptr;
  L.relws = (rel && (op->flags & MMNAS_F_RELRAW)) ? w.take(mmnas_rel_fused_bwd_ws_floats(op->B, op->Sq, op->Sk)) : nullptr;
  L.ws_bwd_bytes = w.off;
  return L;
}

// small.hip: one-launch forms for short sequences
bool sa_small_applies(const mmnas_att_op* op);
int sa_small_fwd(const mmnas_att_op* op, float* Q, float* K, float* V, float* att, float* stats, float* z, hipStream_t st);
bool ffn_small_applies(const mmnas_mlp_op* op);
int ffn_small_fwd(const mmnas_mlp_op* op, float* h, float* z, hipStream_t st);
bool sa_small_bwd_applies(const mmnas_att_op* op);
int sa_small_bwd(const mmnas_att_op* op, const float* Q, const float* K, const float* V, const float* stats, const float* z,
                 float* dt_out, float* dQ, float* dK, float* dV, float* lnpart, hipStream_t st);

// Where an attention operator's LayerNorm runs: inside its own forward launch / inside its own backward launch (the one-launch
// short-sequence kernels above), or neither (its own launch on the general path; the node's mix kernel in a mixed chain).  The ONE
// answer for att_fwd_impl and att_bwd_impl, for what a mixed chain's node epilogue is handed (chain_cand_view, both directions) and for the node's
// fused LayerNorm backward (chain_bwd_mixed).  Shapes, flags and switches decide, not the input pointers: sa_small_applies also
// wants xq == xkv, which a SELF operator of a chain has by construction and which a caller may ask about before it binds
// them; the per-operator entry points compare their own two pointers next to this.
struct LnPlace { bool fwd, bwd; };
static LnPlace att_ln_place(const mmnas_att_op* op) {
  LnPlace p = {false, false};
  if (!(op->flags & MMNAS_F_SELF) || (op->flags & MMNAS_F_REL)) return p;   // (the short-sequence kernels: plain self-attention)
  mmnas_att_op t = *op;
  t.xkv = t.xq;
  p.fwd = sa_small_applies(&t);
  p.bwd = p.fwd && sa_small_bwd_applies(&t);   // (MMNAS_SMALL_BWD=0: the one-launch forward, then the general backward)
  return p;
}

static int att_check(const mmnas_att_op* op, const char* who) {
  MMNAS_REQUIRE(op, MMNAS_E_ARG, "%s: null descriptor", who);
  MMNAS_REQUIRE(op->B > 0 && op->Sq > 0 && op->Sk > 0 && op->d > 0 && op->di > 0, MMNAS_E_SHAPE,
                "%s: B=%d Sq=%d Sk=%d d=%d di=%d", who, op->B, op->Sq, op->Sk, op->d, op->di);
  MMNAS_REQUIRE(op->H * op->dh == op->di, MMNAS_E_SHAPE, "%s: H*dh=%d*%d != di=%d", who, op->H, op->dh, op->di);
  MMNAS_REQUIRE(op->d % 4 == 0 && op->di % 4 == 0, MMNAS_E_SHAPE, "%s: d=%d di=%d must be multiples of 4", who,
                op->d, op->di);
  if (op->flags & MMNAS_F_SELF) MMNAS_REQUIRE(op->Sq == op->Sk, MMNAS_E_SHAPE, "%s: SELF needs Sq == Sk", who);
  if (op->q_off || op->k_off) {   // packed rows
    // (either side alone may be packed: packed keys under dense queries is a guided operator over a ragged language stream --
    //  every attention core reads q_off and k_off independently)
    MMNAS_REQUIRE(!op->q_off || (op->Mq > 0 && op->Mq <= op->B * op->Sq), MMNAS_E_ARG, "%s: packed rows: Mq=%d", who, op->Mq);
    MMNAS_REQUIRE(!op->k_off || (op->Mk > 0 && op->Mk <= op->B * op->Sk), MMNAS_E_ARG, "%s: packed rows: Mk=%d", who, op->Mk);
    if (op->flags & MMNAS_F_SELF) MMNAS_REQUIRE(op->k_off == op->q_off && op->Mk == op->Mq, MMNAS_E_ARG, "%s: packed SELF needs k_off == q_off", who);
    MMNAS_REQUIRE(!(op->k_off && (op->flags & MMNAS_F_MASK)), MMNAS_E_ARG, "%s: packed keys carry no mask", who);
    if (op->flags & MMNAS_F_REL)
      MMNAS_REQUIRE((op->flags & MMNAS_F_RELRAW) && (op->flags & MMNAS_F_SELF) && op->q_off && op->rel_tile_off && op->rel_ntiles >= 0, MMNAS_E_ARG,
                    "%s: a relation bias on packed rows needs the lazy handle (RELRAW), SELF and the relation tile offsets", who);
  }
  return MMNAS_OK;
}

}  // namespace mmnas

using namespace mmnas;

extern "C" int mmnas_att_op_plan(const mmnas_att_op* op, mmnas_plan* plan) {
  int rc = att_check(op, "att_op_plan");
  if (rc) return rc;
  MMNAS_REQUIRE(plan, MMNAS_E_ARG, "att_op_plan: null plan");
  mmnas_att_op tmp = *op;
  tmp.save = nullptr; tmp.ws = nullptr;
  AttLayout L = att_layout(&tmp);
  plan->save_bytes = L.save_bytes;
  plan->ws_fwd_bytes = 256;
  plan->ws_bwd_bytes = L.ws_bwd_bytes;
  return MMNAS_OK;
}

namespace mmnas {
// defer_ln (mixed chains): with NORM the operator stops behind its residual sum z (saved block) and writes no output --
// the node epilogue (mmnas_node_mix_fwd) normalises every candidate of the node and forms the gated sum in one pass.
// *ln_done tells the caller whether the output was normalised here after all (the one-launch short-sequence kernel).
// rel_ready (backbone chains): the relation bias already sits in the saved block (one mmnas_rel_multi_fwd launch at chain entry
// computed it for every relation operator of the stream): skip the per-operator bias launch.
// kv_ready (backbone chains, guided operators): the key / value projections of every guided operator of the chain were
// issued as one grouped launch behind the encoder (they all read the final language state): only Q is projected here.
static int att_fwd_impl(const mmnas_att_op* op, void* stream, bool defer_ln, bool* ln_done, bool rel_ready = false, bool kv_ready = false);
}
extern "C" int mmnas_att_op_fwd(const mmnas_att_op* op, void* stream) {
  bool done;
  return mmnas::att_fwd_impl(op, stream, false, &done);
}
namespace mmnas {
// The forward of an attention operator in three stages, so that a supernet node can run the same stage of all its
// attention candidates as ONE launch (mixed chains): the Q / K / V projections as groups of one grouped product, the
// cores one by one, the merge projections (+ output dropout + residual) as groups of one product with per-group seeds.
static void att_qkv_groups(const mmnas_att_op* op, const AttLayout& L, mmnas_gemm_group* g) {
  memset(g, 0, 3 * sizeof(*g));
  g[0].M = (int)L.Mq; g[0].A[0] = op->xq;  g[0].B[0] = op->Wq; g[0].C = L.Q;
  g[1].M = (int)L.Mk; g[1].A[0] = op->xkv; g[1].B[0] = op->Wk; g[1].C = L.K;
  g[2].M = (int)L.Mk; g[2].A[0] = op->xkv; g[2].B[0] = op->Wv; g[2].C = L.V;
}

static void att_core_desc(const mmnas_att_op* op, const AttLayout& L, mmnas_mha_desc* m) {
  const int fl = op->flags, di = op->di;
  const bool drop = drops(op);
  memset(m, 0, sizeof(*m));
  m->B = op->B; m->H = op->H; m->Sq = op->Sq; m->Sk = op->Sk; m->dh = op->dh;
  m->ldq = m->ldk = m->ldv = m->ldo = di;
  m->Q = L.Q; m->K = L.K; m->V = L.V; m->mask = (fl & MMNAS_F_MASK) ? op->mask : nullptr; m->biasT = L.biasT;
  m->O = L.att; m->lse = L.stats;
  m->q_off = op->q_off; m->k_off = op->k_off;
  m->drop_p = drop ? op->drop_p : 0.f; m->drop_site = 0; m->drop_seed = op->seed;
}

// desc_only != NULL: the relation bias is computed, the core itself is left to the caller (its descriptor in *desc_only)
static int att_core_fwd(const mmnas_att_op* op, const AttLayout& L, void* stream, mmnas_mha_desc* desc_only = nullptr, bool rel_ready = false) {
  const int fl = op->flags;
  const bool rel = (fl & MMNAS_F_REL) && !rel_ready;
  int rc;
  if (rel) {
    if (fl & MMNAS_F_RELRAW) {  // lazy handle: bias straight from the raw [B,Sq,Sk,C] relations
      MMNAS_REQUIRE(op->Wy && op->by, MMNAS_E_ARG, "att_op_fwd: RELRAW without Wy/by");
      // Self-attention (every RelSelfAtt): the one-operator form of the kernel the backbone chains run for ALL relation
      // operators of a stream (relmulti.hip).  A row's bias does not depend on which other rows share its launch, so the
      // per-operator path and the chains produce the same bias BIT FOR BIT -- and with it the same logits.
      if (op->Sq == op->Sk && mmnas_rel_multi_supported(op->C, op->R, op->H) && (long)op->B * op->H * op->Sq * op->Sq < (1l << 31) &&
          !sw::rel_fwd_valu.get()) {
        mmnas_rel_multi q;
        memset(&q, 0, sizeof(q));
        q.B = op->B; q.S = op->Sq; q.C = op->C; q.R = op->R; q.H = op->H; q.n_ops = 1;
        q.raw = op->rel; q.Wy = op->Wy; q.by = op->by;
        q.Wr[0] = op->Wr; q.br[0] = op->br; q.biasT[0] = L.biasT;
        if (op->q_off) {
          MMNAS_REQUIRE(op->rel_tile_off, MMNAS_E_ARG, "att_op_fwd: packed rows without the relation tile offsets");
          q.off = op->q_off; q.tile_off = op->rel_tile_off; q.ntiles = op->rel_ntiles;
        }
        rc = mmnas_rel_multi_fwd(&q, stream);
      } else
      rc = op->q_off ? mmnas_rel_fused_fwd_ragged(op->rel, op->Wy, op->by, op->Wr, op->br, L.biasT, op->B, op->Sq, op->C, op->R,
                                                  op->H, op->q_off, stream)
                     : mmnas_rel_fused_fwd(op->rel, op->Wy, op->by, op->Wr, op->br, L.biasT, op->B, op->Sq, op->Sk, op->C, op->R,
                                           op->H, stream);
    } else {
      rc = mmnas_rel_bias_fwd(op->rel, op->Wr, op->br, L.biasT, op->B, op->Sq, op->Sk, op->R, op->H, stream);
    }
    if (rc) return rc;
  }
  if (desc_only) { att_core_desc(op, L, desc_only); return MMNAS_OK; }
  mmnas_mha_desc m;
  att_core_desc(op, L, &m);
  return mmnas_mha_core_fwd(&m, stream);
}

// the merge projection as one group: C = z (NORM: the LayerNorm follows) or y; residual = the operator's input
static void att_merge_group(const mmnas_att_op* op, const AttLayout& L, mmnas_gemm_group* g) {
  const bool norm = op->flags & MMNAS_F_NORM;
  memset(g, 0, sizeof(*g));
  g->M = (int)L.Mq; g->A[0] = L.att; g->B[0] = op->Wm; g->C = norm ? L.z : op->y;
  if (op->flags & MMNAS_F_RESIDUAL) g->residual = op->xq;
  g->drop_seed = op->seed;
}

static int att_fwd_args(const mmnas_att_op* op) {
  int rc = att_check(op, "att_op_fwd");
  if (rc) return rc;
  MMNAS_REQUIRE(op->xq && op->xkv && op->Wq && op->Wk && op->Wv && op->Wm && op->y && op->save, MMNAS_E_ARG,
                "att_op_fwd: null pointer");
  const int fl = op->flags;
  if (fl & MMNAS_F_NORM) MMNAS_REQUIRE(op->ln_a && op->ln_b, MMNAS_E_ARG, "att_op_fwd: NORM without ln parameters");
  if (fl & MMNAS_F_REL) MMNAS_REQUIRE(op->rel && op->Wr && op->br, MMNAS_E_ARG, "att_op_fwd: REL without rel/Wr/br");
  if (fl & MMNAS_F_MASK) MMNAS_REQUIRE(op->mask, MMNAS_E_ARG, "att_op_fwd: MASK without mask");
  return MMNAS_OK;
}
}  // namespace mmnas

static int mmnas::att_fwd_impl(const mmnas_att_op* op, void* stream, bool defer_ln, bool* ln_done, bool rel_ready, bool kv_ready) {
  *ln_done = true;
  int rc = att_fwd_args(op);
  if (rc) return rc;
  const int fl = op->flags;
  const bool norm = fl & MMNAS_F_NORM;
  const bool drop = drops(op);
  AttLayout L = att_layout(op);
  const int d = op->d, di = op->di;
  if (op->xq == op->xkv && att_ln_place(op).fwd) return sa_small_fwd(op, L.Q, L.K, L.V, L.att, L.stats, L.z, (hipStream_t)stream);

  mmnas_gemm_desc g;
  gemm_init(g, MMNAS_GEMM_NT, di, d, d, d, di);
  g.ngroups = kv_ready ? 1 : 3;
  att_qkv_groups(op, L, g.g);
  if ((rc = mmnas_gemm(&g, stream))) return rc;
  if ((rc = att_core_fwd(op, L, stream, nullptr, rel_ready))) return rc;
  gemm_init(g, MMNAS_GEMM_NT, d, di, di, di, d);
  att_merge_group(op, L, &g.g[0]);
  if (fl & MMNAS_F_RESIDUAL) g.ldres = d;
  if (drop) { g.drop_p = op->drop_p; g.drop_site = 1; g.drop_seed = op->seed; }
  // d = 256: the projection, its dropout + residual epilogue and the LayerNorm as ONE launch (gemmln.hip)
  if (norm && !defer_ln && gemm_ln_applies(&g)) return gemm_ln(&g, op->ln_a, op->ln_b, op->y, d, op->eps, (hipStream_t)stream);
  if ((rc = mmnas_gemm(&g, stream))) return rc;

  if (norm && defer_ln) { *ln_done = false; return MMNAS_OK; }
  if (norm) return mmnas_layernorm_fwd(L.z, op->ln_a, op->ln_b, op->y, (int)L.Mq, d, op->eps, stream);
  return MMNAS_OK;
}

namespace mmnas {
// Parameter-gradient work set aside by the backward functions below when a queue is given: launches that nothing on
// the data-gradient chain waits for (weight-gradient products, LayerNorm parameter reductions, the relation-bias
// backward).  The caller decides when and on which stream they run (SideQueue::flush).
struct SideQueue {
  std::vector<std::function<int(hipStream_t)>> work;
  bool rel_only = false;   // queue only the relation-bias backward; the weight gradients stay paired on the main stream
  // everything `main` has been given so far finishes first; then the queued launches run on `side`
  int flush(hipStream_t main, hipStream_t side, hipEvent_t ev) {
    if (work.empty()) return MMNAS_OK;
    hipStream_t s = side;
    if (hipEventRecord(ev, main) != hipSuccess || hipStreamWaitEvent(side, ev, 0) != hipSuccess)
      s = main;   // (cannot order the streams: stay on the main one, which is always correct)
    for (auto& f : work) {
      const int rc = f(s);
      if (rc) return rc;
    }
    work.clear();
    return MMNAS_OK;
  }
};

// sq == nullptr: the single-stream order (data- and weight-gradient products paired in one launch).
// With a queue: `stream` carries only the chain the NEXT operator's backward waits for -- LayerNorm backward, the
// data-gradient products, the attention core; the weight-gradient products, the LayerNorm parameter reduction and the
// whole relation-bias backward (~40 % of an operator's backward time, read by nothing before the optimizer / the
// gradient exchange) are queued.
// acc_kv (guided operators inside the backbone chain): the key / value source's gradient is ADDED to *dxkv (the chain's
// running sum over the guided operators) instead of overwriting it -- saves the chain a buffer and an add launch each.
// rel_defer (backbone chains): the bias gradient dbiasT stays in the operator's scratch block; ONE mmnas_rel_multi_bwd launch
// behind the stream's last relation operator turns every operator's dbiasT into its dWr / dbr and the shared dWy / dby.
// kv_defer (backbone chains, guided operators): dK / dV stay in the scratch block; the chain turns every guided operator's
// pair into its key / value source gradient and dWk / dWv by grouped launches behind the last guided operator's backward.
// ln_pre (mixed chains, round 6): the LayerNorm backward already ran inside the node's mix kernel -- dz / dt of the scratch block
// are filled and *ln_pre is the pending parameter reduction; op->dy is not read.
// ktab (backbone chains, image stream): the live-row K-tile table of the chain's gradient rows (mmnas_wgrad_live_table) for
// the weight gradients that reduce over the query rows; the per-operator entry point never passes one.
static int att_bwd_impl(const mmnas_att_op* op, hipStream_t stream, SideQueue* sq, bool acc_kv = false, bool rel_defer = false, bool kv_defer = false,
                        const AuxReduce* ln_pre = nullptr, const int* ktab = nullptr) {
  const bool side = sq != nullptr && !sq->rel_only;
  const bool side_rel = sq != nullptr;
  int rc = att_check(op, "att_op_bwd");
  if (rc) return rc;
  MMNAS_REQUIRE(op->xq && op->xkv && op->Wq && op->Wk && op->Wv && op->Wm && op->save && op->ws && op->dy &&
                    op->dxq && op->dWq && op->dWk && op->dWv && op->dWm,
                MMNAS_E_ARG, "att_op_bwd: null pointer");
  const int fl = op->flags;
  const bool norm = fl & MMNAS_F_NORM, rel = fl & MMNAS_F_REL, self = fl & MMNAS_F_SELF;
  const bool drop = drops(op);
  if (!self) MMNAS_REQUIRE(op->dxkv, MMNAS_E_ARG, "att_op_bwd: dxkv required unless SELF");
  if (norm) MMNAS_REQUIRE(op->ln_a && op->dln_a && op->dln_b, MMNAS_E_ARG, "att_op_bwd: NORM gradients missing");
  if (rel) MMNAS_REQUIRE(op->rel && op->Wr && op->br && op->dWr && op->dbr, MMNAS_E_ARG, "att_op_bwd: REL gradients missing");
  AttLayout L = att_layout(op);
  const int d = op->d, di = op->di, Mq = (int)L.Mq, Mk = (int)L.Mk;

  // Short sequences (the language stream): steps 1, 2, 4 and the data-gradient half of 5 + 6 as ONE launch (small.hip), then
  // the four weight gradients as one grouped launch that carries the LayerNorm parameter reduction.
  if (!ln_pre && !sq && op->xq == op->xkv && att_ln_place(op).bwd) {
    float* const dt_out = drop ? L.dt : (norm ? L.dz : nullptr);
    if ((rc = sa_small_bwd(op, L.Q, L.K, L.V, L.stats, L.z, dt_out, L.dQ, L.dK, L.dV, norm ? L.lnws : nullptr, stream))) return rc;
    mmnas_gemm_desc w4;
    gemm_init(w4, MMNAS_GEMM_TN, d, Mq, d, d, d);
    w4.ngroups = 4;
    w4.g[0].M = d; w4.g[0].A[0] = dt_out ? dt_out : op->dy; w4.g[0].B[0] = L.att; w4.g[0].C = op->dWm;
    w4.g[1].M = d; w4.g[1].A[0] = L.dQ; w4.g[1].B[0] = op->xq; w4.g[1].C = op->dWq;
    w4.g[2].M = d; w4.g[2].A[0] = L.dK; w4.g[2].B[0] = op->xq; w4.g[2].C = op->dWk;
    w4.g[3].M = d; w4.g[3].A[0] = L.dV; w4.g[3].B[0] = op->xq; w4.g[3].C = op->dWv;
    w4.accumulate = 1;
    AuxReduce red;
    red.part = norm ? L.lnws : nullptr; red.nrows = op->B; red.d = d;
    red.out[0] = op->dln_a; red.out[1] = op->dln_b; red.out[2] = nullptr;
    return gemm_pair_aux(nullptr, &w4, &red, stream);
  }

  // 1. through LayerNorm and the output dropout
  const float* dz = op->dy;   // gradient wrt z = x + drop(core)
  const float* dt = op->dy;   // gradient wrt core
  AuxReduce lnred;   // the LayerNorm parameter-gradient reduction rides on the first gradient-pair launch below
  lnred.part = nullptr;
  if (norm && ln_pre) {
    lnred = *ln_pre;
    dz = L.dz; dt = drop ? L.dt : L.dz;
  } else if (norm) {
    if ((rc = layernorm_bwd_deferred(L.z, op->ln_a, op->dy, L.dz, op->dln_a, op->dln_b, drop ? L.dt : nullptr, nullptr,
                                     L.lnws, drop ? op->drop_p : 0.f, op->seed, 1, Mq, d, op->eps, (hipStream_t)stream, &lnred)))
      return rc;
    dz = L.dz; dt = drop ? L.dt : L.dz;
  } else if (drop) {
    if ((rc = mmnas_drop_add(op->dy, nullptr, L.dt, (size_t)Mq * d, op->drop_p, op->seed, 1, stream))) return rc;
    dt = L.dt;
  }

  mmnas_gemm_desc g, w, wm, w2;
  // 2. d(att) = dt Wm            [Mq,d] x [d,di]
  gemm_init(g, MMNAS_GEMM_NN, di, d, d, di, di);
  g.g[0].M = Mq; g.g[0].A[0] = dt; g.g[0].B[0] = op->Wm; g.g[0].C = L.datt;
  // 3. dWm += dt^T att           [d,di], reduction over the Mq rows (same launch: mmnas_gemm_pair)
  gemm_init(wm, MMNAS_GEMM_TN, di, Mq, d, di, di);
  wm.g[0].M = d; wm.g[0].A[0] = dt; wm.g[0].B[0] = L.att; wm.g[0].C = op->dWm;
  wm.accumulate = 1; wm.ktab = ktab;
  if (side) { if ((rc = mmnas_gemm(&g, stream))) return rc; }
  else if ((rc = gemm_pair_aux(&g, &wm, &lnred, (hipStream_t)stream))) return rc;

  // 4. attention core backward
  mmnas_mha_desc m;
  att_core_desc(op, L, &m);
  m.dO = L.datt; m.dQ = L.dQ; m.dK = L.dK; m.dV = L.dV; m.dbiasT = L.dbiasT; m.delta = L.delta;
  if ((rc = mmnas_mha_core_bwd(&m, stream))) return rc;

  // 5. + 6. projection weight gradients and input gradients (+ the residual branch dz), pairwise in one launch
  if (self) {
    gemm_init(w, MMNAS_GEMM_TN, d, Mq, di, d, d);
    w.ngroups = 3;
    w.g[0].M = di; w.g[0].A[0] = L.dQ; w.g[0].B[0] = op->xq;  w.g[0].C = op->dWq;
    w.g[1].M = di; w.g[1].A[0] = L.dK; w.g[1].B[0] = op->xkv; w.g[1].C = op->dWk;
    w.g[2].M = di; w.g[2].A[0] = L.dV; w.g[2].B[0] = op->xkv; w.g[2].C = op->dWv;
    w.accumulate = 1; w.ktab = ktab;   // (self-attention: the key rows are the query rows -- one table for the three groups)
    gemm_init(g, MMNAS_GEMM_NN, d, di, di, d, d);
    g.nseg = 3;
    g.g[0].M = Mq; g.g[0].C = op->dxq;
    g.g[0].A[0] = L.dQ; g.g[0].B[0] = op->Wq;
    g.g[0].A[1] = L.dK; g.g[0].B[1] = op->Wk;
    g.g[0].A[2] = L.dV; g.g[0].B[2] = op->Wv;
    if (fl & MMNAS_F_RESIDUAL) { g.g[0].residual = dz; g.ldres = d; }
    if (side) {
      if ((rc = mmnas_gemm(&g, stream))) return rc;
    } else if ((rc = mmnas_gemm_pair(&g, &w, stream))) return rc;
  } else {
    gemm_init(w, MMNAS_GEMM_TN, d, Mq, di, d, d);
    w.g[0].M = di; w.g[0].A[0] = L.dQ; w.g[0].B[0] = op->xq; w.g[0].C = op->dWq;
    w.accumulate = 1; w.ktab = ktab;   // (dWk / dWv below reduce over the language rows: dense)
    gemm_init(g, MMNAS_GEMM_NN, d, di, di, d, d);
    g.g[0].M = Mq; g.g[0].C = op->dxq; g.g[0].A[0] = L.dQ; g.g[0].B[0] = op->Wq;
    if (fl & MMNAS_F_RESIDUAL) { g.g[0].residual = dz; g.ldres = d; }
    if (side) {
      if ((rc = mmnas_gemm(&g, stream))) return rc;
    } else if ((rc = mmnas_gemm_pair(&g, &w, stream))) return rc;
    if (kv_defer) goto params;
    gemm_init(w2, MMNAS_GEMM_TN, d, Mk, di, d, d);
    w2.ngroups = 2;
    w2.g[0].M = di; w2.g[0].A[0] = L.dK; w2.g[0].B[0] = op->xkv; w2.g[0].C = op->dWk;
    w2.g[1].M = di; w2.g[1].A[0] = L.dV; w2.g[1].B[0] = op->xkv; w2.g[1].C = op->dWv;
    w2.accumulate = 1;
    gemm_init(g, MMNAS_GEMM_NN, d, di, di, d, d);
    g.nseg = 2;
    g.g[0].M = Mk; g.g[0].C = op->dxkv;
    g.g[0].A[0] = L.dK; g.g[0].B[0] = op->Wk;
    g.g[0].A[1] = L.dV; g.g[0].B[1] = op->Wv;
    if (acc_kv) g.accumulate = 1;
    if (side) {
      if ((rc = mmnas_gemm(&g, stream))) return rc;
    } else if ((rc = mmnas_gemm_pair(&g, &w2, stream))) return rc;
  }

params:
  // Parameter-gradient work.  Single stream: the weight gradients went out paired above, the relation-bias backward
  // follows.  Side stream: all of it goes there, behind ONE event recorded at this point of `stream`.
  if (side) {
    sq->work.push_back([lnred](hipStream_t s) { return launch_aux_reduce(lnred, s); });
    sq->work.push_back([wm](hipStream_t s) { return mmnas_gemm(&wm, s); });
    sq->work.push_back([w](hipStream_t s) { return mmnas_gemm(&w, s); });
    if (!self) sq->work.push_back([w2](hipStream_t s) { return mmnas_gemm(&w2, s); });
  }
  // 7. relation bias
  if (rel && rel_defer) return MMNAS_OK;
  if (rel && (fl & MMNAS_F_RELRAW)) {
    MMNAS_REQUIRE(op->Wy && op->by && op->dWy && op->dby, MMNAS_E_ARG, "att_op_bwd: RELRAW gradients missing");
    const mmnas_att_op o = *op;
    float* const dbiasT = L.dbiasT;
    float* const relws = L.relws;
    auto relb = [o, dbiasT, relws](hipStream_t s) {
      if (o.q_off)
        return mmnas_rel_fused_bwd_ragged(o.rel, o.Wy, o.by, o.Wr, o.br, dbiasT, o.dWy, o.dby, o.dWr, o.dbr, relws, o.B, o.Sq,
                                          o.C, o.R, o.H, o.q_off, o.rel_tile_off, o.rel_ntiles, s);
      return mmnas_rel_fused_bwd(o.rel, o.Wy, o.by, o.Wr, o.br, dbiasT, o.dWy, o.dby, o.dWr, o.dbr, relws, o.B, o.Sq, o.Sk,
                                 o.C, o.R, o.H, s);
    };
    if (side_rel) { sq->work.push_back(relb); return MMNAS_OK; }
    return relb(stream);
  }
  if (rel)   // (a materialised relation tensor's own gradient may feed the caller: main stream)
    return mmnas_rel_bias_bwd(op->rel, op->Wr, op->br, L.dbiasT, op->drel, op->dWr, op->dbr, 0, op->B, op->Sq,
                              op->Sk, op->R, op->H, stream);
  return MMNAS_OK;
}
}  // namespace mmnas

extern "C" int mmnas_att_op_bwd(const mmnas_att_op* op, void* stream) {
  return att_bwd_impl(op, (hipStream_t)stream, nullptr);
}

// ------------------------------------------------------------------------------------------ MLP
namespace mmnas {

struct MlpLayout {
  float* h[3];      // h[i] = input of layer i (h[0] = x, not stored); saved for i >= 1
  float* z;
  float *dz, *dt, *dp[3], *lnws;
  size_t save_bytes, ws_bwd_bytes;
};

static MlpLayout mlp_layout(const mmnas_mlp_op* op) {
  MlpLayout L;
  const bool norm = op->flags & MMNAS_F_NORM;
  const bool drop = drops(op);
  const size_t M = (size_t)op->M;
  Carver s(op->save);
  L.h[0] = nullptr;
  for (int i = 1; i < 3; ++i) L.h[i] = (i < op->nl) ? s.take(M * op->dims[i]) : nullptr;
  L.z = norm ? s.take(M * op->dims[0]) : nullptr;
  L.save_bytes = s.off;
  size_t maxh = 4;
  for (int i = 1; i < op->nl; ++i) if ((size_t)op->dims[i] > maxh) maxh = op->dims[i];
  Carver w(op->ws);
  L.dz = norm ? w.take(M * op->dims[0]) : nullptr;
  L.dt = drop ? w.take(M * op->dims[0]) : nullptr;
  L.dp[0] = w.take(M * maxh);
  L.dp[1] = op->nl > 2 ? w.take(M * maxh) : nullptr;
  L.dp[2] = nullptr;
  L.lnws = norm ? w.take(mmnas_layernorm_bwd_ws_floats(op->M, op->dims[0])) : nullptr;
  L.ws_bwd_bytes = w.off;
  return L;
}

static int mlp_check(const mmnas_mlp_op* op, const char* who) {
  MMNAS_REQUIRE(op, MMNAS_E_ARG, "%s: null descriptor", who);
  MMNAS_REQUIRE(op->nl >= 1 && op->nl <= 3 && op->M > 0, MMNAS_E_SHAPE, "%s: nl=%d M=%d", who, op->nl, op->M);
  MMNAS_REQUIRE(op->dims[0] == op->dims[op->nl], MMNAS_E_SHAPE, "%s: in/out width differ (%d vs %d)", who,
                op->dims[0], op->dims[op->nl]);
  for (int i = 0; i <= op->nl; ++i)
    MMNAS_REQUIRE(op->dims[i] > 0 && op->dims[i] % 4 == 0, MMNAS_E_SHAPE, "%s: dims[%d]=%d", who, i, op->dims[i]);
  return MMNAS_OK;
}

}  // namespace mmnas

extern "C" int mmnas_mlp_op_plan(const mmnas_mlp_op* op, mmnas_plan* plan) {
  int rc = mlp_check(op, "mlp_op_plan");
  if (rc) return rc;
  MMNAS_REQUIRE(plan, MMNAS_E_ARG, "mlp_op_plan: null plan");
  mmnas_mlp_op tmp = *op;
  tmp.save = nullptr; tmp.ws = nullptr;
  MlpLayout L = mlp_layout(&tmp);
  plan->save_bytes = L.save_bytes ? L.save_bytes : 256;
  plan->ws_fwd_bytes = 256;
  plan->ws_bwd_bytes = L.ws_bwd_bytes;
  return MMNAS_OK;
}

namespace mmnas {
static int mlp_fwd_impl(const mmnas_mlp_op* op, void* stream, bool defer_ln, bool* ln_done);
}
extern "C" int mmnas_mlp_op_fwd(const mmnas_mlp_op* op, void* stream) {
  bool done;
  return mmnas::mlp_fwd_impl(op, stream, false, &done);
}
static int mmnas::mlp_fwd_impl(const mmnas_mlp_op* op, void* stream, bool defer_ln, bool* ln_done) {
  *ln_done = true;
  int rc = mlp_check(op, "mlp_op_fwd");
  if (rc) return rc;
  MMNAS_REQUIRE(op->x && op->y && op->save, MMNAS_E_ARG, "mlp_op_fwd: null pointer");
  const int fl = op->flags;
  const bool norm = fl & MMNAS_F_NORM;
  const bool drop = drops(op);
  if (norm) MMNAS_REQUIRE(op->ln_a && op->ln_b, MMNAS_E_ARG, "mlp_op_fwd: NORM without ln parameters");
  MlpLayout L = mlp_layout(op);
  const int d = op->dims[0];
  // short row counts (the language stream): both layers, the residual and the LayerNorm as ONE launch (small.hip); a deferred
  // LayerNorm (architecture-step nodes) keeps the general path
  if (!(norm && defer_ln) && ffn_small_applies(op)) return ffn_small_fwd(op, L.h[1], L.z, (hipStream_t)stream);
  const float* in = op->x;
  mmnas_gemm_desc g;
  for (int i = 0; i < op->nl; ++i) {
    MMNAS_REQUIRE(op->W[i], MMNAS_E_ARG, "mlp_op_fwd: W[%d] null", i);
    const bool last = i == op->nl - 1;
    gemm_init(g, MMNAS_GEMM_NT, op->dims[i + 1], op->dims[i], op->dims[i], op->dims[i], op->dims[i + 1]);
    g.g[0].M = op->M; g.g[0].A[0] = in; g.g[0].B[0] = op->W[i]; g.g[0].bias = op->b[i];
    if (drop) { g.drop_p = op->drop_p; g.drop_seed = op->seed; g.drop_site = last ? 1u : (i == 0 ? 0u : 2u); }
    if (last) {
      g.g[0].C = norm ? L.z : op->y;
      if (fl & MMNAS_F_RESIDUAL) { g.g[0].residual = op->x; g.ldres = d; }
    } else {
      g.relu = 1;
      g.g[0].C = L.h[i + 1];
    }
    if (last && norm && !defer_ln && gemm_ln_applies(&g)) return gemm_ln(&g, op->ln_a, op->ln_b, op->y, d, op->eps, (hipStream_t)stream);
    if ((rc = mmnas_gemm(&g, stream))) return rc;
    in = L.h[i + 1];
  }
  if (norm && defer_ln) { *ln_done = false; return MMNAS_OK; }
  if (norm) return mmnas_layernorm_fwd(L.z, op->ln_a, op->ln_b, op->y, op->M, d, op->eps, stream);
  return MMNAS_OK;
}

namespace mmnas {
static int mlp_bwd_impl(const mmnas_mlp_op* op, hipStream_t stream, SideQueue* sq, const AuxReduce* ln_pre = nullptr, const int* ktab = nullptr) {
  const bool side = sq != nullptr && !sq->rel_only;
  int rc = mlp_check(op, "mlp_op_bwd");
  if (rc) return rc;
  MMNAS_REQUIRE(op->x && op->save && op->ws && op->dy && op->dx, MMNAS_E_ARG, "mlp_op_bwd: null pointer");
  const int fl = op->flags;
  const bool norm = fl & MMNAS_F_NORM;
  const bool drop = drops(op);
  MlpLayout L = mlp_layout(op);
  const int d = op->dims[0], M = op->M, nl = op->nl;
  for (int i = 0; i < nl; ++i)
    MMNAS_REQUIRE(op->W[i] && op->dW[i], MMNAS_E_ARG, "mlp_op_bwd: W/dW[%d] null", i);

  const float* dz = op->dy;
  const float* dt = op->dy;
  bool last_bias_done = false;
  AuxReduce lnred;   // pending LayerNorm reduction: rides on the first gradient-pair launch
  lnred.part = nullptr;
  if (norm) {
    MMNAS_REQUIRE(op->ln_a && op->dln_a && op->dln_b, MMNAS_E_ARG, "mlp_op_bwd: NORM gradients missing");
    // the column sums of the dropped gradient are the last layer's bias gradient: fused when a
    // separate dt buffer exists
    float* dcol = (drop && op->db[nl - 1]) ? op->db[nl - 1] : nullptr;
    if (ln_pre) lnred = *ln_pre;     // (mixed chains: done inside the node's mix kernel, dcol among its partial rows)
    else if ((rc = layernorm_bwd_deferred(L.z, op->ln_a, op->dy, L.dz, op->dln_a, op->dln_b, drop ? L.dt : nullptr, dcol,
                                          L.lnws, drop ? op->drop_p : 0.f, op->seed, 1, M, d, op->eps, (hipStream_t)stream, &lnred)))
      return rc;
    dz = L.dz; dt = drop ? L.dt : L.dz;
    last_bias_done = dcol != nullptr;
  } else if (drop) {
    if ((rc = mmnas_drop_add(op->dy, nullptr, L.dt, (size_t)M * d, op->drop_p, op->seed, 1, stream))) return rc;
    dt = L.dt;
  }

  const float gate_scale = drop ? 1.0f / (1.0f - op->drop_p) : 1.0f;
  const float* dpre = dt;  // gradient wrt the pre-activation output of layer i
  mmnas_gemm_desc g;
  mmnas_gemm_desc wd[3];   // the weight-gradient products (side-stream mode: issued after the data-gradient chain)
  const bool last_colsum = op->db[nl - 1] && !last_bias_done;
  if (last_colsum && !side)
    if ((rc = mmnas_colsum(dpre, op->db[nl - 1], M, op->dims[nl], op->dims[nl], stream))) return rc;
  for (int i = nl - 1; i >= 0; --i) {
    const float* hin = i == 0 ? op->x : L.h[i];
    const int nout = op->dims[i + 1], nin = op->dims[i];
    // bias gradient: column sums of dpre.  The last layer's ride on the LayerNorm backward when possible (else the
    // colsum launch above / on the side stream); a hidden layer's are accumulated by the epilogue of the data-gradient
    // product that writes its dpre (below)
    // weight gradient dW_i[nout,nin] += dpre^T hin and data gradient, one launch (or: the side stream)
    mmnas_gemm_desc& w = wd[i];
    gemm_init(w, MMNAS_GEMM_TN, nin, M, nout, nin, nin);
    w.g[0].M = nout; w.g[0].A[0] = dpre; w.g[0].B[0] = hin; w.g[0].C = op->dW[i];
    w.accumulate = 1; w.ktab = ktab;
    gemm_init(g, MMNAS_GEMM_NN, nin, nout, nout, nin, nin);
    g.g[0].M = M; g.g[0].A[0] = dpre; g.g[0].B[0] = op->W[i];
    if (i == 0) {
      g.g[0].C = op->dx;
      if (fl & MMNAS_F_RESIDUAL) { g.g[0].residual = dz; g.ldres = d; }
    } else {
      float* out = L.dp[(nl - 1 - i) % 3];   // (side-stream mode reads every dpre later: no buffer is reused)
      g.g[0].C = out;
      g.g[0].gate = L.h[i]; g.ldgate = nin; g.gate_scale = gate_scale;  // relu' and dropout replay from h_i
      g.g[0].colsum = op->db[i - 1];   // db_{i-1} += column sums of dpre_{i-1} (may be NULL: layer without bias)
    }
    if (side) {
      if ((rc = mmnas_gemm(&g, stream))) return rc;
    } else if ((rc = gemm_pair_aux(&g, &w, i == nl - 1 ? &lnred : nullptr, (hipStream_t)stream))) return rc;
    if (i > 0) dpre = g.g[0].C;
  }
  if (side) {
    sq->work.push_back([lnred](hipStream_t s) { return launch_aux_reduce(lnred, s); });
    if (last_colsum) {
      float* const db = op->db[nl - 1];
      const int n = op->dims[nl];
      sq->work.push_back([dt, db, M, n](hipStream_t s) { return mmnas_colsum(dt, db, M, n, n, s); });
    }
    for (int i = nl - 1; i >= 0; --i) {
      const mmnas_gemm_desc w = wd[i];
      sq->work.push_back([w](hipStream_t s) { return mmnas_gemm(&w, s); });
    }
  }
  return MMNAS_OK;
}
}  // namespace mmnas

extern "C" int mmnas_mlp_op_bwd(const mmnas_mlp_op* op, void* stream) {
  return mlp_bwd_impl(op, (hipStream_t)stream, nullptr);
}

// ------------------------------------------------------------------------------------------ backbone chain
// One call = every cell operator of a backbone (Backbone_*.forward, hygr_vqa.py:45-52 / full_vqa.py:46-53) in
// evaluation order: the host issues O(1) calls per step instead of one autograd node, six allocations and a descriptor
// per operator and direction.  Intermediate activations, saved blocks and backward scratch live in ONE caller-owned
// arena laid out by mmnas_chain_plan.
#include <map>
#include <mutex>
#include <utility>
namespace mmnas {

struct ChainLayout {
  size_t y[MMNAS_CHAIN_MAX_OPS], save[MMNAS_CHAIN_MAX_OPS], ws[MMNAS_CHAIN_MAX_OPS], dx[MMNAS_CHAIN_MAX_OPS],
      tmp[MMNAS_CHAIN_MAX_OPS];
  size_t dpre, encdy, relws, ktab, total;
  int last_x, last_y, first_x, first_y, n_guided;
  // per operator: the operator (mixed chains: the node, named by its first operator) whose output it reads, -1 = the chain's
  // input; the node it belongs to (plain chains: itself)
  int src[MMNAS_CHAIN_MAX_OPS], head[MMNAS_CHAIN_MAX_OPS];
  // mixed chains: per node (indexed by the node's first operator) the node output and the sampled candidate's output
  // gradient; one scratch block for the gate-gradient partials
  size_t nout[MMNAS_CHAIN_MAX_OPS], ndact[MMNAS_CHAIN_MAX_OPS], mixws;
};

static int chain_check(const mmnas_chain* c, const char* who) {
  MMNAS_REQUIRE(c && c->ops, MMNAS_E_ARG, "%s: null chain", who);
  MMNAS_REQUIRE(c->n_ops >= 1 && c->n_ops <= MMNAS_CHAIN_MAX_OPS, MMNAS_E_SHAPE, "%s: %d operators (1..%d)", who, c->n_ops, MMNAS_CHAIN_MAX_OPS);
  MMNAS_REQUIRE(c->B > 0 && c->Sx > 0 && c->Sy > 0 && c->d > 0, MMNAS_E_SHAPE, "%s: B=%d Sx=%d Sy=%d d=%d", who, c->B, c->Sx, c->Sy, c->d);
  if (c->y_off) MMNAS_REQUIRE(c->Ny > 0 && c->Ny <= c->B * c->Sy && c->Sy <= 128 && !c->use_side_stream, MMNAS_E_ARG,
                              "%s: ragged decoder stream: Ny=%d of B*Sy=%d rows, Sy=%d <= 128, single stream", who, c->Ny, c->B * c->Sy, c->Sy);
  if (c->x_off) MMNAS_REQUIRE(c->Nx > 0 && c->Nx <= c->B * c->Sx && c->Sx <= 128 && !c->use_side_stream, MMNAS_E_ARG,
                              "%s: ragged language stream: Nx=%d of B*Sx=%d rows, Sx=%d <= 128, single stream", who, c->Nx, c->B * c->Sx, c->Sx);
  bool seen_y = false;
  for (int i = 0; i < c->n_ops; ++i) {
    const mmnas_chain_op& o = c->ops[i];
    MMNAS_REQUIRE(o.kind == MMNAS_CHAIN_ATT || o.kind == MMNAS_CHAIN_MLP, MMNAS_E_ARG, "%s: operator %d: kind %d", who, i, o.kind);
    if (o.on_y) seen_y = true;
    else MMNAS_REQUIRE(!seen_y, MMNAS_E_ARG, "%s: encoder operators must precede the decoder's (operator %d)", who, i);
    if (o.kind == MMNAS_CHAIN_ATT && !(o.att.flags & MMNAS_F_SELF))
      MMNAS_REQUIRE(o.on_y, MMNAS_E_ARG, "%s: operator %d: guided attention needs the decoder stream", who, i);
    if (c->x_off && o.kind == MMNAS_CHAIN_ATT) {
      // the token relations stay a padded [B,Sx,Sx,C] tensor nobody tiles for packed rows; the packed cores: every head size,
      // <= 128 queries / keys per sequence
      MMNAS_REQUIRE(o.on_y || !(o.att.flags & MMNAS_F_REL), MMNAS_E_ARG, "%s: operator %d: ragged language stream: no encoder operator with a relation bias", who, i);
      if (!o.on_y || !(o.att.flags & MMNAS_F_SELF))
        MMNAS_REQUIRE(!o.on_y || c->Sy <= 128, MMNAS_E_ARG,
                      "%s: operator %d: ragged language stream: packed keys need Sy=%d <= 128 queries", who, i, c->Sy);
    }
  }
  if (c->mixed) {
    MMNAS_REQUIRE(c->gate && c->gate_width >= 1 && c->gate_width <= MMNAS_MIXED_MAX, MMNAS_E_ARG, "%s: mixed chain without a gate block (width %d)", who, c->gate_width);
    MMNAS_REQUIRE(!c->use_side_stream, MMNAS_E_ARG, "%s: mixed chains run on one stream", who);
    MMNAS_REQUIRE(c->d <= 1024, MMNAS_E_SHAPE, "%s: mixed chains need d <= 1024", who);
    int node = -1, live = 0, count = 0;
    for (int i = 0; i < c->n_ops; ++i) {
      const mmnas_chain_op& o = c->ops[i];
      if (o.node != node) {
        MMNAS_REQUIRE(o.node == node + 1, MMNAS_E_ARG, "%s: operator %d: node %d after node %d", who, i, o.node, node);
        MMNAS_REQUIRE(node < 0 || live == 1, MMNAS_E_ARG, "%s: node %d has %d differentiated candidates (exactly one)", who, node, live);
        node = o.node; live = 0; count = 0;
      } else {
        MMNAS_REQUIRE(o.on_y == c->ops[i - 1].on_y, MMNAS_E_ARG, "%s: node %d mixes the two streams", who, node);
      }
      MMNAS_REQUIRE(o.cand >= 0 && o.cand < c->gate_width, MMNAS_E_ARG, "%s: operator %d: candidate %d outside the gate row", who, i, o.cand);
      MMNAS_REQUIRE(++count <= MMNAS_MIXED_MAX, MMNAS_E_SHAPE, "%s: node %d has more than %d candidates", who, node, MMNAS_MIXED_MAX);
      live += o.detached ? 0 : 1;
    }
    MMNAS_REQUIRE(live == 1, MMNAS_E_ARG, "%s: node %d has %d differentiated candidates (exactly one)", who, node, live);
  }
  return MMNAS_OK;
}

// rows of the decoder stream: B * Sy, or the packed row count of a ragged batch
static inline size_t chain_rows_y(const mmnas_chain* c) { return c->y_off ? (size_t)c->Ny : (size_t)c->B * c->Sy; }
// rows of the language stream: B * Sx, or the packed row count of a ragged language stream (x_off)
static inline size_t chain_rows_x(const mmnas_chain* c) { return c->x_off ? (size_t)c->Nx : (size_t)c->B * c->Sx; }

// operator i with its stream-dependent fields filled in (shapes, masks, relation tensors): all that chain_layout, which runs
// before an arena exists, needs; the buffers come with chain_bind
static void chain_op_shapes(const mmnas_chain* c, int i, mmnas_att_op& a, mmnas_mlp_op& m) {
  const mmnas_chain_op& o = c->ops[i];
  const int S = o.on_y ? c->Sy : c->Sx;
  if (o.kind == MMNAS_CHAIN_ATT) {
    a = o.att;
    a.B = c->B; a.d = c->d; a.Sq = S;
    const bool self = a.flags & MMNAS_F_SELF;
    a.Sk = self ? S : c->Sx;
    const uint8_t* mask = (self && o.on_y) ? c->y_mask : c->x_mask;
    a.q_off = a.k_off = nullptr; a.Mq = a.Mk = 0; a.rel_tile_off = nullptr; a.rel_ntiles = 0;
    if (o.on_y && c->y_off) {   // ragged decoder stream: packed queries; self-attention over the sample's own packed rows
      a.q_off = c->y_off; a.Mq = c->Ny;
      if (self) { a.k_off = c->y_off; a.Mk = c->Ny; mask = nullptr; a.rel_tile_off = c->y_tile_off; a.rel_ntiles = c->y_ntiles; }
    }
    if (c->x_off && (!o.on_y || !self)) {   // ragged language stream: the keys of an encoder or guided operator are its packed rows
      a.k_off = c->x_off; a.Mk = c->Nx; mask = nullptr;
      if (!o.on_y) { a.q_off = c->x_off; a.Mq = c->Nx; }
    }
    a.mask = mask;
    if (mask) a.flags |= MMNAS_F_MASK; else a.flags &= ~MMNAS_F_MASK;
    if (a.flags & MMNAS_F_REL) a.rel = o.on_y ? c->y_rel : c->x_rel;
  } else {
    m = o.mlp;
    m.M = o.on_y ? (int)chain_rows_y(c) : (int)chain_rows_x(c);
  }
}

static int chain_layout(const mmnas_chain* c, ChainLayout& L) {
  size_t off = 0;
  auto take = [&](size_t bytes) { size_t r = off; off += al(bytes); return r; };
  L.last_x = L.last_y = L.first_x = L.first_y = -1;
  L.n_guided = 0;
  int cur[2] = {-1, -1}, head = 0;   // per stream: who wrote its current state
  for (int i = 0; i < c->n_ops; ++i) {
    if (i > 0 && (!c->mixed || c->ops[i].node != c->ops[i - 1].node)) { cur[c->ops[head].on_y ? 1 : 0] = head; head = i; }
    L.head[i] = head; L.src[i] = cur[c->ops[i].on_y ? 1 : 0];
    if (head != i) continue;   // (mixed chains: the streams' first / last markers refer to NODES, the first operator of each)
    if (c->ops[i].on_y) { if (L.first_y < 0) L.first_y = i; L.last_y = i; }
    else { if (L.first_x < 0) L.first_x = i; L.last_x = i; }
  }
  const size_t nx = chain_rows_x(c) * c->d * sizeof(float), ny = chain_rows_y(c) * c->d * sizeof(float);
  for (int i = 0; i < c->n_ops; ++i) {
    const mmnas_chain_op& o = c->ops[i];
    mmnas_att_op a; mmnas_mlp_op m;
    chain_op_shapes(c, i, a, m);
    mmnas_plan pl;
    int rc = o.kind == MMNAS_CHAIN_ATT ? mmnas_att_op_plan(&a, &pl) : mmnas_mlp_op_plan(&m, &pl);
    if (rc) return rc;
    const size_t n = o.on_y ? ny : nx;
    L.y[i] = take(n);
    L.save[i] = take(pl.save_bytes);
    L.ws[i] = take(pl.ws_bwd_bytes);
    L.dx[i] = take(n);
    const bool guided = o.kind == MMNAS_CHAIN_ATT && !(a.flags & MMNAS_F_SELF) && !(c->mixed && o.detached);
    L.tmp[i] = guided ? take(nx) : 0;   // (hoisted key / value source gradient of a guided operator: summed once, chain_guided_kv_bwd)
    L.n_guided += guided;
  }
  L.dpre = take(nx);
  L.encdy = take(nx);
  L.relws = take(mmnas_rel_multi_bwd_ws_floats(c->B, c->Sx > c->Sy ? c->Sx : c->Sy) * sizeof(float));
  L.mixws = 0;
  if (c->mixed) {
    int nodes = 0;
    for (int i = 0; i < c->n_ops; ++i) {
      const bool first = L.head[i] == i;
      L.nout[i] = first ? take(c->ops[i].on_y ? ny : nx) : 0;
      L.ndact[i] = first ? take(c->ops[i].on_y ? ny : nx) : 0;
      nodes += first;
    }
    // one partial-sum area per node: the gate-gradient reductions of the backward are issued as ONE launch at its end
    L.mixws = take((size_t)(nodes > 0 ? nodes : 1) * mmnas_mixed_sum_ws_floats() * sizeof(float));
  }
  // The image stream's live-row K-tile table and the live bits it is built from (mmnas_wgrad_live_table): in the input-gradient
  // block of the stream's FIRST operator / node, which no chain, plain or mixed, ever hands out -- chain_din, the only reader
  // of L.dx, returns dy_in for every operator whose node is the stream's first.  B Sy d floats hold the 2 ceil(B Sy / 32) + 1
  // words for every d >= 1.  (Not a block of its own: the planners' byte counts are pinned as part of the arena contract,
  // tests/test_abi.py.)
  L.ktab = L.first_y >= 0 ? L.dx[L.first_y] : 0;
  L.total = off;
  return MMNAS_OK;
}

// ---- one binding of an operator to the chain ----
// Operator i as the walkers use it: chain_op_shapes' fields, its saved block and its backward scratch from the arena and, on
// request, the layout of the two.  What turns a per-operator ChainLayout offset into a pointer lives between here and
// chain_bind_bwd: the walkers below name buffers by operator (mixed chains: by node = its first operator) only.
struct BoundOp {
  int i;
  bool att;                        // which of a / m is the operator
  mmnas_att_op a; mmnas_mlp_op m;
  AttLayout al; MlpLayout ml;      // (chain_bind with layouts = true)
  float* y;                        // the operator's own output block (plain chains: chain_out picks x_out / y_out for a stream's last)
  const int* ktab;                 // backward, image-stream operators (mixed chains: the sampled candidate): the live-row K-tile table (else NULL)
  int flags() const { return att ? a.flags : m.flags; }
  float eps() const { return att ? a.eps : m.eps; }
};
static inline float* chain_buf(const mmnas_chain* c, size_t off) { return (float*)((char*)c->arena + off); }
static void chain_bind(const mmnas_chain* c, const ChainLayout& L, int i, BoundOp& b, bool layouts = false) {
  b.i = i; b.att = c->ops[i].kind == MMNAS_CHAIN_ATT; b.ktab = nullptr;
  chain_op_shapes(c, i, b.a, b.m);
  b.y = chain_buf(c, L.y[i]);
  if (b.att) { b.a.save = chain_buf(c, L.save[i]); b.a.ws = chain_buf(c, L.ws[i]); if (layouts) b.al = att_layout(&b.a); }
  else { b.m.save = chain_buf(c, L.save[i]); b.m.ws = chain_buf(c, L.ws[i]); if (layouts) b.ml = mlp_layout(&b.m); }
}
// output buffer of operator i (mixed chains: of the node whose first operator is i)
static float* chain_out(const mmnas_chain* c, const ChainLayout& L, int i) {
  return i == L.last_x ? c->x_out : (i == L.last_y ? c->y_out : chain_buf(c, c->mixed ? L.nout[i] : L.y[i]));
}
// input of operator i: the previous output on its stream, or the chain's input
static const float* chain_in(const mmnas_chain* c, const ChainLayout& L, int i) {
  return L.src[i] >= 0 ? chain_out(c, L, L.src[i]) : (c->ops[i].on_y ? c->y_in : c->x_in);
}
// the FINAL language state: the key / value source of every guided operator
static const float* chain_x_final(const mmnas_chain* c, const ChainLayout& L) { return L.last_x >= 0 ? c->x_out : c->x_in; }
// input-gradient buffer of operator i (mixed chains: of its node, kept in the sampled candidate i's block).  L.dx[L.first_y] is
// never handed out here -- the image stream's first node writes dy_in -- and is TAKEN: it holds the live-row table (chain_layout)
static float* chain_din(const mmnas_chain* c, const ChainLayout& L, int i) {
  return L.head[i] == L.first_x ? c->dx_in : (L.head[i] == L.first_y ? c->dy_in : chain_buf(c, L.dx[i]));
}
// hoisted key / value source gradient of guided operator i; mixed chains: node i0's sampled-candidate output gradient and the
// k-th node's partial sums of the gate gradients
static float* chain_guided_tmp(const mmnas_chain* c, const ChainLayout& L, int i) { return chain_buf(c, L.tmp[i]); }
static float* chain_node_dact(const mmnas_chain* c, const ChainLayout& L, int i0) { return chain_buf(c, L.ndact[i0]); }
static float* chain_gate_ws(const mmnas_chain* c, const ChainLayout& L, int k) { return chain_buf(c, L.mixws) + (size_t)k * mmnas_mixed_sum_ws_floats(); }
// forward pointers: the input(s) and where the output goes
static void chain_bind_fwd(BoundOp& b, const mmnas_chain* c, const ChainLayout& L, float* out) {
  const float* in = chain_in(c, L, b.i);
  if (b.att) { b.a.xq = in; b.a.xkv = (b.a.flags & MMNAS_F_SELF) ? in : chain_x_final(c, L); b.a.y = out; }   // guided: keys / values from the FINAL language state
  else { b.m.x = in; b.m.y = out; }
}
// backward pointers: the input(s), the output gradient, where the input gradient goes (returned)
static float* chain_bind_bwd(BoundOp& b, const mmnas_chain* c, const ChainLayout& L, const float* dy) {
  const float* in = chain_in(c, L, b.i);
  float* dx = chain_din(c, L, b.i);
  if (b.att) {
    const bool self = b.a.flags & MMNAS_F_SELF;
    b.a.xq = in; b.a.xkv = self ? in : chain_x_final(c, L);
    b.a.dy = dy; b.a.dxq = dx;
    b.a.dxkv = self ? nullptr : chain_buf(c, L.dpre);     // guided: added into the chain's running sum (zeroed by chain_bwd_begin)
    b.a.drel = nullptr;
  } else { b.m.x = in; b.m.dy = dy; b.m.dx = dx; }
  return dx;
}
// one bound operator's launches.  Forward: *ln_done as att_fwd_impl reports it.  Backward: guided operators add into dxkv.
static int chain_run_fwd(const BoundOp& b, hipStream_t s, bool defer_ln, bool* ln_done, bool rel_ready, bool kv_ready) {
  return b.att ? att_fwd_impl(&b.a, s, defer_ln, ln_done, rel_ready, kv_ready) : mlp_fwd_impl(&b.m, s, defer_ln, ln_done);
}
static int chain_run_bwd(const BoundOp& b, hipStream_t s, SideQueue* sq, bool rel_defer, bool kv_defer, const AuxReduce* ln_pre = nullptr) {
  return b.att ? att_bwd_impl(&b.a, s, sq, !(b.a.flags & MMNAS_F_SELF), rel_defer, kv_defer, ln_pre, b.ktab) : mlp_bwd_impl(&b.m, s, sq, ln_pre, b.ktab);
}
// Where candidate i's LayerNorm runs, forward and backward (att_ln_place; an MLP candidate with a LayerNorm never normalises
// itself in a mixed chain: mlp_fwd_impl keeps the general path under defer_ln), and with it what the node epilogue reads for the
// candidate in EITHER direction: its pre-LayerNorm sum with the LayerNorm parameters, or -- no LayerNorm, or the operator's own
// forward normalised -- its output alone (*la = NULL).  b: bound with layouts.
static LnPlace chain_cand_view(const BoundOp& b, const float** z, const float** la, const float** lb) {
  LnPlace p = {false, false};
  if (b.att) p = att_ln_place(&b.a);
  if (!(b.flags() & MMNAS_F_NORM) || p.fwd) { *z = b.y; *la = nullptr; *lb = nullptr; }
  else if (b.att) { *z = b.al.z; *la = b.a.ln_a; *lb = b.a.ln_b; }
  else { *z = b.ml.z; *la = b.m.ln_a; *lb = b.m.ln_b; }
  return p;
}

// ---- live-row K-tile table of a padded batch's gradient rows ----
// The reference computes the padding rows and masks them as KEYS in every attention and in AttFlat, so the gradient that enters
// the decoder chain is exactly 0 on every padded row, and every operator a chain can hold keeps such a row at exactly 0 (the MLP
// family and LayerNorm work row by row; a zero dO row gives a zero dQ row, a masked key P = 0 and with it zero dK / dV rows).
// The weight gradients dW += dY^T X then reduce over rows that contribute exact zeros.  The table names the 32-row K-tiles that
// hold every live row -- greedy cover, the next tile starts on the first live row not yet covered -- and the split-K products walk
// only those (gemm.hip, mmnas_gemm_desc::ktab).  Dead rows are established from the data at every call: row r is dead iff its
// mask byte is set AND all d values are +-0 (sign bit cleared; NaN / Inf make a row live), so a caller whose gradient is not
// zero under the mask keeps those rows.
// One launch: wave w of the grid decides rows 32 w .. 32 w + 31 (the values of the masked rows only, 16-byte buffer loads with
// the unmasked rows' offsets out of range: no memory request) and publishes their live bits; the last workgroup to arrive
// (arrival counter of the stream's stream-K workspace, left at zero) walks the bit words with one wave: lane l holds rows
// 64 l .. 64 l + 63 and 4096 + 64 l .., every step is a readlane, a shift and a find-first-bit.
constexpr int LIVE_MAX_ROWS = 8192;
int sk_workspace(hipStream_t st, float** ws, size_t* ws_floats, int** cnt, int* ncnt);   // gemm.hip
typedef unsigned u32x4_t __attribute__((ext_vector_type(4)));

__global__ void __launch_bounds__(256) wgrad_live_kernel(const float* __restrict__ dy, const uint8_t* __restrict__ mask, const int M, const int d,
                                                         int* __restrict__ tab, unsigned* __restrict__ bits, const int nwords, int* __restrict__ cnt) {
  __shared__ int s_last;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int w = blockIdx.x * 4 + wave;
  if (w < nwords) {
    const int r0 = w * 32;
    const int r = r0 + (lane & 31);
    const bool in = lane < 32 && r < M;
    const bool masked = in && mask[r] != 0;
    const unsigned need = (unsigned)__ballot(masked);            // rows whose values decide
    unsigned live = (unsigned)__ballot(in && !masked);
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)dy, 0, (unsigned)M * (unsigned)d * 4u, 0x00020000);
    for (int c0 = 0; c0 < d; c0 += 256) {
      const int col = c0 + lane * 4;
#pragma unroll
      for (int hb = 0; hb < 2; ++hb) {
        u32x4_t v[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int rr = hb * 16 + i;
          const bool ld = ((need >> rr) & 1u) != 0 && col < d;
          v[i] = __builtin_amdgcn_raw_buffer_load_b128(rs, ld ? (unsigned)((r0 + rr) * d + col) * 4u : ~0u, 0, 0);
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const bool nz = ((v[i].x | v[i].y | v[i].z | v[i].w) & 0x7fffffffu) != 0;
          if (__ballot(nz) != 0) live |= 1u << (hb * 16 + i);
        }
      }
    }
    if (lane == 0) __hip_atomic_store(bits + w, live, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the words have been written through ...
  __syncthreads();                                    // ... before the workgroup announces its arrival
  if (tid == 0) s_last = __hip_atomic_fetch_add(cnt, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (int)gridDim.x - 1;
  __syncthreads();
  if (!s_last || wave != 0) return;
  if (lane == 0) __hip_atomic_store(cnt, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // ready for the next launch
  unsigned wd[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int i = 2 * lane + (j & 1) + 128 * (j >> 1);
    wd[j] = i < nwords ? __hip_atomic_load(bits + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
  }
  int count = 0, pos = 0;
  while (pos < M) {
    const int wi = pos >> 6, sl = wi & 63;
    const unsigned lo = wi < 64 ? __builtin_amdgcn_readlane(wd[0], sl) : __builtin_amdgcn_readlane(wd[2], sl);
    const unsigned hi = wi < 64 ? __builtin_amdgcn_readlane(wd[1], sl) : __builtin_amdgcn_readlane(wd[3], sl);
    const unsigned long long m = (((unsigned long long)hi << 32) | lo) >> (pos & 63);
    if (m == 0) { pos = (wi + 1) << 6; continue; }
    const int r = pos + __builtin_ctzll(m);
    if (lane == 0) tab[1 + count] = r;
    ++count;
    pos = r + 32;
  }
  if (lane == 0) tab[0] = count;
}

static int live_table_launch(const float* dy, const uint8_t* mask, int M, int d, int* tab, hipStream_t st) {
  const int nwords = cdiv(M, 32);
  float* ws; size_t wsf; int* cnt; int ncnt;
  const int rc = sk_workspace(st, &ws, &wsf, &cnt, &ncnt);
  if (rc) return rc;
  MMNAS_LAUNCH(wgrad_live_kernel, dim3(cdiv(nwords, 4)), dim3(256), 0, st, dy, mask, M, d, tab, (unsigned*)(tab + 1 + nwords), nwords, cnt + ncnt - 1);
  return check_launch("wgrad_live_table");
}
static bool live_table_fits(long M, int d) { return M > 0 && M <= LIVE_MAX_ROWS && d > 0 && d % 4 == 0 && (double)M * d * 4.0 < 4.0e9; }

// ---- side stream + events, one set per (device, main stream) ----
struct SideCtx { hipStream_t side; hipStream_t enc; hipEvent_t ev[MMNAS_CHAIN_MAX_OPS + 2]; hipEvent_t ovl[4]; bool used; };
static std::mutex g_side_mu;
static std::map<std::pair<int, hipStream_t>, SideCtx> g_side;

static SideCtx* side_ctx(hipStream_t main, bool create) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return nullptr;
  std::lock_guard<std::mutex> lk(g_side_mu);
  auto key = std::make_pair(dev, main);
  auto it = g_side.find(key);
  if (it == g_side.end()) {
    if (!create) return nullptr;
    SideCtx s;
    memset(&s, 0, sizeof(s));
    // lowest priority: when both streams have workgroups to dispatch, the data-gradient chain goes first
    int least = 0, greatest = 0;
    const bool prio = sw::side_prio.get() &&
                      hipDeviceGetStreamPriorityRange(&least, &greatest) == hipSuccess && least != greatest;
    if ((prio ? hipStreamCreateWithPriority(&s.side, hipStreamNonBlocking, least)
              : hipStreamCreateWithFlags(&s.side, hipStreamNonBlocking)) != hipSuccess) return nullptr;
    for (auto& e : s.ev)
      if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return nullptr;
    // the language stream's own stream (chain overlap): highest priority -- its launches are a handful of workgroups on
    // a latency-bound chain and must not queue behind the image stream's thousand-workgroup launches
    if ((prio ? hipStreamCreateWithPriority(&s.enc, hipStreamNonBlocking, greatest)
              : hipStreamCreateWithFlags(&s.enc, hipStreamNonBlocking)) != hipSuccess) return nullptr;
    for (auto& e : s.ovl)
      if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return nullptr;
    it = g_side.emplace(key, s).first;
  }
  return &it->second;
}

// Encoder / decoder overlap.  The language stream's operators run on 896 rows: 56-224 workgroups per launch, ~10 us
// each whatever they compute, on a quarter of the CUs.  The image-stream operators in front of the FIRST guided
// operator do not read the language state, so forward they run beside the encoder, and backward the encoder's
// operators run beside theirs (every guided operator's gradient has reached the language state by then).
// MEASURED: no gain (5.746 vs 5.738 ms per supernet step, 12.15 vs 12.15 ms per training step).  A language-stream launch
// is resident on every CU for its whole latency-bound duration, and its LDS / wave slots cost the image stream's
// GEMM one of its three workgroups per CU meanwhile: in the trace the co-running kernels take 1.3-1.5x their solo time
// (GEMM 26.6 -> 39.6 us, attention 22 -> 32 us), which returns what the overlap saves.  Off by default
// (MMNAS_CHAIN_OVERLAP=1 enables it); kept because the fork / join structure is what a multi-stream caller needs.
static bool chain_overlap_on() { return sw::chain_overlap.get() != 0; }   // mmnas_set_chain_overlap() overrides
static bool head_overlap_on() { return sw::head_overlap.get() != 0; }
static bool head_glimpse1_on() { return sw::head_glimpse1.get() != 0; }   // 0: the one-glimpse logit layer as GEMM launches (A/B, tests); read per call
static bool head_projT_on() { return sw::head_projt.get() != 0; }         // 0: the answer projection's gradients from the untransposed loss gradient; read per call
static int first_guided(const mmnas_chain* c) {
  for (int i = 0; i < c->n_ops; ++i)
    if (c->ops[i].kind == MMNAS_CHAIN_ATT && !(c->ops[i].att.flags & MMNAS_F_SELF)) return i;
  return c->n_ops;
}
static int ev_fork(hipStream_t from, hipStream_t to, hipEvent_t e) {
  if (hipEventRecord(e, from) != hipSuccess || hipStreamWaitEvent(to, e, 0) != hipSuccess) {
    set_error("chain: event record / wait failed");
    return MMNAS_E_LAUNCH;
  }
  return MMNAS_OK;
}


// ---- relation bias of all lazy-handle relation operators of a stream in one launch per direction (relmulti.hip) ----
static bool rel_hoist_on() { return sw::rel_hoist.get() != 0; }   // default 1; mmnas_set_rel_hoist() overrides
struct RelGroups {
  std::vector<mmnas_rel_multi> groups[2];      // [0]: the language stream's, [1]: the image stream's
  bool hoisted[MMNAS_CHAIN_MAX_OPS];
  RelGroups() { memset(hoisted, 0, sizeof(hoisted)); }
};
// Which operators take part: attention operators with MMNAS_F_REL | MMNAS_F_RELRAW whose shape relmulti.hip covers; backward
// (bwd = true) only the differentiated ones.  Operators of one stream that share (raw, Wy, by, H, C) and the key mask form
// a group.  The mask is the one the operators' attention cores apply (att_core_desc): every core that reads a hoisted biasT --
// mha_fwd_kernel / mha_fwd_pair_kernel, mha_fwd_b16_kernel / mha_fwd_b16_two_kernel, mha_bwd_q_kernel, mha_bwd_kv_kernel,
// mha_bwd_fused_kernel, mha_bwd_b16_kernel -- adds the bias and then SELECTS -1e9 under a masked key (no arithmetic on the sum, the row maximum is
// taken behind the select), and every backward core writes the bias gradient there as a literal 0: the relation kernels
// leave the planes under the masked tail keys of a padded batch unwritten forward and unread backward (relmulti.hip).
static void chain_rel_groups(const mmnas_chain* c, const ChainLayout& L, bool bwd, RelGroups& G) {
  if (!rel_hoist_on() || c->use_side_stream) return;
  for (int i = 0; i < c->n_ops; ++i) {
    const mmnas_chain_op& o = c->ops[i];
    if (o.kind != MMNAS_CHAIN_ATT) continue;
    if (bwd && c->mixed && o.detached) continue;
    if (!(o.att.flags & MMNAS_F_REL) || !(o.att.flags & MMNAS_F_RELRAW) || !(o.att.flags & MMNAS_F_SELF)) continue;
    BoundOp b;
    chain_bind(c, L, i, b, true);
    const mmnas_att_op& a = b.a;
    const AttLayout& al_ = b.al;
    if (!mmnas_rel_multi_supported(a.C, a.R, a.H) || !a.rel || !a.Wy || !a.by) continue;
    if ((long)a.B * a.H * a.Sq * a.Sq >= (1l << 31)) continue;
    std::vector<mmnas_rel_multi>& gs = G.groups[o.on_y ? 1 : 0];
    mmnas_rel_multi* g = nullptr;
    const unsigned char* const kmask = (a.flags & MMNAS_F_MASK) ? (const unsigned char*)a.mask : nullptr;
    for (auto& q : gs)
      if (q.raw == a.rel && q.Wy == a.Wy && q.by == a.by && q.H == a.H && q.C == a.C && q.key_mask == kmask && q.n_ops < MMNAS_REL_MULTI_MAX) { g = &q; break; }
    if (!g) {
      mmnas_rel_multi q;
      memset(&q, 0, sizeof(q));
      q.B = a.B; q.S = a.Sq; q.C = a.C; q.R = a.R; q.H = a.H;
      q.raw = a.rel; q.Wy = a.Wy; q.by = a.by; q.dWy = a.dWy; q.dby = a.dby;
      q.off = a.q_off; q.tile_off = a.rel_tile_off; q.ntiles = a.rel_ntiles;
      q.key_mask = kmask;
      q.ws = chain_buf(c, L.relws);
      gs.push_back(q);
      g = &gs.back();
    }
    const int j = g->n_ops++;
    g->Wr[j] = a.Wr; g->br[j] = a.br; g->biasT[j] = al_.biasT; g->dbiasT[j] = al_.dbiasT; g->dWr[j] = a.dWr; g->dbr[j] = a.dbr;
    G.hoisted[i] = true;
  }
}
static int chain_rel_fwd(const RelGroups& G, hipStream_t st, int only = -1) {
  for (int s = 0; s < 2; ++s)
    if (only < 0 || only == s)
      for (const auto& g : G.groups[s]) { const int rc = mmnas_rel_multi_fwd(&g, st); if (rc) return rc; }
  return MMNAS_OK;
}
// The image stream's relation launches BESIDE the language stream's operators (round 5, MMNAS_REL_OVERLAP=1; OFF by default:
// MEASURED SLOWER -- supernet step 4.70 -> 4.81-4.88 ms, arch step 8.02 -> 8.21-8.25 ms, three alternations on one box: the
// fourth form of stream overlap tried on this path and the fourth that lost to the cross-stream event waits and to the
// co-running kernels slowing each other; kept because the fork / join structure is tested and documents the negative).  The
// encoder is a dependent chain of ~40 launches of 56-224 workgroups on 896 rows -- 0.25 ms forward, 0.35 ms backward during
// which most of the chip idles -- and the image stream's relation bias depends on nothing it computes: forward it is issued
// on the side stream at chain entry and joined in front of the first relation operator of the decoder; backward it is issued
// on the side stream behind the decoder's first operator (every bias gradient exists) and joined at the end of the call,
// while the encoder's backward runs on the caller's stream.  A bucket mark that covers the relation parameters is recorded
// on the side stream behind the launch (the side stream waited for the caller's stream first: the event covers both).
static bool rel_overlap_on() { return sw::rel_overlap.get() != 0; }
static int chain_rel_bwd(const RelGroups& G, int stream_y, hipStream_t st) {
  for (const auto& g : G.groups[stream_y]) {
    MMNAS_REQUIRE(g.dWy && g.dby, MMNAS_E_ARG, "chain_bwd: relation operators without the stem layer's gradient sinks");
    const int rc = mmnas_rel_multi_bwd(&g, st);
    if (rc) return rc;
  }
  return MMNAS_OK;
}


// ---- key / value projections of all guided operators of a chain in grouped launches ----
// Every GuidedAtt of a decoder reads the SAME key / value source -- the final language state (hygr_vqa.py:45-52: pre = x) --
// through its own Wk / Wv: M = B * Sx = 896 rows, 56 tiles per product, a quarter of a round of workgroups.  Forward: right
// behind the encoder, K_n = x Wk_n^T and V_n = x Wv_n^T of up to 4 operators per grouped launch (8 groups); each operator
// then projects only its queries.  Backward: behind the LAST guided operator's backward (the first in chain order), the
// key / value source gradients dxkv_n = dK_n Wk_n + dV_n Wv_n into per-operator buffers and dWk_n / dWv_n, 4 operators per
// gradient-pair launch; one add_many launch sums the buffers (and the head's gradient) into the encoder's output gradient.
static bool node_lnb_on() { return sw::node_lnb.get() != 0; }   // default 1: the sampled candidate's LayerNorm backward inside the node's mix kernel
static bool guided_hoist_on() { return sw::guided_hoist.get() != 0; }   // default 1
struct GuidedSet {
  int idx[MMNAS_CHAIN_MAX_OPS], n;
  bool hoisted[MMNAS_CHAIN_MAX_OPS];
  GuidedSet() : n(0) { memset(hoisted, 0, sizeof(hoisted)); }
};
constexpr int GUIDED_PER_LAUNCH = 4;   // 2 groups each of <= MMNAS_GEMM_MAX_GROUPS = 9
static void chain_guided_set(const mmnas_chain* c, bool bwd, bool allow, GuidedSet& G) {
  if (!allow || !guided_hoist_on() || c->use_side_stream) return;
  int di = -1;
  for (int i = 0; i < c->n_ops; ++i) {
    const mmnas_chain_op& o = c->ops[i];
    if (o.kind != MMNAS_CHAIN_ATT || (o.att.flags & MMNAS_F_SELF)) continue;
    if (bwd && c->mixed && o.detached) continue;
    if (di < 0) di = o.att.di;
    if (o.att.di != di || G.n >= ADD_MANY_MAX - 2) continue;   // (another head layout: that operator keeps its own launches)
    G.idx[G.n++] = i; G.hoisted[i] = true;
  }
  if (G.n < 2) { for (int j = 0; j < G.n; ++j) G.hoisted[G.idx[j]] = false; G.n = 0; }   // (one operator: nothing to merge)
}
static int chain_guided_kv_fwd(const mmnas_chain* c, const ChainLayout& L, const GuidedSet& G, hipStream_t st) {
  const float* x_final = chain_x_final(c, L);
  for (int j0 = 0; j0 < G.n; j0 += GUIDED_PER_LAUNCH) {
    const int n = G.n - j0 < GUIDED_PER_LAUNCH ? G.n - j0 : GUIDED_PER_LAUNCH;
    mmnas_gemm_desc g;
    for (int j = 0; j < n; ++j) {
      const int i = G.idx[j0 + j];
      BoundOp b;
      chain_bind(c, L, i, b, true);
      const mmnas_att_op& a = b.a;
      const AttLayout& al_ = b.al;
      if (j == 0) { gemm_init(g, MMNAS_GEMM_NT, a.di, c->d, c->d, c->d, a.di); g.ngroups = 2 * n; }
      mmnas_gemm_group* gg = g.g + 2 * j;
      memset(gg, 0, 2 * sizeof(*gg));
      gg[0].M = (int)al_.Mk; gg[0].A[0] = x_final; gg[0].B[0] = a.Wk; gg[0].C = al_.K;
      gg[1].M = (int)al_.Mk; gg[1].A[0] = x_final; gg[1].B[0] = a.Wv; gg[1].C = al_.V;
    }
    const int rc = mmnas_gemm(&g, st);
    if (rc) return rc;
  }
  return MMNAS_OK;
}
// behind the last guided operator's backward: per-operator key / value source gradients + dWk / dWv, then their sum (+ the
// head's gradient of the language state, when there is one) into `out`
static int chain_guided_kv_bwd(const mmnas_chain* c, const ChainLayout& L, const GuidedSet& G, const float* extra, const float* extra2,
                               float* out, hipStream_t st) {
  const float* x_final = chain_x_final(c, L);
  const float* srcs[ADD_MANY_MAX + 2];
  int ns = 0;
  if (extra) srcs[ns++] = extra;
  if (extra2) srcs[ns++] = extra2;
  for (int j0 = 0; j0 < G.n; j0 += GUIDED_PER_LAUNCH) {
    const int n = G.n - j0 < GUIDED_PER_LAUNCH ? G.n - j0 : GUIDED_PER_LAUNCH;
    mmnas_gemm_desc g, w;
    for (int j = 0; j < n; ++j) {
      const int i = G.idx[j0 + j];
      BoundOp b;
      chain_bind(c, L, i, b, true);
      const mmnas_att_op& a = b.a;
      const AttLayout& al_ = b.al;
      const int Mk = (int)al_.Mk, di = a.di, d = c->d;
      if (j == 0) {
        gemm_init(g, MMNAS_GEMM_NN, d, di, di, d, d); g.ngroups = n; g.nseg = 2;
        gemm_init(w, MMNAS_GEMM_TN, d, Mk, di, d, d); w.ngroups = 2 * n; w.accumulate = 1;
      }
      float* tmp = chain_guided_tmp(c, L, i);
      memset(&g.g[j], 0, sizeof(g.g[j]));
      g.g[j].M = Mk; g.g[j].C = tmp;
      g.g[j].A[0] = al_.dK; g.g[j].B[0] = a.Wk;
      g.g[j].A[1] = al_.dV; g.g[j].B[1] = a.Wv;
      memset(&w.g[2 * j], 0, 2 * sizeof(w.g[0]));
      w.g[2 * j].M = di; w.g[2 * j].A[0] = al_.dK; w.g[2 * j].B[0] = x_final; w.g[2 * j].C = a.dWk;
      w.g[2 * j + 1].M = di; w.g[2 * j + 1].A[0] = al_.dV; w.g[2 * j + 1].B[0] = x_final; w.g[2 * j + 1].C = a.dWv;
      srcs[ns++] = tmp;
    }
    const int rc = mmnas_gemm_pair(&g, &w, st);
    if (rc) return rc;
  }
  return add_many(srcs, ns, out, chain_rows_x(c) * c->d, st);
}

}  // namespace mmnas

extern "C" int mmnas_set_rel_overlap(int on) { return mmnas::sw::rel_overlap.set(on != 0); }
extern "C" int mmnas_set_guided_hoist(int on) { return mmnas::sw::guided_hoist.set(on != 0); }
extern "C" int mmnas_set_rel_hoist(int on) { return mmnas::sw::rel_hoist.set(on != 0); }
extern "C" int mmnas_set_chain_overlap(int on) { return mmnas::sw::chain_overlap.set(on != 0); }

extern "C" int mmnas_set_wgrad_live(int on) { return sw::wgrad_live.set(on != 0); }
extern "C" int mmnas_wgrad_live_table_ints(int M) { return M > 0 ? 2 * cdiv(M, 32) + 1 : 1; }
extern "C" int mmnas_wgrad_live_table(const float* dy, const unsigned char* mask, int M, int d, int* tab, void* stream) {
  MMNAS_REQUIRE(dy && mask && tab, MMNAS_E_ARG, "wgrad_live_table: null pointer");
  MMNAS_REQUIRE(live_table_fits(M, d), MMNAS_E_SHAPE, "wgrad_live_table: M=%d (1..%d) d=%d (a multiple of 4)", M, LIVE_MAX_ROWS, d);
  return live_table_launch(dy, mask, M, d, tab, (hipStream_t)stream);
}

extern "C" int mmnas_chain_plan(const mmnas_chain* c, size_t* arena_bytes) {
  int rc = chain_check(c, "chain_plan");
  if (rc) return rc;
  MMNAS_REQUIRE(arena_bytes, MMNAS_E_ARG, "chain_plan: null output");
  ChainLayout L;
  if ((rc = chain_layout(c, L))) return rc;
  *arena_bytes = L.total;
  return MMNAS_OK;
}

namespace mmnas {
// ---- the stream steps both walkers take: mmnas_chain_fwd / _bwd name them by operator, chain_fwd_mixed / chain_bwd_mixed by
// node (= its first operator) ----
// Forward, chain entry: every hoisted relation bias.  may_fork and MMNAS_REL_OVERLAP: the image stream's on the side stream
// beside the encoder (see rel_overlap_on); *forked is then that stream's context, and the caller joins it (chain_rel_join) in
// front of the first decoder operator / node that reads a hoisted bias.
static int chain_rel_prologue(const mmnas_chain* c, const ChainLayout& L, const RelGroups& RG, hipStream_t st, bool may_fork, SideCtx** forked) {
  SideCtx* rsc = (may_fork && rel_overlap_on() && !RG.groups[1].empty() && L.last_x >= 0 && L.first_y >= 0) ? side_ctx(st, true) : nullptr;
  *forked = rsc;
  if (!rsc) return chain_rel_fwd(RG, st);
  int rc;
  if ((rc = ev_fork(st, rsc->side, rsc->ovl[0]))) return rc;
  if ((rc = chain_rel_fwd(RG, rsc->side, 1))) return rc;
  return chain_rel_fwd(RG, st, 0);
}
static int chain_rel_join(SideCtx* rsc, hipStream_t st) { return ev_fork(rsc->side, st, rsc->ovl[1]); }   // the image stream's bias exists from here on
// Forward, chain exit: a stream without operators hands its input on
static int chain_fwd_passthrough(const mmnas_chain* c, const ChainLayout& L, hipStream_t st) {
  const size_t nx = chain_rows_x(c) * c->d * sizeof(float), ny = chain_rows_y(c) * c->d * sizeof(float);
  if (L.last_x < 0 && hipMemcpyAsync(c->x_out, c->x_in, nx, hipMemcpyDeviceToDevice, st) != hipSuccess) return MMNAS_E_LAUNCH;
  if (L.last_y < 0 && hipMemcpyAsync(c->y_out, c->y_in, ny, hipMemcpyDeviceToDevice, st) != hipSuccess) return MMNAS_E_LAUNCH;
  return MMNAS_OK;
}

// What a backward walk carries from step to step.
struct ChainBwd {
  const mmnas_chain* c; const ChainLayout* L;
  hipStream_t st;       // the caller's stream
  SideQueue* sq;        // plain chains with a side stream: the queued parameter-gradient work (else NULL)
  RelGroups RG;         // relation operators whose bias gradient waits for the one launch behind their stream's first operator / node
  GuidedSet GS;         // guided operators whose dK / dV wait for the grouped launches behind the first of them in chain order
  int G;                // ... that operator: the last hoisted guided operator in backward order (-1: none)
  float *dpre, *encdy;  // running sum of the unhoisted guided operators' key / value source gradients; the encoder's output gradient
  size_t ex;
  const float* enc_grad = nullptr;   // set by the hoisted launch: the encoder's output gradient, complete
  SideCtx* rel_bwd_side = nullptr;   // set when the image stream's relation backward went to the side stream: joined below
  const int* ktab = nullptr;         // live-row K-tile table of the image stream's gradient rows (chain_live_table); NULL: dense
};
// The chain's table (plain and mixed chains), or NULL (*out) where the dense walk stays: no mask, the ragged stream, no
// image-stream operator, a shape the kernel does not take, MMNAS_WGRAD_LIVE=0.
static int chain_live_table(const mmnas_chain* c, const ChainLayout& L, hipStream_t st, const int** out) {
  *out = nullptr;
  if (!c->y_mask || c->y_off || L.first_y < 0 || !sw::wgrad_live.get() || !live_table_fits((long)c->B * c->Sy, c->d)) return MMNAS_OK;
  int* tab = (int*)chain_buf(c, L.ktab);
  const int rc = live_table_launch(c->dy_out, c->y_mask, c->B * c->Sy, c->d, tab, st);
  if (!rc) *out = tab;
  return rc;
}
// hoist: relation and guided hoists allowed (not under the encoder / decoder overlap of a plain chain)
static int chain_bwd_begin(ChainBwd& S, const mmnas_chain* c, const ChainLayout& L, hipStream_t st, SideQueue* sq, bool hoist) {
  S.c = c; S.L = &L; S.st = st; S.sq = sq;
  S.dpre = chain_buf(c, L.dpre); S.encdy = chain_buf(c, L.encdy);
  S.ex = chain_rows_x(c) * c->d;
  // before any operator's backward launch, on the caller's stream: a side stream's queued products run behind an event that
  // this stream records later
  if (int r = chain_live_table(c, L, st, &S.ktab)) return r;
  if (hoist) chain_rel_groups(c, L, true, S.RG);
  chain_guided_set(c, true, hoist, S.GS);
  S.G = -1;
  for (int i = 0; i < c->n_ops && S.G < 0; ++i)
    if (S.GS.hoisted[i]) S.G = i;
  if (L.n_guided > S.GS.n && hipMemsetAsync(S.dpre, 0, S.ex * sizeof(float), st) != hipSuccess) return MMNAS_E_LAUNCH;
  return MMNAS_OK;
}
// entering the encoder: its output gradient = the head's + the guided operators'
static int chain_enc_dy(ChainBwd& S, hipStream_t s, const float** out) {
  const mmnas_chain* c = S.c;
  MMNAS_REQUIRE(c->dx_out || S.L->n_guided, MMNAS_E_ARG, "chain_bwd: no gradient reaches the encoder (dx_out NULL, no guided operator)");
  if (S.enc_grad) { *out = S.enc_grad; return MMNAS_OK; }
  if (c->dx_out && S.L->n_guided) {
    const int r = mmnas_drop_add(c->dx_out, S.dpre, S.encdy, S.ex, 0.f, 0, 0, s);
    if (r) return r;
    *out = S.encdy;
  } else *out = c->dx_out ? c->dx_out : S.dpre;
  return MMNAS_OK;
}
// behind operator i's backward: when it is the last hoisted guided operator in backward order, every hoisted dK / dV exists
static int chain_guided_release(ChainBwd& S, int i, hipStream_t s) {
  if (!S.GS.n || i != S.G) return MMNAS_OK;
  const int r = chain_guided_kv_bwd(S.c, *S.L, S.GS, S.c->dx_out, S.GS.n < S.L->n_guided ? S.dpre : nullptr, S.encdy, s);
  if (!r) S.enc_grad = S.encdy;
  return r;
}
// Behind the backward of operator / node i, issued on stream s.  A stream's first operator is its last in backward order: every
// relation operator's bias gradient exists now -- before operator `mark`'s mark event (mark < 0: none), which covers the relation
// parameters, see nets._chain.
static int chain_first_done(ChainBwd& S, int i, int mark, hipStream_t s) {
  const mmnas_chain* c = S.c; const ChainLayout& L = *S.L;
  int r;
  hipStream_t mark_stream = s;
  if (i == L.first_y && !S.RG.groups[1].empty()) {
    SideCtx* rsc = (rel_overlap_on() && L.last_x >= 0 && !S.sq) ? side_ctx(S.st, true) : nullptr;
    if (rsc) {   // beside the encoder's backward (see rel_overlap_on); joined at the end of the call
      if ((r = ev_fork(s, rsc->side, rsc->ovl[2]))) return r;
      if ((r = chain_rel_bwd(S.RG, 1, rsc->side))) return r;
      S.rel_bwd_side = rsc;
      mark_stream = rsc->side;
    } else if ((r = chain_rel_bwd(S.RG, 1, s))) return r;
  }
  if (i == L.first_x && !S.RG.groups[0].empty()) {
    // (every relation group shares ONE partial-row workspace: the image stream's launches on the side stream are joined
    //  before the language stream's write into it -- ADVICE r5; the join at the end of the call then finds nothing pending)
    if (S.rel_bwd_side) { if ((r = ev_fork(S.rel_bwd_side->side, s, S.rel_bwd_side->ovl[3]))) return r; S.rel_bwd_side = nullptr; }
    if ((r = chain_rel_bwd(S.RG, 0, s))) return r;
  }
  if (mark >= 0 && c->marks && c->marks[mark] && hipEventRecord((hipEvent_t)c->marks[mark], mark_stream) != hipSuccess) {
    set_error("chain_bwd: cannot record the mark event of operator %d", mark);
    return MMNAS_E_LAUNCH;
  }
  return MMNAS_OK;
}
// mixed chains: every node's pending gate-gradient reduction -- ONE launch at the end of the backward
struct GateReds {
  const float* part[MMNAS_CHAIN_MAX_OPS]; float* out[MMNAS_CHAIN_MAX_OPS]; int nwg[MMNAS_CHAIN_MAX_OPS], width[MMNAS_CHAIN_MAX_OPS];
  int n = 0;
};
// chain exit: the last side-stream join, the gate gradients (reds: mixed chains), the input gradients of a stream without operators
static int chain_bwd_close(ChainBwd& S, const GateReds* reds) {
  const mmnas_chain* c = S.c; const ChainLayout& L = *S.L;
  hipStream_t st = S.st;
  int rc;
  if (S.rel_bwd_side && (rc = ev_fork(S.rel_bwd_side->side, st, S.rel_bwd_side->ovl[3]))) return rc;   // the relation gradients are in
  if (reds && reds->n && (rc = mixed_reduce_many(reds->part, reds->out, reds->nwg, reds->width, reds->n, st))) return rc;   // every node's gate gradients
  if (L.first_y < 0 && hipMemcpyAsync(c->dy_in, c->dy_out, chain_rows_y(c) * c->d * sizeof(float), hipMemcpyDeviceToDevice, st) != hipSuccess)
    return MMNAS_E_LAUNCH;
  if (L.first_x < 0) {
    const float* g0 = c->dx_out;
    if (S.enc_grad) g0 = S.enc_grad;
    else if (c->dx_out && L.n_guided) {
      if ((rc = mmnas_drop_add(c->dx_out, S.dpre, c->dx_in, S.ex, 0.f, 0, 0, st))) return rc;
      g0 = nullptr;
    } else if (!c->dx_out) g0 = S.dpre;
    if (g0 && hipMemcpyAsync(c->dx_in, g0, S.ex * sizeof(float), hipMemcpyDeviceToDevice, st) != hipSuccess) return MMNAS_E_LAUNCH;
  }
  return MMNAS_OK;
}

// ---- mixed chains: the architecture step (MixedOp modes 'full' / 'two') ----
// Per node: every evaluated candidate's forward up to its pre-LayerNorm sum, then ONE epilogue launch that normalises
// all of them and forms the gated node output (mmnas_node_mix_fwd).  Backward: one launch turns the node's output
// gradient into the gate gradients of all candidates (their outputs recomputed from the saved sums) and the sampled
// candidate's output gradient; only that candidate's backward runs.
static int chain_fwd_mixed(const mmnas_chain* c, hipStream_t st, const ChainLayout& L) {
  int rc;
  RelGroups RG;     // every relation candidate's bias (18 in the VQA search space) before the first node
  chain_rel_groups(c, L, false, RG);
  SideCtx* rsc = nullptr;   // the image stream's candidates beside the encoder nodes; joined in front of the first decoder node
  if ((rc = chain_rel_prologue(c, L, RG, st, true, &rsc))) return rc;
  for (int i0 = 0; i0 < c->n_ops;) {
    int i1 = i0;
    while (i1 < c->n_ops && c->ops[i1].node == c->ops[i0].node) ++i1;
    if (rsc && i0 == L.first_y && (rc = chain_rel_join(rsc, st))) return rc;
    BoundOp cand[MMNAS_MIXED_MAX];   // the node's candidates: each writes its own block, the epilogue the node's output
    for (int i = i0; i < i1; ++i) {
      chain_bind(c, L, i, cand[i - i0], true);
      chain_bind_fwd(cand[i - i0], c, L, cand[i - i0].y);
    }
    // The node's attention candidates on the general path run stage by stage, each stage ONE launch for all of them: their
    // Q / K / V projections (up to 9 groups: same N = d_inside, K = d), their cores, their merge projections (own dropout
    // seed per group).  3 + 3 launches -> 1 + 1 per decoder node of the VQA search space (self / relation / guided).
    const BoundOp* g[MMNAS_MIXED_MAX];
    int ng = 0;
    for (int i = i0; i < i1; ++i) {
      const BoundOp& b = cand[i - i0];
      if (!b.att || att_ln_place(&b.a).fwd) continue;
      if (ng > 0) {
        const mmnas_att_op& f = g[0]->a;
        const bool d0 = drops(&f), d1 = drops(&b.a);
        if (b.a.di != f.di || ((b.a.flags ^ f.flags) & MMNAS_F_RESIDUAL) || d0 != d1 || (d0 && b.a.drop_p != f.drop_p)) continue;
      }
      if (3 * (ng + 1) > MMNAS_GEMM_MAX_GROUPS) continue;
      if ((rc = att_fwd_args(&b.a))) return rc;
      g[ng++] = &b;
    }
    if (ng < 2) ng = 0;   // (a single one takes the per-operator route below)
    if (ng) {
      const mmnas_att_op& f = g[0]->a;
      mmnas_gemm_desc gd;
      gemm_init(gd, MMNAS_GEMM_NT, f.di, c->d, c->d, c->d, f.di);
      gd.ngroups = 3 * ng;
      for (int j = 0; j < ng; ++j) att_qkv_groups(&g[j]->a, g[j]->al, gd.g + 3 * j);
      if ((rc = mmnas_gemm(&gd, st))) return rc;
      {   // the cores: two of one geometry (self / relation-self) share a launch, the rest one by one
        mmnas_mha_desc md[MMNAS_MIXED_MAX];
        for (int j = 0; j < ng; ++j)
          if ((rc = att_core_fwd(&g[j]->a, g[j]->al, st, &md[j], RG.hoisted[g[j]->i]))) return rc;   // (relation biases first, unless hoisted)
        bool done[MMNAS_MIXED_MAX] = {false};
        for (int j = 0; j < ng; ++j) {
          if (done[j]) continue;
          int mate = -1;
          for (int q = j + 1; q < ng && mate < 0; ++q)
            if (!done[q] && md[q].Sq == md[j].Sq && md[q].Sk == md[j].Sk && md[q].H == md[j].H && md[q].dh == md[j].dh) mate = q;
          if (mate >= 0) { if ((rc = mha_core_fwd_pair(&md[j], &md[mate], st))) return rc; done[mate] = true; }
          else if ((rc = mmnas_mha_core_fwd(&md[j], st))) return rc;
          done[j] = true;
        }
      }
      gemm_init(gd, MMNAS_GEMM_NT, c->d, f.di, f.di, f.di, c->d);
      gd.ngroups = ng;
      for (int j = 0; j < ng; ++j) att_merge_group(&g[j]->a, g[j]->al, &gd.g[j]);
      if (f.flags & MMNAS_F_RESIDUAL) gd.ldres = c->d;
      if (drops(&f)) { gd.drop_p = f.drop_p; gd.drop_site = 1; gd.drop_seed = f.seed; }
      if ((rc = mmnas_gemm(&gd, st))) return rc;
    }
    // the remaining candidates one by one, and what the epilogue reads for each.  The gate values of the node's candidates are a
    // row of the [n_nodes, width] block picked apart by candidate index -- the kernel reads gate[j] for entry j, so the
    // candidates are passed in candidate order
    // (candidates of the node that were not evaluated -- mode 'two' -- stay NULL: no term in the sum, no gate gradient)
    const float* zs[MMNAS_MIXED_MAX] = {nullptr}; const float* as[MMNAS_MIXED_MAX] = {nullptr}; const float* bs[MMNAS_MIXED_MAX] = {nullptr};
    int width = 0;
    float eps = 1e-6f;
    for (int i = i0; i < i1; ++i) {
      const BoundOp& b = cand[i - i0];
      bool staged = false;
      for (int j = 0; j < ng; ++j) staged |= g[j] == &b;
      // (who normalised is not asked of the launch: att_fwd_impl and chain_cand_view take the same att_ln_place answer; a staged
      //  candidate never normalises itself -- NORM: the node epilogue does; otherwise the merge product wrote the output)
      bool ln_done;
      if (!staged && (rc = chain_run_fwd(b, st, true, &ln_done, RG.hoisted[i], false))) return rc;
      if (b.flags() & MMNAS_F_NORM) eps = b.eps();
      const int k = c->ops[i].cand;
      chain_cand_view(b, &zs[k], &as[k], &bs[k]);
      if (k + 1 > width) width = k + 1;
    }
    const int M = c->ops[i0].on_y ? (int)chain_rows_y(c) : (int)chain_rows_x(c);
    if ((rc = mmnas_node_mix_fwd(zs, as, bs, width, c->gate + (size_t)c->ops[i0].node * c->gate_width, chain_out(c, L, i0), M, c->d, eps, st))) return rc;
    i0 = i1;
  }
  return chain_fwd_passthrough(c, L, st);
}

static int chain_bwd_mixed(const mmnas_chain* c, hipStream_t st, const ChainLayout& L) {
  MMNAS_REQUIRE(c->dgate, MMNAS_E_ARG, "chain_bwd: mixed chain without a gate-gradient block");
  int rc;
  ChainBwd S;       // the sampled relation / guided candidates are the hoisted ones
  if ((rc = chain_bwd_begin(S, c, L, st, nullptr, true))) return rc;
  GateReds reds;
  // node starts in order
  int starts[MMNAS_CHAIN_MAX_OPS + 1], nn = 0;
  for (int i = 0; i < c->n_ops; ++i)
    if (L.head[i] == i) starts[nn++] = i;
  starts[nn] = c->n_ops;
  const float* cur_dy = c->dy_out;
  for (int k = nn - 1; k >= 0; --k) {
    const int i0 = starts[k], i1 = starts[k + 1];
    if (i0 == L.last_x && (rc = chain_enc_dy(S, st, &cur_dy))) return rc;
    BoundOp cand[MMNAS_MIXED_MAX];
    const float* zs[MMNAS_MIXED_MAX] = {nullptr}; const float* as[MMNAS_MIXED_MAX] = {nullptr}; const float* bs[MMNAS_MIXED_MAX] = {nullptr};
    int width = 0, act = -1, act_op = -1;
    LnPlace act_ln = {false, false};
    float eps = 1e-6f;
    for (int i = i0; i < i1; ++i) {
      BoundOp& b = cand[i - i0];
      chain_bind(c, L, i, b, true);
      const int kc = c->ops[i].cand;
      const LnPlace p = chain_cand_view(b, &zs[kc], &as[kc], &bs[kc]);
      if (kc + 1 > width) width = kc + 1;
      if (!c->ops[i].detached) { act = kc; act_op = i; act_ln = p; }
      if (b.flags() & MMNAS_F_NORM) eps = b.eps();
    }
    float* dact = chain_node_dact(c, L, i0);
    const int M = c->ops[i0].on_y ? (int)chain_rows_y(c) : (int)chain_rows_x(c);
    const size_t grow = (size_t)c->ops[i0].node * c->gate_width;
    // The sampled candidate: its descriptor first -- its LayerNorm backward rides in the node's mix kernel (round 6) when the
    // epilogue's view carries the candidate's LayerNorm parameters, i.e. its own forward did not normalise, and the candidate
    // does not take the one-launch short-sequence backward, which does its own.  Otherwise the mix kernel hands on the
    // gradient of the candidate's output and the candidate's backward starts at its LayerNorm.
    BoundOp& b = cand[act_op - i0];
    if (c->ops[act_op].on_y) b.ktab = S.ktab;   // (the node's mix kernel and its LayerNorm backward work row by row: dead rows stay +-0)
    float* dx = chain_bind_bwd(b, c, L, dact);
    NodeLnBwd lnb;
    lnb.dz = nullptr;
    AuxReduce lnpre;
    lnpre.part = nullptr;
    if (node_lnb_on() && c->d <= 256 && as[act] && !act_ln.bwd) {
      const bool drop = b.att ? drops(&b.a) : drops(&b.m);
      lnb.dz = b.att ? b.al.dz : b.ml.dz; lnb.dt = !drop ? nullptr : (b.att ? b.al.dt : b.ml.dt); lnb.part = b.att ? b.al.lnws : b.ml.lnws;
      lnb.drop = make_drop(drop ? (b.att ? b.a.drop_p : b.m.drop_p) : 0.f, b.att ? b.a.seed : b.m.seed, 1);
      lnpre.part = lnb.part; lnpre.d = c->d;
      lnpre.out[0] = b.att ? b.a.dln_a : b.m.dln_a; lnpre.out[1] = b.att ? b.a.dln_b : b.m.dln_b;
      lnpre.out[2] = (!b.att && drop && b.m.db[b.m.nl - 1]) ? b.m.db[b.m.nl - 1] : nullptr;   // (the last layer's bias gradient among the partial rows)
    }
    {
      float* wsk = chain_gate_ws(c, L, k);
      int nwg = 0;
      if ((rc = node_mix_bwd_impl(zs, as, bs, width, c->gate + grow, cur_dy, dact, act, c->dgate + grow, wsk, M, c->d, eps, st, false, &nwg,
                                  lnb.dz ? &lnb : nullptr)))
        return rc;
      if (nwg > 0) { reds.part[reds.n] = wsk; reds.out[reds.n] = c->dgate + grow; reds.nwg[reds.n] = nwg; reds.width[reds.n] = width; ++reds.n; }
      lnpre.nrows = nwg;
    }
    // the sampled candidate's backward
    if ((rc = chain_run_bwd(b, st, nullptr, S.RG.hoisted[act_op], S.GS.hoisted[act_op], lnb.dz ? &lnpre : nullptr))) return rc;
    if ((rc = chain_guided_release(S, act_op, st))) return rc;
    cur_dy = dx;
    if ((rc = chain_first_done(S, i0, act_op, st))) return rc;
  }
  return chain_bwd_close(S, &reds);
}
}  // namespace mmnas

extern "C" int mmnas_chain_fwd(const mmnas_chain* c, void* stream) {
  int rc = chain_check(c, "chain_fwd");
  if (rc) return rc;
  MMNAS_REQUIRE(c->x_in && c->y_in && c->x_out && c->y_out && c->arena, MMNAS_E_ARG, "chain_fwd: null pointer");
  hipStream_t st = (hipStream_t)stream;
  ChainLayout L;
  if ((rc = chain_layout(c, L))) return rc;
  if (c->mixed) return chain_fwd_mixed(c, st, L);
  RelGroups RG;     // the relation bias of every relation operator of the chain: one launch per stream, here
  chain_rel_groups(c, L, false, RG);
  const int G = first_guided(c);
  const bool ovl = chain_overlap_on() && !c->use_side_stream && L.last_x >= 0 && L.first_y >= 0 && G > L.first_y;
  // the image stream's bias beside the encoder (see rel_overlap_on): joined in front of the decoder's first relation operator
  SideCtx* rsc = nullptr;
  if ((rc = chain_rel_prologue(c, L, RG, st, !ovl, &rsc))) return rc;
  int rel_join_at = -1;
  for (int i = L.first_y; rsc && i < c->n_ops && rel_join_at < 0; ++i)
    if (RG.hoisted[i] && c->ops[i].on_y) rel_join_at = i;
  GuidedSet GS;
  chain_guided_set(c, false, !ovl, GS);
  auto run = [&](int i, hipStream_t s) -> int {
    BoundOp b;
    chain_bind(c, L, i, b);
    chain_bind_fwd(b, c, L, chain_out(c, L, i));
    bool done;
    return chain_run_fwd(b, s, false, &done, RG.hoisted[i], GS.hoisted[i]);
  };
  if (!ovl) {
    for (int i = 0; i < c->n_ops; ++i) {
      // the final language state exists: key / value projections of every guided operator (grouped launches)
      if (GS.n && i == G && (rc = chain_guided_kv_fwd(c, L, GS, st))) return rc;
      if (i == rel_join_at && (rc = chain_rel_join(rsc, st))) return rc;
      if ((rc = run(i, st))) return rc;
    }
  } else {
    SideCtx* sc = side_ctx(st, true);
    MMNAS_REQUIRE(sc, MMNAS_E_LAUNCH, "chain_fwd: cannot create the encoder stream");
    if ((rc = ev_fork(st, sc->enc, sc->ovl[0]))) return rc;
    // encoder operators [first_x, last_x] on their own stream, the decoder's [first_y, G) on the caller's: issued alternately
    int ie = L.first_x, id = L.first_y;
    while (ie <= L.last_x || id < G) {
      if (ie <= L.last_x && (rc = run(ie++, sc->enc))) return rc;
      if (id < G && (rc = run(id++, st))) return rc;
    }
    if ((rc = ev_fork(sc->enc, st, sc->ovl[1]))) return rc;   // the final language state exists from here on
    for (int i = G; i < c->n_ops; ++i)
      if ((rc = run(i, st))) return rc;
  }
  return chain_fwd_passthrough(c, L, st);
}

extern "C" int mmnas_chain_bwd(const mmnas_chain* c, void* stream) {
  int rc = chain_check(c, "chain_bwd");
  if (rc) return rc;
  MMNAS_REQUIRE(c->x_in && c->y_in && c->x_out && c->y_out && c->arena && c->dy_out && c->dx_in && c->dy_in, MMNAS_E_ARG,
                "chain_bwd: null pointer");
  hipStream_t st = (hipStream_t)stream;
  ChainLayout L;
  if ((rc = chain_layout(c, L))) return rc;
  if (c->mixed) return chain_bwd_mixed(c, st, L);
  SideCtx* sc = c->use_side_stream ? side_ctx(st, true) : nullptr;
  MMNAS_REQUIRE(!c->use_side_stream || sc, MMNAS_E_LAUNCH, "chain_bwd: cannot create the side stream");
  hipStream_t side = sc ? sc->side : nullptr;
  if (sc) sc->used = true;
  SideQueue q;
  q.rel_only = c->use_side_stream == 2;
  SideQueue* sq = sc ? &q : nullptr;
  // When the queued parameter-gradient work is released: MMNAS_SIDE_FLUSH=op -> behind every operator (it then competes
  // with the data-gradient chain for the CUs); default -> once behind the decoder and once behind the encoder, so it
  // fills the latency-bound tail of the backward pass (encoder on 896 rows, LSTM, stem) instead.
  // (get(): the row records that it was read, so mmnas_switch_info reports it as it reports every cached switch)
  static const bool per_op = sw::side_flush.get() && !strcmp(getenv(sw::side_flush.name), "op");
  const int G = first_guided(c);
  const bool ovl = chain_overlap_on() && !c->use_side_stream && L.last_x >= 0 && L.first_y >= 0 && G > L.first_y;
  ChainBwd S;
  if ((rc = chain_bwd_begin(S, c, L, st, sq, !ovl))) return rc;
  // one operator's backward on stream s: gradient of its output in, gradient of its input out (returned through *dxo)
  auto run = [&](int i, hipStream_t s, const float* dyi, const float** dxo) -> int {
    BoundOp b;
    chain_bind(c, L, i, b);
    if (c->ops[i].on_y) b.ktab = S.ktab;
    float* dx = chain_bind_bwd(b, c, L, dyi);
    int r;
    if ((r = chain_run_bwd(b, s, sq, S.RG.hoisted[i], S.GS.hoisted[i]))) return r;
    if ((r = chain_guided_release(S, i, s))) return r;
    *dxo = dx;
    // (encoder / decoder overlap: an event behind operator i on ONE of the two streams says nothing about the operators
    //  with larger indices still running on the other -- the marks are recorded behind the join below instead)
    return chain_first_done(S, i, ovl ? -1 : i, s);
  };
  const float* cur_dy = c->dy_out;
  if (!ovl) {
    for (int i = c->n_ops - 1; i >= 0; --i) {
      if (sq && i == L.last_x && (rc = q.flush(st, side, sc->ev[0]))) return rc;   // the decoder's parameter-gradient work
      if (i == L.last_x && (rc = chain_enc_dy(S, st, &cur_dy))) return rc;
      if ((rc = run(i, st, cur_dy, &cur_dy))) return rc;
      if (sq && per_op && (rc = q.flush(st, side, sc->ev[i + 1]))) return rc;
    }
    if (sq && (rc = q.flush(st, side, sc->ev[1]))) return rc;
  } else {
    SideCtx* oc = side_ctx(st, true);
    MMNAS_REQUIRE(oc, MMNAS_E_LAUNCH, "chain_bwd: cannot create the encoder stream");
    for (int i = c->n_ops - 1; i >= G; --i)        // every guided operator is in here: the language state's gradient completes
      if ((rc = run(i, st, cur_dy, &cur_dy))) return rc;
    if ((rc = ev_fork(st, oc->enc, oc->ovl[2]))) return rc;
    const float* enc_dy = nullptr;
    if ((rc = chain_enc_dy(S, oc->enc, &enc_dy))) return rc;
    int ie = L.last_x, id = G - 1;
    while (ie >= L.first_x || id >= L.first_y) {    // encoder on its stream beside the decoder's leading operators
      if (ie >= L.first_x && (rc = run(ie--, oc->enc, enc_dy, &enc_dy))) return rc;
      if (id >= L.first_y && (rc = run(id--, st, cur_dy, &cur_dy))) return rc;
    }
    if ((rc = ev_fork(oc->enc, st, oc->ovl[3]))) return rc;
    if (c->marks)
      for (int i = 0; i < c->n_ops; ++i)
        if (c->marks[i] && hipEventRecord((hipEvent_t)c->marks[i], st) != hipSuccess) {
          set_error("chain_bwd: cannot record the mark event of operator %d", i);
          return MMNAS_E_LAUNCH;
        }
  }
  return chain_bwd_close(S, nullptr);
}

extern "C" int mmnas_chain_join(void* main_stream, void* waiting_stream) {
  SideCtx* sc = side_ctx((hipStream_t)main_stream, false);
  if (!sc || !sc->used) return MMNAS_OK;
  hipEvent_t e = sc->ev[MMNAS_CHAIN_MAX_OPS];
  if (hipEventRecord(e, sc->side) != hipSuccess || hipStreamWaitEvent((hipStream_t)waiting_stream, e, 0) != hipSuccess) {
    set_error("chain_join: event record / wait failed");
    return MMNAS_E_LAUNCH;
  }
  return MMNAS_OK;
}

// ------------------------------------------------------------------------------------------ answer head
// AttFlat(x) + AttFlat(y) -> LayerNorm -> answer projection (hygr_vqa.py:113-119 / full_vqa.py:105-114 with
// modules.py:59-85) as one call per direction: ~28 launches issued back to back instead of ~75 behind 40 autograd
// nodes (the head's kernels take 5-15 us each, so the per-node host cost -- not the GPU -- set its duration).
namespace mmnas {

struct HeadSideLayout { float *h, *logit, *probs, *pooled, *dpooled, *dlog, *dh, *dxpool, *g1part; };
static inline int head_rows(const mmnas_head* hd, const mmnas_attflat_side& sd) { return sd.off ? sd.M : hd->B * sd.S; }
struct HeadLayout {
  HeadSideLayout s[2];
  float *xo, *sum, *xy, *dxy, *dsum, *lnws, *g1proj, *dlogT;
  size_t total;
};

static HeadLayout head_layout(const mmnas_head* hd) {
  HeadLayout L;
  Carver c(hd->arena);
  const size_t B = hd->B;
  for (int k = 0; k < 2; ++k) {
    const mmnas_attflat_side& sd = k ? hd->sy : hd->sx;
    const size_t M = sd.off ? (size_t)sd.M : B * sd.S;
    HeadSideLayout& s = L.s[k];
    s.h = c.take(M * hd->MID); s.logit = c.take(M * hd->G); s.probs = c.take(M * hd->G); s.pooled = c.take(B * hd->G * hd->d);
    s.dpooled = c.take(B * hd->G * hd->d); s.dlog = c.take(M * hd->G); s.dh = c.take(M * hd->MID); s.dxpool = c.take(M * hd->d);
    // one glimpse: partial column sums of the glimpse-logit backward (head.hip), reduced by the next pair launch
    s.g1part = (hd->G == 1 && glimpse1_supported(hd->MID)) ? c.take((size_t)glimpse1_bwd_blocks((long)M, hd->MID) * 3 * hd->MID) : nullptr;
  }
  L.xo = c.take(B * hd->OUT); L.sum = c.take(B * hd->OUT); L.xy = c.take(B * hd->OUT);
  L.dxy = c.take(B * hd->OUT); L.dsum = c.take(B * hd->OUT);
  L.lnws = c.take(mmnas_layernorm_bwd_ws_floats(hd->B, hd->OUT));
  // one answer unit (the ITM matching score): the projection through the one-unit kernels of head.hip
  L.g1proj = (hd->ANS == 1 && glimpse1_supported(hd->OUT)) ? c.take((size_t)glimpse1_bwd_blocks((long)B, hd->OUT) * 3 * hd->OUT) : nullptr;
  // an answer layer whose width is no multiple of 4 (3129): its loss gradient [B, ANS] has unaligned rows, which put both
  // gradient products of the projection on the guarded-load path (26.7 + 14.8 us); transposed once to [ANS, B] they are a
  // TN product (dxy = dlogits Wp, reduction over the answers) and an NN product (dWp += dlogits^T xy) with aligned rows
  L.dlogT = (hd->ANS % 4 != 0 && hd->B % 4 == 0 && hd->ANS > 1) ? c.take((size_t)hd->ANS * B) : nullptr;
  L.total = c.off;
  return L;
}

static int head_check(const mmnas_head* hd, const char* who) {
  MMNAS_REQUIRE(hd, MMNAS_E_ARG, "%s: null descriptor", who);
  MMNAS_REQUIRE(hd->B > 0 && hd->d > 0 && hd->MID > 0 && hd->G > 0 && hd->OUT > 0 && hd->ANS > 0 && hd->sx.S > 0 && hd->sy.S > 0,
                MMNAS_E_SHAPE, "%s: B=%d d=%d MID=%d G=%d OUT=%d ANS=%d Sx=%d Sy=%d", who, hd->B, hd->d, hd->MID, hd->G, hd->OUT,
                hd->ANS, hd->sx.S, hd->sy.S);
  MMNAS_REQUIRE(hd->d % 4 == 0 && hd->MID % 4 == 0 && hd->OUT % 4 == 0, MMNAS_E_SHAPE, "%s: d, MID, OUT must be multiples of 4", who);
  for (int k = 0; k < 2; ++k) {
    const mmnas_attflat_side& sd = k ? hd->sy : hd->sx;
    if (sd.off) MMNAS_REQUIRE(sd.M > 0 && sd.M <= hd->B * sd.S, MMNAS_E_ARG, "%s: packed side %d: M=%d of B*S=%d rows", who, k, sd.M, hd->B * sd.S);
  }
  return MMNAS_OK;
}

}  // namespace mmnas

extern "C" int mmnas_head_plan(const mmnas_head* hd, size_t* arena_bytes) {
  int rc = head_check(hd, "head_plan");
  if (rc) return rc;
  MMNAS_REQUIRE(arena_bytes, MMNAS_E_ARG, "head_plan: null output");
  mmnas_head tmp = *hd;
  tmp.arena = nullptr;
  *arena_bytes = head_layout(&tmp).total;
  return MMNAS_OK;
}

extern "C" int mmnas_head_fwd(const mmnas_head* hd, void* stream) {
  int rc = head_check(hd, "head_fwd");
  if (rc) return rc;
  MMNAS_REQUIRE(hd->arena && hd->logits && hd->ln_a && hd->ln_b && hd->Wp, MMNAS_E_ARG, "head_fwd: null pointer");
  HeadLayout L = head_layout(hd);
  const bool drop = drops(hd);
  const int B = hd->B, d = hd->d, MID = hd->MID, G = hd->G, OUT = hd->OUT;
  mmnas_gemm_desc g;
  hipStream_t st = (hipStream_t)stream;
  // The two AttFlat branches are independent chains of four small launches each.  MMNAS_HEAD_OVERLAP=1 runs the
  // language side's on the second stream beside the image side's, joined where the image side's merge adds its result.
  // MEASURED: slower (supernet step 5.61 -> 5.70 ms, two alternations): each cross-stream event wait costs more than the
  // ~10 us launch it hides.  Off by default -- the third form of stream overlap tried on this path, none of which paid.
  // Default: one stream, and the two sides' glimpse-logit products share a launch (two groups of one grouped GEMM).
  SideCtx* oc = head_overlap_on() ? side_ctx(st, true) : nullptr;
  if (oc && (rc = ev_fork(st, oc->enc, oc->ovl[0]))) return rc;
  const mmnas_attflat_side* sides[2] = {&hd->sx, &hd->sy};
  for (int k = 0; k < 2; ++k)
    MMNAS_REQUIRE(sides[k]->x && sides[k]->W1 && sides[k]->W2 && sides[k]->Wm, MMNAS_E_ARG, "head_fwd: side %d null pointer", k);
  auto side_stream = [&](int k) -> void* { return (oc && k == 0) ? (void*)oc->enc : stream; };
  // h = drop(relu(x W1^T + b1))                                   (FC, modules.py:13-31; own dropout seed per side)
  if (!oc) {   // both sides as the two groups of one launch (own weights, own dropout stream per group)
    gemm_init(g, MMNAS_GEMM_NT, MID, d, d, d, MID);
    g.ngroups = 2; g.relu = 1;
    if (drop) { g.drop_p = hd->drop_p; g.drop_seed = sides[0]->seed; g.drop_site = 0; }
    for (int k = 0; k < 2; ++k) {
      const mmnas_attflat_side& sd = *sides[k];
      g.g[k].M = head_rows(hd, sd); g.g[k].A[0] = sd.x; g.g[k].B[0] = sd.W1; g.g[k].bias = sd.b1; g.g[k].C = L.s[k].h;
      if (drop) g.g[k].drop_seed = sd.seed;
    }
    if ((rc = mmnas_gemm(&g, stream))) return rc;
  }
  for (int k = 0; k < 2 && oc; ++k) {
    const mmnas_attflat_side& sd = *sides[k];
    gemm_init(g, MMNAS_GEMM_NT, MID, d, d, d, MID);
    g.g[0].M = head_rows(hd, sd); g.g[0].A[0] = sd.x; g.g[0].B[0] = sd.W1; g.g[0].bias = sd.b1; g.g[0].C = L.s[k].h; g.relu = 1;
    if (drop) { g.drop_p = hd->drop_p; g.drop_seed = sd.seed; g.drop_site = 0; }
    if ((rc = mmnas_gemm(&g, side_stream(k)))) return rc;
  }
  // glimpse logits = h W2^T + b2                                   (MLP.linear, modules.py:34-41)
  const bool g1 = G == 1 && !oc && glimpse1_supported(MID) && head_glimpse1_on();
  if (g1) {   // one glimpse: a matrix-vector product per side, both in one launch (head.hip)
    if ((rc = glimpse1_fwd(L.s[0].h, hd->sx.W2, hd->sx.b2, L.s[0].logit, (long)head_rows(hd, hd->sx), L.s[1].h, hd->sy.W2, hd->sy.b2,
                           L.s[1].logit, (long)head_rows(hd, hd->sy), MID, st)))
      return rc;
  }
  gemm_init(g, MMNAS_GEMM_NT, G, MID, MID, MID, G);
  for (int k = 0; k < 2 && !g1; ++k) {
    const mmnas_attflat_side& sd = *sides[k];
    mmnas_gemm_group& gg = g.g[oc ? 0 : k];
    gg.M = head_rows(hd, sd); gg.A[0] = L.s[k].h; gg.B[0] = sd.W2; gg.bias = sd.b2; gg.C = L.s[k].logit;
    if (oc && (rc = mmnas_gemm(&g, side_stream(k)))) return rc;
  }
  if (!oc && !g1) { g.ngroups = 2; if ((rc = mmnas_gemm(&g, stream))) return rc; }
  for (int k = 0; k < 2; ++k) {
    const mmnas_attflat_side& sd = *sides[k];
    const HeadSideLayout& s = L.s[k];
    void* const ks = side_stream(k);
    // masked softmax over the sequence + weighted sum                (modules.py:78-84)
    if ((rc = sd.off ? attflat_pool_fwd_packed(s.logit, sd.x, s.probs, s.pooled, B, sd.S, d, G, sd.off, (hipStream_t)ks)
                     : mmnas_attflat_pool_fwd(s.logit, sd.x, sd.mask, s.probs, s.pooled, B, sd.S, d, G, ks))) return rc;
    // merge; the image side adds the language side's result (x_out + y_out, hygr_vqa.py:116)
    gemm_init(g, MMNAS_GEMM_NT, OUT, G * d, G * d, G * d, OUT);
    g.g[0].M = B; g.g[0].A[0] = s.pooled; g.g[0].B[0] = sd.Wm; g.g[0].bias = sd.bm; g.g[0].C = k ? L.sum : L.xo;
    if (k) { g.g[0].residual = L.xo; g.ldres = OUT; }
    if (k && oc && (rc = ev_fork(oc->enc, st, oc->ovl[1]))) return rc;   // the language side's result exists from here on
    if ((rc = mmnas_gemm(&g, ks))) return rc;
  }
  if ((rc = mmnas_layernorm_fwd(L.sum, hd->ln_a, hd->ln_b, L.xy, B, OUT, hd->eps, stream))) return rc;
  if (L.g1proj && head_glimpse1_on())
    return glimpse1_fwd(L.xy, hd->Wp, hd->bp, hd->logits, B, nullptr, nullptr, nullptr, nullptr, 0, OUT, st);
  gemm_init(g, MMNAS_GEMM_NT, hd->ANS, OUT, OUT, OUT, hd->ANS);
  g.g[0].M = B; g.g[0].A[0] = L.xy; g.g[0].B[0] = hd->Wp; g.g[0].bias = hd->bp; g.g[0].C = hd->logits;
  return mmnas_gemm(&g, stream);
}

extern "C" int mmnas_head_bwd(const mmnas_head* hd, void* stream) {
  int rc = head_check(hd, "head_bwd");
  if (rc) return rc;
  MMNAS_REQUIRE(hd->arena && hd->dlogits && hd->ln_a && hd->dln_a && hd->dln_b && hd->Wp && hd->dWp, MMNAS_E_ARG, "head_bwd: null pointer");
  HeadLayout L = head_layout(hd);
  const bool drop = drops(hd);
  const float gate_scale = drop ? 1.0f / (1.0f - hd->drop_p) : 1.0f;
  const int B = hd->B, d = hd->d, MID = hd->MID, G = hd->G, OUT = hd->OUT, ANS = hd->ANS;
  hipStream_t st = (hipStream_t)stream;
  mmnas_gemm_desc g, w;
  // answer projection
  if (L.g1proj && head_glimpse1_on()) {
    AuxReduce pr;
    if ((rc = glimpse1_bwd(hd->dlogits, L.xy, hd->Wp, 1.0f, 0, L.dxy, nullptr, hd->dWp, L.g1proj, B, OUT, st, &pr))) return rc;
    if ((rc = launch_aux_reduce(pr, st))) return rc;
  } else if (L.dlogT && head_projT_on()) {
    if ((rc = transpose2d(hd->dlogits, L.dlogT, B, ANS, st))) return rc;
    gemm_init(g, MMNAS_GEMM_TN, OUT, ANS, B, OUT, OUT);            // dxy [B, OUT] = dlogT^T [B, ANS] Wp [ANS, OUT]
    g.g[0].M = B; g.g[0].A[0] = L.dlogT; g.g[0].B[0] = hd->Wp; g.g[0].C = L.dxy;
    if ((rc = mmnas_gemm(&g, stream))) return rc;
    gemm_init(w, MMNAS_GEMM_NN, OUT, B, B, OUT, OUT);              // dWp [ANS, OUT] += dlogT [ANS, B] xy [B, OUT]
    w.g[0].M = ANS; w.g[0].A[0] = L.dlogT; w.g[0].B[0] = L.xy; w.g[0].C = hd->dWp; w.accumulate = 1;
    if ((rc = mmnas_gemm(&w, stream))) return rc;
  } else {
    gemm_init(w, MMNAS_GEMM_TN, OUT, B, ANS, OUT, OUT);
    w.g[0].M = ANS; w.g[0].A[0] = hd->dlogits; w.g[0].B[0] = L.xy; w.g[0].C = hd->dWp; w.accumulate = 1;
    gemm_init(g, MMNAS_GEMM_NN, OUT, ANS, ANS, OUT, OUT);
    g.g[0].M = B; g.g[0].A[0] = hd->dlogits; g.g[0].B[0] = hd->Wp; g.g[0].C = L.dxy;
    if ((rc = mmnas_gemm_pair(&g, &w, stream))) return rc;
  }
  if (hd->dbp && (rc = mmnas_colsum(hd->dlogits, hd->dbp, B, ANS, ANS, stream))) return rc;
  // proj_norm
  AuxReduce lnred;
  lnred.part = nullptr;
  if ((rc = layernorm_bwd_deferred(L.sum, hd->ln_a, L.dxy, L.dsum, hd->dln_a, hd->dln_b, nullptr, nullptr, L.lnws, 0.f, 0, 0, B, OUT,
                                   hd->eps, st, &lnred)))
    return rc;
  SideCtx* oc = head_overlap_on() ? side_ctx(st, true) : nullptr;
  if (oc && (rc = ev_fork(st, oc->enc, oc->ovl[2]))) return rc;   // the sum's gradient is complete: both sides start
  for (int k = 1; k >= 0; --k) {
    const mmnas_attflat_side& sd = k ? hd->sy : hd->sx;
    const HeadSideLayout& s = L.s[k];
    MMNAS_REQUIRE(sd.x && sd.dx && sd.dW1 && sd.dW2 && sd.dWm, MMNAS_E_ARG, "head_bwd: side %d null pointer", k);
    hipStream_t st = (oc && k == 0) ? oc->enc : (hipStream_t)stream;   // (shadows: the language side on the second stream)
    void* const stream = (void*)st;
    const int M = head_rows(hd, sd);
    // merge: the sum's gradient reaches both sides unchanged
    gemm_init(w, MMNAS_GEMM_TN, G * d, B, OUT, G * d, G * d);
    w.g[0].M = OUT; w.g[0].A[0] = L.dsum; w.g[0].B[0] = s.pooled; w.g[0].C = sd.dWm; w.accumulate = 1;
    gemm_init(g, MMNAS_GEMM_NN, G * d, OUT, OUT, G * d, G * d);
    g.g[0].M = B; g.g[0].A[0] = L.dsum; g.g[0].B[0] = sd.Wm; g.g[0].C = s.dpooled;
    if ((rc = gemm_pair_aux(&g, &w, k ? &lnred : nullptr, st))) return rc;
    if (sd.dbm && (rc = mmnas_colsum(L.dsum, sd.dbm, B, OUT, OUT, stream))) return rc;
    // pooling
    if ((rc = sd.off ? attflat_pool_bwd_packed(s.probs, sd.x, s.dpooled, s.dlog, s.dxpool, B, sd.S, d, G, sd.off, st)
                     : mmnas_attflat_pool_bwd(s.probs, sd.x, sd.mask, s.dpooled, s.dlog, s.dxpool, B, sd.S, d, G, stream))) return rc;
    // glimpse-logit linear: dh = dlog W2 with relu' and the dropout replay from h; db1 rides as column sums of dh
    AuxReduce g1red;
    g1red.part = nullptr;
    if (G == 1 && glimpse1_supported(MID) && head_glimpse1_on()) {   // one glimpse: an outer product + three reductions, one pass over h
      if ((rc = glimpse1_bwd(s.dlog, s.h, sd.W2, gate_scale, 1, s.dh, sd.db1, sd.dW2, s.g1part, M, MID, st, &g1red))) return rc;
      if (sd.db2 && (rc = mmnas_colsum(s.dlog, sd.db2, M, G, G, stream))) return rc;
    } else {
    gemm_init(w, MMNAS_GEMM_TN, MID, M, G, MID, MID);
    w.g[0].M = G; w.g[0].A[0] = s.dlog; w.g[0].B[0] = s.h; w.g[0].C = sd.dW2; w.accumulate = 1;
    gemm_init(g, MMNAS_GEMM_NN, MID, G, G, MID, MID);
    g.g[0].M = M; g.g[0].A[0] = s.dlog; g.g[0].B[0] = sd.W2; g.g[0].C = s.dh;
    g.g[0].gate = s.h; g.ldgate = MID; g.gate_scale = gate_scale;
    g.g[0].colsum = sd.db1;
    if ((rc = mmnas_gemm_pair(&g, &w, stream))) return rc;
    if (sd.db2 && (rc = mmnas_colsum(s.dlog, sd.db2, M, G, G, stream))) return rc;
    }
    // FC: dx = dh W1 + the pooling path's share
    gemm_init(w, MMNAS_GEMM_TN, d, M, MID, d, d);
    w.g[0].M = MID; w.g[0].A[0] = s.dh; w.g[0].B[0] = sd.x; w.g[0].C = sd.dW1; w.accumulate = 1;
    gemm_init(g, MMNAS_GEMM_NN, d, MID, MID, d, d);
    g.g[0].M = M; g.g[0].A[0] = s.dh; g.g[0].B[0] = sd.W1; g.g[0].C = sd.dx;
    g.g[0].residual = s.dxpool; g.ldres = d;
    if ((rc = gemm_pair_aux(&g, &w, g1red.part ? &g1red : nullptr, st))) return rc;
  }
  if (oc && (rc = ev_fork(oc->enc, st, oc->ovl[3]))) return rc;
  return MMNAS_OK;
}
