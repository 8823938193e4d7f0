// Runtime switches of the native library: every MMNAS_* environment variable the C side reads is one row of
// MMNAS_SWITCHES below (docs/SWITCHES.md is the inventory; the README table is printed from it by tools/switch_table.py).
//
//   kind      int       unset or empty: the default; otherwise atoi
//             bool      as int, then != 0
//             exact1    on only when the value starts with '1'          (the opt-in idiom: "2" is off)
//             presence  on when the variable exists at all              ("0" is on)
//             string    read with getenv where it is used; the row documents it (value: 1 when set and not empty)
//   policy    once        read at the first use, then cached
//             every_call  read at every use
//             reload      read by gemm.hip's load_tuning(): at the first product and at mmnas_gemm_reload_tuning()
//
// Switch::set installs an override (the mmnas_set_* calls) that every later get() returns, whatever the policy.
#pragma once

namespace mmnas {

int env_int(const char* name, int dflt);   // unset or empty: dflt; otherwise atoi

enum SwKind { sw_int, sw_bool, sw_exact1, sw_presence, sw_string };
enum SwPolicy { sw_once, sw_every_call, sw_reload };

struct Switch {
  const char* name;
  int dflt;
  SwKind kind;
  SwPolicy policy;
  const char* help;   // "[kind, policy] one line"
  int value;          // valid when state != 0
  int state;          // 0: nothing cached; 1 / 2: cached from the default / the environment; 3: set by call

  int get() { return state ? value : read(); }   // a cached switch: one load and one compare
  int read();                                    // parses the environment; caches unless the policy is every_call
  int reload();                                  // parses the environment and caches (drops an override)
  int set(int v);                                // override; returns the previous effective value
  int peek(int* source) const;                   // the effective value without caching anything; *source as mmnas_switch_info
};

//  X(identifier, variable, default, kind, policy, help)
#define MMNAS_SWITCHES(X) \
  /* ops.hip: backbone chains, answer head */ \
  X(chain_overlap, "MMNAS_CHAIN_OVERLAP", 0, bool, once, "language stream beside the leading image-stream operators (mmnas_set_chain_overlap); measured: no gain, DESIGN.md section 5") \
  X(head_overlap, "MMNAS_HEAD_OVERLAP", 0, bool, once, "the answer head's two AttFlat sides on two streams") \
  X(head_glimpse1, "MMNAS_HEAD_GLIMPSE1", 1, bool, every_call, "0: the head's one-glimpse logit layer as GEMM launches (A/B, tests); ops.py reads it too") \
  X(head_projt, "MMNAS_HEAD_PROJT", 1, bool, every_call, "0: the answer projection's gradients from the untransposed loss gradient") \
  X(rel_hoist, "MMNAS_REL_HOIST", 1, bool, once, "relation bias of all lazy-handle operators of a stream in one launch per direction (mmnas_set_rel_hoist); 0: one fused launch per operator (supernet step 4.54 -> 5.00 ms)") \
  X(rel_overlap, "MMNAS_REL_OVERLAP", 0, bool, once, "the image stream's relation launches on a second stream (mmnas_set_rel_overlap); measured slower, +2.5 % on the supernet step") \
  X(node_lnb, "MMNAS_NODE_LNB", 1, bool, once, "architecture step: the sampled candidate's LayerNorm backward inside the node's mix kernel (7.81 -> 7.72 ms, profiles/r06_node_lnb_ab.txt); 0: its own launch") \
  X(guided_hoist, "MMNAS_GUIDED_HOIST", 1, bool, once, "key / value projections of a chain's guided operators as grouped launches (mmnas_set_guided_hoist)") \
  X(rel_fwd_valu, "MMNAS_REL_FWD_VALU", 0, exact1, every_call, "1: a lone RelSelfAtt computes its bias with the per-operator fused kernel instead of the one-operator multi kernel (A/B)") \
  X(side_prio, "MMNAS_SIDE_PRIO", 1, bool, every_call, "0: the chains' extra streams without stream priorities (read when a stream pair is created)") \
  X(side_flush, "MMNAS_SIDE_FLUSH", 0, string, once, "op: side-stream parameter-gradient work released behind every operator instead of once per phase") \
  X(wgrad_live, "MMNAS_WGRAD_LIVE", 1, int, once, "image-stream weight gradients of a padded batch's chain reduce over the 32-row K-tiles that cover the live gradient rows only (mmnas_set_wgrad_live); 0: all B Sy rows") \
  /* small.hip: short-sequence operators */ \
  X(small_ops, "MMNAS_SMALL_OPS", 1, bool, once, "SelfAtt of <= 16 rows as one launch forward (mmnas_set_small_ops); 0: the general path") \
  X(small_bwd, "MMNAS_SMALL_BWD", 1, bool, once, "the same operators' backward as two launches (mmnas_set_small_bwd)") \
  X(small_ffn, "MMNAS_SMALL_FFN", 0, int, once, "FeedForward forward as one launch (mmnas_set_small_ffn): 1 four slices of 256 hidden units, 2 eight of 128; measured neutral (profiles/r05_small_ffn_ab.txt)") \
  /* gemmln.hip: product + LayerNorm row-panel kernel */ \
  X(gemm_ln, "MMNAS_GEMM_LN", 0, exact1, once, "1: the merge / last FFN product and its LayerNorm as one row-panel launch (mmnas_set_gemm_ln); measured neutral, profiles/r06_ab.txt") \
  X(gemm_ln_minm, "MMNAS_GEMM_LN_MINM", 2048, int, once, "fewest rows for the row-panel kernel (read together with MMNAS_GEMM_LN)") \
  X(gemm_ln_maxk, "MMNAS_GEMM_LN_MAXK", 256, int, once, "largest K for the row-panel kernel (read together with MMNAS_GEMM_LN)") \
  /* attention.hip, attention_bwd16.hip */ \
  X(mha_nw, "MMNAS_MHA_NW", 4, int, every_call, "2: attention cores never use 4-wave workgroups (4-wave groups measured 7-15 % faster; the streaming forward always runs four)") \
  X(mha_stream_mink, "MMNAS_MHA_STREAM_MINK", 257, int, every_call, "fewest keys at which the attention forward streams the keys in blocks of 128 (1..257; more than 256 keys always stream; dense rows only)") \
  X(mha_pair, "MMNAS_MHA_PAIR", 1, bool, once, "0: two attention cores of one geometry as two launches (mixed chain)") \
  X(mha_bwd_fused, "MMNAS_MHA_BWD_FUSED", 1, bool, once, "0: the attention backward as separate dQ and dK / dV kernels (dense rows only)") \
  X(mha_fwd_b16, "MMNAS_MHA_FWD_B16", 1, bool, once, "0: attention forward (d_h = 64, 65..128 keys) on the fp32 MFMA kernels instead of split-bf16 operands (profiles/r06_attention_b16_ab.txt)") \
  X(mha_fwd_b16_two, "MMNAS_MHA_FWD_B16_TWO", 320, int, once, "more than this many (sample, head) pairs: the split-bf16 forward runs two per workgroup") \
  X(mha_bwd_b16, "MMNAS_MHA_BWD_B16", 1, bool, once, "0: attention backward (d_h = 64, 65..128 keys) on the fp32 MFMA kernels instead of split-bf16 operands (supernet step -1.6 % with both)") \
  /* relmulti.hip, relfused.hip */ \
  X(rel_multi_dbg, "MMNAS_REL_MULTI_DBG", 0, int, once, "timing experiments of a -DMMNAS_DBG_REL=1 build only (wrong results): 1 no stores, 2 no raw reloads, 4 no head-projection MFMAs") \
  X(rel_multi_wgs, "MMNAS_REL_MULTI_WGS", 3, int, once, "workgroups per CU of the multi-operator relation forward (tuning)") \
  X(rel_multi_yield, "MMNAS_REL_MULTI_YIELD", 0, int, once, "1 | 3: the multi-operator relation kernels' yield variants (tuning)") \
  X(rel_keylimit, "MMNAS_REL_KEYLIMIT", 1, int, once, "multi-operator relation kernels of a padded batch walk only the elements under keys up to each sample's last unmasked one (mmnas_set_rel_keylimit); 0: all B S^2 elements") \
  X(rel_bwd_valu, "MMNAS_REL_BWD_VALU", 1, bool, once, "0: the fused relation backward as the all-MFMA kernel (A/B)") \
  /* gemm.hip: tuning, read by load_tuning() */ \
  X(gemm_tile, "MMNAS_GEMM_TILE", 0, int, reload, "64 | 128: force the tile shape") \
  X(gemm_generic, "MMNAS_GEMM_GENERIC", 0, presence, reload, "set (to anything): force the guarded-load path; ops.py reads it too") \
  X(gemm_sk, "MMNAS_GEMM_SK", 1, int, reload, "stream-K / split-K: 0 never, 1 automatic, 2 always") \
  X(gemm_wgs, "MMNAS_GEMM_WGS", 0, int, reload, "co-resident workgroup budget (0: 1024 for 64^2 tiles, 512 for 128^2)") \
  X(gemm_min_units, "MMNAS_GEMM_MIN_UNITS", 4, int, reload, "fewest K-tiles a workgroup is given (at least 1)") \
  X(gemm_gm, "MMNAS_GEMM_GM", 0, int, reload, "row-panels per tile-order block (0: 8)") \
  X(gemm_xcd, "MMNAS_GEMM_XCD", 1, int, reload, "0: identity workgroup mapping") \
  X(gemm_split, "MMNAS_GEMM_SPLIT", 6, int, reload, "products as 6 / 3 / 1 bf16 MFMA products of split operands (6: fp32-grade; 3, 1: reduced precision), 0: fp32 MFMA") \
  X(gemm_pair, "MMNAS_GEMM_PAIR", 1, int, reload, "0: mmnas_gemm_pair launches its two products separately") \
  X(gemm_split_slots, "MMNAS_GEMM_SPLIT_SLOTS", 0, int, reload, "split-K pieces wanted over all tiles (0: from SPLIT_P and SPLIT_MINWG)") \
  X(gemm_split_p, "MMNAS_GEMM_SPLIT_P", 24, int, reload, "K-tiles per split-K piece (at least 1)") \
  X(gemm_split_minwg, "MMNAS_GEMM_SPLIT_MINWG", 256, int, reload, "fewest split-K pieces in total when pieces of SPLIT_P would be fewer") \
  X(gemm_pf, "MMNAS_GEMM_PF", 2, int, reload, "1 | 2: K-tiles of operand loads in flight ahead of the MFMA block (64^2 fp32 path)") \
  X(gemm_hyb_t, "MMNAS_GEMM_HYB_T", 16, int, reload, "fewest K-tiles per output tile for the whole-tiles + streamed-tail hybrid") \
  X(gemm_lean, "MMNAS_GEMM_LEAN", 3, int, reload, "lean kernels: bit 0 NT / NN products, bit 1 split-K TN products") \
  X(gemm_lean_maxb, "MMNAS_GEMM_LEAN_MAXB", 8 << 20, int, reload, "largest B matrix (bytes) the lean tile order is used for") \
  X(lstm_fwd_p, "MMNAS_LSTM_FWD_P", 0, int, every_call, "K-tiles per workgroup of the LSTM forward step's stream-K product (0: whole tiles; read per time step)") \
  X(lstm_bwd_p, "MMNAS_LSTM_BWD_P", 8, int, every_call, "K-tiles per workgroup of the LSTM backward step's stream-K product (0: whole tiles; read per time step)") \
  /* util.hip */ \
  X(prof_dump, "MMNAS_PROF_DUMP", 0, string, every_call, "file: mmnas_prof_collect appends one kind,tag,ms,flops,bytes row per bracketed launch (tools/prof_shapes.py)")

namespace sw {
#define MMNAS_SW_DECLARE(id, var, dflt, kind, policy, help) extern Switch id;
MMNAS_SWITCHES(MMNAS_SW_DECLARE)
#undef MMNAS_SW_DECLARE
}  // namespace sw

}  // namespace mmnas
