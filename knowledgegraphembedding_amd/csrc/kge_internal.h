// kge_internal.h — argument blocks shared by the host dispatcher and the kernels.
#pragma once
#include <cstdlib>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <utility>

#include "../../include/kge_hip.h"
#include "kge_device.h"

namespace kge {

enum RowOp : int { ROW_TRAIN = 0, ROW_GIVEN = 1 };

// Query shipping (kge_ship_step): this rank holds only the entity rows
// [own_lo, own_hi) of the table; the row kernels see the GLOBAL batch and
// the shipped q vectors, and touch only owned rows (the table pointer is the
// shard's base minus own_lo rows, so rows keep their global ids).
struct ShipArgs {
  int64_t own_lo, own_hi;
  int world, me;
  const float* q_in;      // [B, Le] q of every row (summed over the shards)
  const float* qp_in;     // [B, Le] head-batch: the positive's tail-form q (h∘r)
  float* qp_out;          // k_ship_q, head-batch
  float* part_out;        // [B, 4] this shard's (max T·s, Z, NL, MG) per row
  const float* parts_in;  // [world, B, 4] every shard's
  float* s_out;           // [B, n] raw scores of the owned negatives
  float* pq;              // [B, Le] head-batch: dL/d(h∘r) of the positive
  float* pstats;          // [B, 4] positive statistics (owner of t; zero elsewhere)
};

struct ScoreArgs {
  const float* ent;
  const float* rel;
  const float* modulus;
  const int64_t* pos;
  const int64_t* neg;
  int64_t neg_stride;  // neg index of (i, j) = neg[i * neg_stride + j]
  int64_t B, n, E, R;
  int Le, Lr;
  RowGeom eg;
  Consts c;
  int64_t jpw;  // candidates per wave work-unit
  float* out;
  int32_t* err;
};

struct RowArgs {
  const float* ent;
  const float* rel;
  const float* modulus;
  const int64_t* pos;
  const int64_t* neg;
  int64_t neg_stride;
  int64_t B, n, E, R;
  int Le, Lr;
  RowGeom eg;
  Consts c;
  int op;           // RowOp
  int adversarial;  // args.negative_adversarial_sampling
  float adv_T;      // args.adversarial_temperature
  int uni_weight;   // args.uni_weight
  float uni_inv;    // 1 / global batch (uni_weight)
  const float* sub_w;
  const float* w_sum;
  float* wsum_out;    // non-null: k_build_q's block 0 writes Σ sub_w here (= w_sum)
  const float* g_in;  // ROW_GIVEN: dL/dscore [B, n]
  float* g_out;       // ROW_TRAIN: dL/ds_ij [B, n]
  float* q_out;       // [B, Le]
  float* dq_out;      // [B, Le]  dL/dq of the negatives (k_row → k_row_epi)
  float* ent_contrib; // [2B, Le]  slot 0 = head row, slot 1 = tail row
  float* rel_contrib; // [B, Lr]
  float* row_stats;   // [B, 4]  logσ(s_pos), neg term, d/dmodulus, s_pos
  int n_lds;          // floats reserved for raw scores in LDS (TRAIN: n)
  int fuse_epi;       // 1: k_row runs the epilogue in its tail, no k_row_epi launch
  int32_t* err;
  void (*timer_mid)(hipStream_t);  // stage-timer hook between the row-pass launches (or null)
  ShipArgs sh;        // query shipping stages only
  float* q_sl;        // non-null (VEC = 4): q also slice-major for k_entity_sl, [slice][row][re 64 | im 64 slots]
  int q_sl_w;         //   slots per slice
};

// k_row's LDS merge buffer: [2][Le] floats, and at least the 256 floats the
// fused Σw reduction (block_weight_sum) uses as its tree
__host__ __device__ inline int vb_floats(int Le) { return 2 * Le > 256 ? 2 * Le : 256; }

// Rows wider than the register-tiled kernels hold (kge_wide.inc, check_model's
// ns = 0): the entity pass cuts each row into WIDE_PARTS column parts (its
// reg_partial slots per entity), and k_row_w keeps one float per negative in LDS
constexpr int WIDE_PARTS = 8;
inline size_t wide_row_lds(int64_t n) { return sizeof(float) * (size_t)(n > 0 ? n : 1); }

struct RelArgs {
  const float* rel;
  int64_t R, E, B, Bn;
  int Lr;
  const int32_t* off;
  const int32_t* occ;
  const float* rel_contrib;  // [B, Lr]
  float reg3;
  float* reg_partial;        // [R]
  float* grad_rel;
  int write_grad;            // store grad_rel (always, unless the optimizer is fused and asks not to)
  AdamT adam;                // fused optimizer step (adam.p == null: none)
  AdamK adamk;
};

// Loss finalisation (k_finalize, or the entity launch's last block: EntArgs.fin)
struct FinArgs {
  const float* row_stats;    // [B, 4]
  const float* sub_w;        // nullable
  const float* w_sum;        // nullable → Σ of sub_w
  int64_t B;
  int uni_weight;
  float uni_n;               // global batch size (uni_weight means)
  const float* reg_partial;  // or null; summed over [reg_a0, reg_a1) then [reg_b0, reg_b1)
  int64_t reg_a0, reg_a1, reg_b0, reg_b1;  // (entity parts, relation rows; a sub-range for an owner's step)
  float regularization;
  float* losses;             // [4]
  float* grad_modulus;       // nullable
  const int32_t* err;        // device error flag, copied to losses[4]
  AdamT adam;                // fused optimizer step of the pRotatE modulus (adam.p == null: none)
  AdamK adamk;
};

struct EntArgs {
  const float* ent;
  const float* modulus;
  int64_t E;
  int64_t e_begin, e_end;  // entity rows this launch covers (a chunk of [0, E))
  int Le;
  RowGeom eg;
  Consts c;
  const int32_t* off;   // CSR offsets (entity buckets first)
  const int32_t* occ;   // occurrence ids, ascending inside each bucket
  int64_t Bn;           // ids < Bn: negative (i, j) = (id / n, id % n)
  int64_t n;
  const float* g;       // [B, n]
  const float* q;       // [B, Le]
  const float* ent_contrib;  // ids >= Bn index [2B, Le]
  float reg3;           // 3 * regularization (0 = off)
  float* reg_partial;   // [E] Σ|x|^3 per row (when reg3 != 0)
  float* grad_ent;
  int write_grad;       // store grad_ent (unless the fused optimizer asks not to)
  int64_t B;            // batch rows (the q buffer's height)
  int nsl;              // > 0: column-sliced pass k_entity_sl with nsl slices of slice_w slots (VEC = 4)
  int slice_w;
  int align_sl;         // k_entity_sl: line-aligned 64-slot slices per row (entity_slice_align)
  const float* q_sl;    // k_entity_sl<.., QSL>: q slice-major (written by k_row; even slices only) or null
  AdamT adam;           // fused optimizer step (adam.p == null: none)
  AdamK adamk;
  RelArgs rel;          // rel_blocks > 0: trailing blocks of k_entity_sl run the relation pass
  int64_t rel_blocks;
  FinArgs fin;          // fin_fused: the launch's last block runs the loss finalisation
  int fin_fused;        // (only when nothing it reads is written by this launch)
  // the LAZY instantiations only (kge_train_step_lazy): row place p of the
  // launch works on entity rows[p], p < *nrows — the batch's touched rows,
  // ascending, compacted on the device (launch_touched_rows); e_begin / e_end
  // are not read
  const int32_t* rows;
  const int32_t* nrows;
};

// k_entity_sl's leading blocks: the fused finalisation and the relation rows,
// rounded up to a multiple of 8 (the XCD count) when there are any
__host__ __device__ inline unsigned ent_lead_blocks(const EntArgs& a) {
  const unsigned l = (unsigned)a.rel_blocks + (a.fin_fused ? 1u : 0u);
  return (l + 7u) & ~7u;
}

// Near-tie window of the fast ranking passes (all three): a candidate whose
// fast fp32 score lies within delta[q] of the query's fast true score is not
// counted but listed for the reference-order refinement (kge_rank_ref.h).
// a diagnostic switch read per launch: true when the variable is set to "0"
inline bool env_flag_off(const char* name) {
  const char* e = getenv(name);
  return e && e[0] == '0' && e[1] == 0;
}
// a launch's kernel by its direction: head-batch's instantiation or tail-batch's
template <typename K>
inline K pick_dir(int mode, K head, K tail) {
  return mode == HEAD_BATCH ? head : tail;
}

struct RankWin {
  const float* delta;  // [nq]
  int32_t* ucnt;       // [nq]  listed candidates (may exceed cap: overflow)
  int32_t* ulist;      // [nq, cap]
  int cap;
};

__device__ __forceinline__ void win_count(const RankWin& w, int64_t q, int64_t e, float s, float st, float dlt,
                                          int& g) {
  const float diff = s - st;
  if (diff > dlt) {
    ++g;
  } else if (diff >= -dlt) {
    const int idx = atomicAdd(&w.ucnt[q], 1);
    if (idx < w.cap) w.ulist[q * (int64_t)w.cap + idx] = (int32_t)e;
  }
}

struct RankArgs {
  const float* ent;
  const float* rel;
  const float* modulus;
  const int64_t* queries;
  int64_t nq, E, R;
  int Le, Lr;
  RowGeom eg;
  Consts c;
  const int64_t* filt_off;
  const int64_t* filt_ids;
  int64_t cpw;          // candidates per wave work-unit
  float* q;             // [nq, Le]
  float* s_true;        // [nq]
  int64_t* true_id;     // [nq]
  int32_t* gt;          // [nq]
  const uint32_t* fbits;  // [nq, W] excluded candidates (filtered ids + the true id)
  int64_t W;
  RankWin win;
  int32_t* err;
  int prep_only;        // launch k_rank_prep only (the MFMA / tile paths count on their own)
  int zero_counts;      // k_rank_prep zeroes gt and the five counters after it (eq, gtx, eqx, ucnt, done)
  int both_dirs;        // (prep_only) both directions in one launch: queries [nq, 3] shared, per-query
                        // arrays of 2·nq (head-batch's first); not for wide rows
  int64_t cstride;      // distance between those counter arrays (the workspace's query count: nq, or 2·nq
                        // when both directions share one workspace and gt points into it)
  const float* trig;    // RotatE: [R, 2, Lr] reference cos | sin of the phases, or null
};

// Reference-order refinement (k_rank_window / k_rank_refine / k_rank_exact).
struct RefArgs {
  const float* ent;
  const float* rel;
  const float* modulus;
  const int64_t* queries;
  int64_t nq, E, R;
  int Le, Lr, K;           // K = reduction length (complex: Le / 2)
  Consts c;
  const float* q;          // [nq, Le] fast-path q (k_rank_prep)
  float* qref;             // [nq, Le] reference-order q
  const int64_t* true_id;  // [nq]
  const float* s_true;     // [nq] fast-path true score
  float* sref_true;        // [nq] reference-order true score
  float* s_true_w;         // [nq] k_rank_true_ref writes s_true here (the split-bf16 path's true score)
  int true_exact;          // s_true is the reference-order score (k_rank_true_ref): δ covers the candidate only
  float* delta;            // [nq] window
  const float* stats;      // [2] max row L2 norm, max |x| of the entity table
  int exact_fast;          // the fast pass is already in reference order (TransE on the register tile)
  const int32_t* ucnt;
  const int32_t* ulist;
  int cap;
  const uint32_t* fbits;
  int64_t W;
  int32_t* gt;             // += refined strictly-greater
  int32_t* eq;             // += refined ties
  int32_t* gtx;            // overflowed queries: exact counts over every candidate
  int32_t* eqx;
  int32_t* err;
  const float* trig;       // RotatE: [R, 2, Lr] reference cos | sin of the phases, or null
  float fast_u;            // > 0: the fast pass's error bound in u·‖q‖·max‖e‖ (split-bf16 tile)
  int ref_slots;           // k_rank_refine: half-waves with an LDS row slot (set by its launcher)
  int ref_global;          // k_rank_refine: q and rows read from global memory (rows too wide for LDS)
  // pRotatE with the caller's sin (kge_rank_sin_args / kge_rank_finish_sin):
  // query q's items [item_off[q], item_off[q+1]) — item 0 the true entity, then
  // the listed candidates (or, for an overflowed window, entity ids 0..E-1) —
  // each K phase sums (args) or their sin as the caller's library evaluates it
  const int64_t* item_off; // [nq + 1] or null
  const float* sins;       // [item_off[nq], K] or null (refine / exact read it)
  float* args;             // [item_off[nq], K] (k_rank_sin_args writes it)
  int lib_sin;             // window: the reference sin is a library's (≤ 1 ulp), not correctly rounded
  int screen;              // k_rank_refine (pRotatE list stage): each listed candidate's score interval
                           // under any library sin within 1 ulp (ref_score_half_prot_bounds); those
                           // whose interval clears the true one's are decided on the device, only the
                           // others stay in the list for the library sin
  int decide;              // (screen) 0: decide nothing, keep every listed candidate (diagnostic)
  int32_t* ucnt_w;         // (screen) the list, rewritten in place
  int32_t* ulist_w;
  float* sref_hi;          // [nq] (screen) the true score interval's upper end (sref_true: its lower)
  int32_t* done;           // [nq] finish stage: the query's items were delivered (a second delivery is an error)
  const int64_t* ltag;     // sin_args / finish: the list tag the list stage wrote, expected = ltag_v
  int64_t ltag_v[3];
};

// Register-tiled filtered ranking (kge_kernels.inc, k_rank_tile): 64 queries ×
// 64 candidates per workgroup, the dim-2 reduction done as one sequential sum
// per (query, candidate) pair.  The gather pass (B columns = the queries' true
// rows) writes s_true with the same instruction sequence the scan pass uses.
struct TileArgs {
  const float* q;          // [nq, Le]  from k_rank_prep ([re | im] for complex rows)
  const float* ent;        // [E, Le]
  const float* modulus;    // pRotatE
  int64_t nq, E;
  int Le, K;               // K = reduction length (complex: Le / 2)
  Consts c;
  const int64_t* true_id;  // [nq]
  float* s_true;           // [nq]  gather pass writes, scan pass reads
  const uint32_t* fbits;   // [nq, W] filtered-candidate bitmap
  int64_t W;
  int32_t* gt;             // [nq]
  RankWin win;
  const float* qph;        // pRotatE: [nq, K, 2] (sin, cos) of q's phase sums (launch_prot_phase)
  const float* eph;        // pRotatE: [E, K, 2] (cos, sin) of the candidate phases
};

// Top-k link prediction (kge_topk).  The candidate table is cut into `parts`
// ranges of `span` candidates (a multiple of 64); every (query, part) keeps a
// list of its k best unexcluded candidates sorted by (score descending, id
// ascending) and writes it to pscore / pid [nq, parts, k] (unused places:
// score −∞, id INT32_MAX); k_topk_merge reduces a query's lists.
// k_topk_prep / k_topk_scan (stage 0 / 1); k_topk_prep_rows (stage 2,
// kge_topk_shard): q from the caller's fixed_rows, no table read:
struct TopkArgs {
  const float* ent;
  const float* rel;
  const float* modulus;
  const int64_t* queries;
  int64_t nq, E, R;
  int Le, Lr;
  RowGeom eg;
  Consts c;
  float* q;               // [nq, Le]
  int64_t* qsan;          // [nq, 3] the queries with the predicted column set to 0 (the filter table's lookup)
  int64_t* state;         // [nq] TOPK_VALID, or TOPK_BAD for a query with an id out of range
  const uint32_t* fbits;  // [nq, W] excluded candidates
  int64_t W;
  int k, parts;
  int64_t span;
  float* pscore;
  int32_t* pid;
  int32_t* err;
  int stage;
  const float* fixed_rows;  // [nq, Le] stage 2: the fixed side's rows (E, R: the global counts)
};
// (both negative: the bitmap launches read state as "true id", and set no bit for it)
constexpr int64_t TOPK_VALID = -1, TOPK_BAD = -2;
constexpr int32_t TOPK_NO_ID = 0x7fffffff;

// k_topk_tile: t.true_id = the queries' state; t.s_true, t.gt, t.win unused
struct TopkTileArgs {
  TileArgs t;
  int k, parts;
  int64_t span;
  float* pscore;
  int32_t* pid;
};

// LDS geometry of the staged row walk (kge_row_walk.inc), floats; the three
// entries below share it.  A row slot is the row rounded to 4 floats;
__host__ __device__ inline int refine_lp(int Le) { return (Le + 3) & ~3; }
// a chunk's score array is 1 + cpc scores and 2 counters, rounded to 4;
__host__ __device__ inline int walk_scrp(int cpc) { return (cpc + 1 + 2 + 3) & ~3; }
// its exclusion bitmap is cpc bits, 32-bit words rounded to 4.
__host__ __device__ inline int walk_bmw(int cpc) { return (((cpc + 31) >> 5) + 3) & ~3; }
// Half-waves with an LDS row slot, at most 8: the slots share 64 KB with the
// entry's fixed_floats; 0: not even one fits, rows are read in place.
inline int walk_slots(int Le, int fixed_floats) {
  const int k = (65536 / 4 - fixed_floats) / refine_lp(Le);
  return k > 8 ? 8 : (k < 1 ? 0 : k);
}

// Ranking against per-query candidate lists (kge_rank_candidates; k_rank_cand,
// k_rank_cand_q).  Work unit = (query, chunk of cpc candidates), chunk-minor on
// grid.x; gt / eq are the workspace's per-query counters, zeroed by the call.
struct CandArgs {
  const float* ent;
  const float* rel;
  const float* modulus;
  const float* trig;       // RotatE: [R, 2, Lr] reference cos | sin of the phases, or null
  const int64_t* queries;  // [nq, 3]
  const int64_t* cand;     // [nq, C]; negative: padding
  int64_t nq, C, E, R;
  int Le, Lr, K;           // K = reduction length (complex: Le / 2)
  Consts c;
  int64_t chunks;          // chunks per query
  int cpc;                 // candidates per chunk (the last one may hold fewer)
  int vec4;                // rows staged in 16-byte slots (the header's alignment rule)
  int nslot;               // half-waves with an LDS row slot (cand_slots)
  int in_place;            // rows too wide for LDS: q from qref, rows read in place
  float* qref;             // [nq, Le] reference-order q (in_place only; k_rank_cand_q writes it)
  int32_t* gt;             // [nq] += strictly greater
  int32_t* eq;             // [nq] += equal
  int32_t* err;
};
constexpr int CAND_CPC_MAX = 1024;  // candidates per chunk: the chunk's scores sit in LDS
// fixed: q and the largest score array
inline int cand_slots(int Le) { return walk_slots(Le, refine_lp(Le) + walk_scrp(CAND_CPC_MAX)); }

// Relation prediction (kge_rank_relations; k_rank_rel).  Work unit = (query,
// chunk of cpc consecutive relations), chunk-minor on grid.x; gt / eq are the
// workspace's per-query counters, zeroed by the call.
struct RelRankArgs {
  const float* ent;
  const float* rel;
  const float* modulus;
  const float* trig;        // RotatE: [R, 2, Lr] cos | sin of the phases (the caller's, or the workspace's)
  const int64_t* queries;   // [nq, 3]; r = -1: no true relation (scores only)
  const int64_t* filt_off;  // [nq + 1] or null: no filter
  const int64_t* filt_ids;  // relation ids excluded per query
  int64_t nq, E, R;
  int Le, Lr, K;            // K = reduction length (complex: Le / 2)
  Consts c;
  int64_t chunks;           // chunks per query
  int cpc;                  // relations per chunk (the last one may hold fewer)
  int vec4;                 // rows staged in 16-byte slots
  int nslot;                // half-waves with an LDS row slot (rel_slots)
  int in_place;             // rows too wide for LDS: h, t and the relation rows read in place
  float* scores;            // [nq, R] or null
  int32_t* gt;              // [nq] += strictly greater
  int32_t* eq;              // [nq] += equal
  int32_t* err;
};
constexpr int REL_CPC_MAX = 1024;  // relations per chunk: the chunk's scores sit in LDS
// fixed: the h and t rows, the largest score array and filter bitmap
inline int rel_slots(int Le) {
  return walk_slots(Le, 2 * refine_lp(Le) + walk_scrp(REL_CPC_MAX) + walk_bmw(REL_CPC_MAX));
}

// Sharded filtered ranking (kge_rank_shard; k_rshard_rows, k_rshard_true,
// k_rshard_count).  `ent` points own_lo rows before the shard: only rows
// [own_lo, own_hi) are read.  COUNT's work unit = (chunk of cpc consecutive owned
// rows, query), query-minor on grid.x; counts are the caller's, zeroed by the call.
struct ShardArgs {
  const float* ent;
  const float* rel;
  const float* modulus;
  const float* trig;         // RotatE: [R, 2, Lr] reference cos | sin of the phases, or null
  const int64_t* queries;    // [nq, 3]
  const int64_t* filt_off;   // per-query lists [nq + 1], or (ftab) the whole index's [E·R + 1] starts
  const int64_t* filt_ids;
  int ftab;                  // KGE_RANK_FILTER_TABLE
  int64_t nq, E, R;
  int64_t own_lo, own_hi;    // the owned rows (global ids)
  int Le, Lr, K;             // K = reduction length (complex: Le / 2)
  Consts c;
  int64_t chunks;            // chunks of the owned range
  int cpc;                   // rows per chunk (the last one may hold fewer)
  int vec4;                  // rows staged in 16-byte slots (the header's alignment rule)
  int nslot;                 // half-waves with an LDS row slot (shard_slots)
  int in_place;              // rows too wide for LDS: q from qref, rows read in place
  int qw;                    // queries per workgroup asked for (KGE_RANK_SHARD_QPW; the launch decides, and sets nslot)
  float* fixed_rows;        // [nq, Le] the fixed side's rows (ROWS writes, TRUE / COUNT read the reduced ones)
  float* s_true;             // [nq] (TRUE writes, COUNT reads the reduced ones)
  float* qref;               // [nq, Le] reference-order q (in_place only; k_rshard_q writes it)
  int64_t* counts;           // [2, nq] += strictly greater | equal
  int32_t* err;
};
constexpr int SHARD_CPC_MAX = 1024;  // rows per chunk: the chunk's scores and its exclusion bitmap sit in LDS
// fixed: the q, largest score array and bitmap of each of the workgroup's qw queries
inline int shard_slots(int Le, int qw = 1) {
  return walk_slots(Le, qw * (refine_lp(Le) + walk_scrp(SHARD_CPC_MAX) + walk_bmw(SHARD_CPC_MAX)));
}

// Sharded ranking against candidate lists (kge_rank_candidates_shard;
// k_rshard_cand, k_rshard_cand_q).  `ent` points own_lo rows before the shard:
// only rows [own_lo, own_hi) are read.  Work unit = (query, chunk of cpc list
// places), chunk-minor on grid.x; the workgroup scores the chunk's OWNED
// candidates only.  counts are the caller's, zeroed by the call.
struct CandShardArgs {
  const float* ent;
  const float* rel;
  const float* modulus;
  const float* trig;         // RotatE: [R, 2, Lr] reference cos | sin of the phases, or null
  const int64_t* queries;    // [nq, 3]
  const int64_t* cand;       // [nq, C]; negative: padding
  int64_t nq, C, E, R;
  int64_t own_lo, own_hi;    // the owned rows (global ids)
  int Le, Lr, K;             // K = reduction length (complex: Le / 2)
  Consts c;
  int64_t chunks;            // chunks per query
  int cpc;                   // list places per chunk (the last one may hold fewer)
  int vec4;                  // rows staged in 16-byte slots (the header's alignment rule)
  int nslot;                 // half-waves with an LDS row slot (cand_shard_slots)
  int in_place;              // rows too wide for LDS: q from qref, rows read in place
  const float* fixed_rows;   // [nq, Le] the reduced fixed-side rows (KGE_RSHARD_ROWS)
  const float* s_true;       // [nq] the reduced reference-order true scores (KGE_RSHARD_TRUE)
  float* qref;               // [nq, Le] reference-order q (in_place only; k_rshard_cand_q writes it)
  int64_t* counts;           // [2, nq] += strictly greater | equal
  int32_t* err;
};
constexpr int CAND_SHARD_CPC_MAX = 1024;  // list places per chunk: the chunk's scores and owned ids sit in LDS
// a chunk's compacted owned ids (int32) rounded to 4, and the 4 waves' counts of one compaction round
__host__ __device__ inline int walk_idw(int cpc) { return ((cpc + 3) & ~3) + 4; }
// fixed: q, the largest score array and the largest id list
inline int cand_shard_slots(int Le) {
  return walk_slots(Le, refine_lp(Le) + walk_scrp(CAND_SHARD_CPC_MAX) + walk_idw(CAND_SHARD_CPC_MAX));
}

// kge_rank_shard_fast: the fast counting pass on a shard-local view (k_rsf_prep,
// k_rsf_window, the counting tiles, k_rsf_finish).  r is the refinement's
// argument block over the VIEW: r.ent = the shard's first row, r.E = its row
// count, every id local (global − own_lo).  r.true_id holds each query's state:
// −1 a query with an id out of range, [0, r.E) the true row's local id, r.E the
// true row is another rank's.  r.s_true is the workspace's copy of the caller's
// reduced reference-order scores (NaN for a bad query), r.true_exact = 1.
struct ShardFastArgs {
  RefArgs r;
  RowGeom eg;               // k_rsf_prep's slots (by fixed_rows' and the relation table's alignment)
  const float* fixed_rows;  // [nq, Le] the reduced fixed-side rows
  const float* s_true_in;   // [nq] the reduced reference-order true scores
  int64_t own_lo, E_glob;   // the shard's first row and the table's row count (global)
  float* q_w;               // [nq, Le] = r.q        (k_rsf_prep writes)
  float* s_true_w;          // [nq]     = r.s_true
  int64_t* state_w;         // [nq]     = r.true_id
  int32_t* gt_w;            // [nq]     = r.gt       (zeroed by k_rsf_prep)
  int32_t* ucnt_w;          // [nq]     = r.ucnt     (k_rsf_window: cap + 1 for an infinite s_true, a rescan)
  uint32_t* bits_w;         // [nq, W]  = r.fbits    (k_rsf_window adds the owned true row's bit)
  int64_t* counts;          // [2, nq] strictly greater | equal (k_rsf_finish writes every place)
  int32_t* listed;          // [nq] or null
  int nslot;                // k_rsf_finish: half-waves with an LDS row slot (rsf_slots)
  int in_place;             // k_rsf_finish: q and one slot do not fit LDS, rows are read where they lie
};
// k_rsf_finish's dynamic LDS, floats: [q: Lp][slots: nslot × Lp][2 counters, rounded to 4]
inline int rsf_slots(int Le) { return walk_slots(Le, refine_lp(Le) + 4); }

// What one ModelOps::row call launches (Launch::row, kge_kernels.inc / kge_wide.inc).
enum class RowStage : int {
  Pass = 0,       // q build + gather loop (k_row), with the epilogue in its tail when RowArgs.fuse_epi
  Epilogue = 1,   // the separate epilogue (k_row_epi); nothing when fuse_epi
  QOnly = 2,      // q build alone (the factor-exchange step rebuilds q for the global batch)
  // query shipping (kge_ship_step; not for wide rows)
  ShipQ = 3,      // q (and the positive's q, head-batch)
  ShipRows = 4,   // the owned negatives' row pass
  ShipMerge = 5,  // merge of the ranks' partial statistics
  ShipChain = 6,  // chain rule
};

// What one ModelOps::rank_ref call launches (launch_rank_ref): the ranking's
// reference-order refinement.
enum class RefStage : int {
  Window = 0,     // k_rank_window: each query's near-tie window δ and its reference-order q
  Refine = 1,     // k_rank_refine: the listed candidates rescored in the reference's order
  Exact = 2,      // k_rank_exact: queries whose window overflowed the list, over every candidate
  SinArgs = 3,    // k_rank_sin_args: pRotatE phase sums of every item, for the caller's sin
  TrueRef = 4,    // k_rank_true_ref: the true score in the reference's order (RefArgs.true_exact)
  Interval = 5,   // k_rank_exact_iv: pRotatE's list stage, overflowed windows by score intervals
};

struct ModelOps {
  int (*score)(int mode, int vec, int ns, const ScoreArgs&, int64_t units, hipStream_t);
  int (*row)(int mode, int vec, int ns, RowStage, const RowArgs&, size_t lds, hipStream_t);
  int (*entity)(int mode, int vec, int ns, const EntArgs&, int opt, hipStream_t);  // opt: OptKind
  int (*rank)(int mode, int vec, int ns, const RankArgs&, hipStream_t);
  int (*rank_tile)(int mode, int gather, const TileArgs&, hipStream_t);
  int (*rank_ref)(int mode, RefStage, const RefArgs&, hipStream_t);
  int (*topk)(int mode, int vec, int ns, const TopkArgs&, hipStream_t);
  int (*topk_tile)(int mode, const TopkTileArgs&, hipStream_t);
  int (*rank_cand)(int mode, const CandArgs&, hipStream_t);
  int (*rank_rel)(const RelRankArgs&, hipStream_t);
  int (*rank_shard)(int mode, int stage, const ShardArgs&, hipStream_t);  // stage: KGE_RSHARD_*
  // kge_rank_shard_fast, stage 0: k_rsf_prep (vec / ns: fixed_rows' slots), 1: k_rsf_window, 2: k_rsf_finish
  int (*rank_shard_fast)(int mode, int vec, int ns, int stage, const ShardFastArgs&, hipStream_t);
  int (*rank_cand_shard)(int mode, const CandShardArgs&, hipStream_t);
};

ModelOps model_ops_transe();
ModelOps model_ops_distmult();
ModelOps model_ops_complex();
ModelOps model_ops_rotate();
ModelOps model_ops_protate();

}  // namespace kge
