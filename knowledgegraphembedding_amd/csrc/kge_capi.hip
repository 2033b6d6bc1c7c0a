// kge_capi.hip — the extern "C" boundary declared in include/kge_hip.h.
// Host-side argument checks, workspace carving and launch sequencing; no
// allocation, no synchronisation (graph-capturable).
//
// Layout: shared helpers, then training (StepCall → StepPlan → the rows /
// entity / finalize phases), then ranking (RankCall → RankRun → table, queries,
// tail), then the one extern "C" block whose entries fill a call struct by name.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "kge_common.h"

namespace kge {
namespace {

struct Geom {
  int vec, ns;
  RowGeom eg;
  bool cplx;
};

const ModelOps& ops_for(int model) {
  static const ModelOps tbl[5] = {model_ops_transe(), model_ops_distmult(), model_ops_complex(),
                                  model_ops_rotate(), model_ops_protate()};
  return tbl[model];
}

int hip_status(hipError_t e) { return e == hipSuccess ? KGE_OK : (KGE_ERR_HIP_BASE + (int)e); }
int launch_status(int e) { return e == 0 ? KGE_OK : (e < 0 ? KGE_ERR_DIM : KGE_ERR_HIP_BASE + e); }

bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

// model.py:63-70 plus the broadcast rules of the plug-ins.
int check_model(const kge_model_desc* m, Geom* g) {
  if (!m) return KGE_ERR_ARG;
  // a caller built against another layout of this struct (KGE_ABI_VERSION)
  if (m->struct_size != (int32_t)sizeof(kge_model_desc)) return KGE_ERR_ABI;
  if (m->model < KGE_TRANSE || m->model > KGE_PROTATE) return KGE_ERR_MODEL;
  if (!m->entity_embedding || !m->relation_embedding) return KGE_ERR_ARG;
  if (m->nentity <= 0 || m->nrelation <= 0 || m->entity_dim <= 0 || m->relation_dim <= 0) return KGE_ERR_ARG;
  if (m->nentity >= (int64_t)1 << 31 || m->nrelation >= (int64_t)1 << 30) return KGE_ERR_DIM;
  const int Le = m->entity_dim, Lr = m->relation_dim;
  g->cplx = (m->model == KGE_COMPLEX || m->model == KGE_ROTATE);
  int span;
  if (m->model == KGE_ROTATE) {
    if (Le != 2 * Lr) return KGE_ERR_SHAPE;  // RotatE: -de, not -dr
    span = Lr;
  } else if (m->model == KGE_COMPLEX) {
    if (Le != Lr || (Le & 1)) return KGE_ERR_SHAPE;  // ComplEx: -de and -dr
    span = Le / 2;
  } else {
    if (Le != Lr) return KGE_ERR_SHAPE;
    span = Le;
  }
  if (m->model == KGE_PROTATE && !m->modulus) return KGE_ERR_ARG;
  const bool v4 = (span % 4 == 0) && aligned16(m->entity_embedding) && aligned16(m->relation_embedding);
  g->vec = v4 ? 4 : 1;
  const int S = span / g->vec;
  int ns = 1;
  while (64 * ns < S) ns *= 2;
  if (ns > (g->vec == 4 ? 8 : 32)) {
    // (half-)rows over 2048 floats: the run-time-looped kernels of
    // kge_wide.inc (single-float elements, ns = 0)
    g->vec = 1;
    g->ns = 0;
    g->eg.S = span;
    g->eg.half = g->cplx ? span : 0;
    return KGE_OK;
  }
  g->ns = ns;
  g->eg.S = S;
  g->eg.half = g->cplx ? span : 0;
  return KGE_OK;
}

int kernel_mode(int32_t mode) { return (mode == KGE_HEAD_BATCH) ? HEAD_BATCH : TAIL_BATCH; }

// The candidates of a scoring call.  'single' scores (h, r, t) with the
// tail-batch formulas, t in place of one negative per row: the ids alias the
// positives' third column.
struct Negatives {
  const int64_t* ids;
  int64_t stride;  // id of (i, j) = ids[i * stride + j]
};
int negatives_of(int32_t mode, const int64_t* pos, const int64_t* neg, int64_t nneg, Negatives* out) {
  if (mode == KGE_SINGLE) {
    if (nneg != 1) return KGE_ERR_ARG;
    *out = {pos + 2, 3};
  } else {
    if (!neg) return KGE_ERR_ARG;
    *out = {neg, nneg};
  }
  return KGE_OK;
}

// With float4 slots (vec = 4) the entity and relation passes store the
// gradient rows and stream the fused Adam's param / exp_avg / exp_avg_sq 16
// bytes at a time, so those buffers must be 16-byte aligned like the tables
// (a NULL pointer passes: whether it may be NULL is the entry's own check;
// pRotatE's modulus is one float, updated by scalar accesses).
bool grad_streams_aligned(const Geom& geo, const float* grad_entity, const float* grad_relation,
                          const kge_adam_desc* adam) {
  if (geo.vec != 4) return true;
  if (!aligned16(grad_entity) || !aligned16(grad_relation)) return false;
  if (adam)
    for (const kge_adam_tensor* t : {&adam->entity, &adam->relation})
      if (!aligned16(t->param) || !aligned16(t->exp_avg) || !aligned16(t->exp_avg_sq)) return false;
  return true;
}

Consts consts_of(const kge_model_desc* m) {
  Consts c;
  c.gamma = m->gamma;
  c.kappa = m->phase_divisor;
  c.kappa_p = m->phase_divisor_p;
  c.modulus = 0.f;
  return c;
}

struct Carver {
  char* base;
  size_t off = 0;
  explicit Carver(void* p) : base((char*)p) {}
  template <typename T>
  T* take(size_t count) {
    off = (off + 255) & ~(size_t)255;
    T* p = base ? (T*)(base + off) : nullptr;
    off += count * sizeof(T);
    return p;
  }
};

hipStream_t as_stream(void* s) { return (hipStream_t)s; }

// Diagnostic switches, read per call so a test can flip them between calls;
// none changes a result bit (each selects between paths that are tested
// bitwise equal): KGE_ENT_SLICES (force the entity pass's column-slice count;
// 0 = the row-per-wave k_entity), KGE_FIN_SEPARATE (the loss finalisation as
// its own launch), KGE_CSR_SERIAL (the occurrence CSR before the row pass, not
// beside it), KGE_RANK_SIDE (the ranking's table work on the side stream),
// KGE_RANK_SIN_SCREEN=0 (pRotatE: send every listed near-tie to the caller's
// sin, no device screen).
int env_int(const char* name, int dflt) {
  const char* e = getenv(name);
  return e ? atoi(e) : dflt;
}

// ---- timers (bench instrumentation; see kge_stage_timer in the header)
// Events created on first use and kept; a reset rewinds `used`.
struct EventPool {
  std::vector<hipEvent_t> ev;
  size_t used = 0;  // events recorded so far
  // records the next event on s; false (and none used up) when that fails
  bool record(hipStream_t s) {
    if (used == ev.size()) {
      hipEvent_t e;
      if (hipEventCreate(&e) != hipSuccess) return false;
      ev.push_back(e);
    }
    if (hipEventRecord(ev[used], s) != hipSuccess) return false;
    ++used;
    return true;
  }
};

// the training step's stage timer: TM_COUNT marks per timed call
enum TimerMark { TM_START, TM_Q_BUILT, TM_ROWS_END, TM_EPI_END, TM_CSR_JOINED, TM_ENTITY_END, TM_END, TM_COUNT };
static_assert(TM_COUNT == KGE_TIMER_STAGES + 1, "a stage is the time between two marks");
struct StageTimer {
  bool on = false;
  int period = 1;   // time one train call in `period`
  size_t seen = 0;  // train calls since enabled
  EventPool pool;
  void mark(hipStream_t s) {
    if (on) pool.record(s);
  }
  // kge_stage_timer reads the marks in TM_COUNT's: a timed call that runs only
  // part of the step owes the marks after its last live one
  void pad_after(hipStream_t s, TimerMark last_live) {
    for (int k = last_live + 1; k < TM_COUNT; ++k) mark(s);
  }
};
StageTimer g_timer;
void timer_mark(hipStream_t s) { g_timer.mark(s); }  // RowArgs.timer_mid: TM_Q_BUILT

// the ranking's stage timer (kge_stage_timer commands 4 / 5): marks tagged by
// slot — 0 the call starts (with the call's number of directions), 1 fast pass
// begins, 2 fast pass ends, 3 ranks written.  A call is the marks from one
// slot-0 mark to the next; a stage is the time between the call's first mark of
// its slot and its last mark of the next slot, so a call that writes ranks in
// several pieces (pRotatE's per-chunk finish calls each mark slot 3) is timed to
// its last piece, and the list stage's own calls need no padding.
struct RankTimer {
  bool on = false;
  EventPool pool;
  std::vector<int> slot, ndir;  // per recorded event
  void mark(hipStream_t s, int sl, int nd = 1) {
    if (!on || !pool.record(s)) return;
    if (slot.size() < pool.used) {
      slot.resize(pool.used);
      ndir.resize(pool.used);
    }
    slot[pool.used - 1] = sl;
    ndir[pool.used - 1] = nd;
  }
};
RankTimer g_rank_timer;

// the KGE_TIMER_STAGES stage times of one timed train call (its TM_COUNT
// events at e), added to ms
hipError_t add_stage_ms(const hipEvent_t* e, float* ms) {
  hipError_t err = hipEventSynchronize(e[TM_END]);
  for (int k = 0; k < KGE_TIMER_STAGES && err == hipSuccess; ++k) {
    float t = 0.f;
    err = hipEventElapsedTime(&t, e[k], e[k + 1]);
    ms[k] += t;
  }
  return err;
}

// ---- side stream: the index-only work (occurrence CSR) and the relation
// pass run beside the gather kernels of the caller's stream.  Fork/join via
// events (a pattern stream capture records as graph edges); the caller's
// stream never runs ahead of anything the side stream still reads or writes.
struct Side {
  hipStream_t s = nullptr;
  hipEvent_t fork = nullptr, csr_done = nullptr, epi_done = nullptr, rel_done = nullptr;
  hipEvent_t rk_fork = nullptr, rk_join = nullptr;  // ranking: the entity table's statistics / split beside the queries' stages
};

Side* side_for_device() {
  static Side sides[64];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return nullptr;
  Side& sd = sides[dev];
  if (!sd.s) {
    if (hipStreamCreateWithFlags(&sd.s, hipStreamNonBlocking) != hipSuccess) return nullptr;
    hipEventCreateWithFlags(&sd.fork, hipEventDisableTiming);
    hipEventCreateWithFlags(&sd.csr_done, hipEventDisableTiming);
    hipEventCreateWithFlags(&sd.epi_done, hipEventDisableTiming);
    hipEventCreateWithFlags(&sd.rel_done, hipEventDisableTiming);
    hipEventCreateWithFlags(&sd.rk_fork, hipEventDisableTiming);
    hipEventCreateWithFlags(&sd.rk_join, hipEventDisableTiming);
  }
  return &sd;
}

// One edge of a fork or join.  The status is the caller's to return: under
// stream capture an edge the runtime refuses would otherwise leave a graph
// that races, reported as KGE_OK.
int edge_record(hipEvent_t ev, hipStream_t s) { return hip_status(hipEventRecord(ev, s)); }
int edge_wait(hipStream_t s, hipEvent_t ev) { return hip_status(hipStreamWaitEvent(s, ev, 0)); }

// ================================================================ training

struct GradWs {
  float *g, *q, *dq, *ent_contrib, *rel_contrib, *row_stats, *reg_partial, *wsum;
  int32_t *keys, *cnt, *off, *tmp, *occ;
  float* q_sl;  // slice-major q for the sliced entity pass (single-call steps with even slices)
  void* scan_tmp;
  size_t scan_tmp_bytes;
};

GradWs carve_grad(void* ws, const kge_model_desc* m, int64_t B, int64_t n, size_t* bytes) {
  Carver c(ws);
  GradWs w;
  const int64_t Bn = B * n, N = Bn + 3 * B, nb = m->nentity + m->nrelation;
  w.g = c.take<float>(Bn);
  w.q = c.take<float>(B * (int64_t)m->entity_dim);
  w.dq = c.take<float>(B * (int64_t)m->entity_dim);
  w.ent_contrib = c.take<float>(2 * B * (int64_t)m->entity_dim);
  w.rel_contrib = c.take<float>(B * (int64_t)m->relation_dim);
  w.row_stats = c.take<float>(B * 4);
  w.reg_partial = c.take<float>(8 * m->nentity + m->nrelation);  // per (entity, column slice) + per relation
  w.wsum = c.take<float>(4);
  w.keys = c.take<int32_t>(N);
  w.cnt = c.take<int32_t>(nb + 1);
  w.off = c.take<int32_t>(nb + 1);
  w.tmp = c.take<int32_t>(N);
  w.occ = c.take<int32_t>(N);
  w.q_sl = c.take<float>(8 * B * 512);  // up to 8 slices × B rows × (64 + 64) float4 slots
  w.scan_tmp_bytes = csr_scan_temp_bytes(nb);
  w.scan_tmp = c.take<uint8_t>((int64_t)w.scan_tmp_bytes);
  *bytes = c.off + 256;
  return w;
}

// What the lazy step (kge_train_step_lazy) adds behind carve_grad's
// `grad_bytes`: the touched-row list, at most U = min(E, B·n + 2B) ids, its
// length, and the compaction's scratch.
struct LazyWs {
  int32_t *rows, *nrows;
  void* sel_tmp;
  size_t sel_tmp_bytes;
};
int64_t lazy_places(const kge_model_desc* m, int64_t B, int64_t n) {
  const int64_t occ = B * n + 2 * B;
  return occ < m->nentity ? occ : m->nentity;
}
LazyWs carve_lazy(void* ws, const kge_model_desc* m, int64_t B, int64_t n, size_t grad_bytes, size_t* bytes) {
  Carver c(ws);
  c.off = grad_bytes;
  LazyWs w;
  w.rows = c.take<int32_t>(lazy_places(m, B, n));
  w.nrows = c.take<int32_t>(4);
  w.sel_tmp_bytes = touched_rows_temp_bytes(m->nentity);
  w.sel_tmp = c.take<uint8_t>((int64_t)w.sel_tmp_bytes);
  *bytes = c.off + 256;
  return w;
}

// Data-parallel factor exchange (kge_train_rows_slice / kge_train_step_from_rows)
// XS_CSR_ONLY: the occurrence CSR of a batch alone, on the caller's stream;
// XS_FROM_ROWS_CSR: XS_FROM_ROWS with that CSR already in the workspace
enum XStage : int { XS_NONE = 0, XS_ROWS_ONLY = 1, XS_FROM_ROWS = 2, XS_CSR_ONLY = 3, XS_FROM_ROWS_CSR = 4 };

// One call of the training family as its entry describes it; an entry fills
// the groups it means and leaves the rest at these defaults.
struct StepCall {
  struct {
    const kge_model_desc* m;
    int32_t mode;
    const int64_t *pos, *neg;
    int64_t batch, nneg;
  } in;
  struct {
    void* workspace;
    size_t bytes;
    int32_t* err_flag;
    void* stream;
  } ws;
  struct Loss {
    const float* subsampling_weight = nullptr;
    const float* weight_sum = nullptr;  // the caller's Σw (the exchange stages need it)
    int32_t uni_weight = 1;
    int64_t uni_batch = 0;  // > 0: the global batch the uni_weight means divide by
    int32_t adversarial = 1;
    float adversarial_temperature = 1.f;
    float regularization = 0.f;
  } loss;
  const kge_adam_desc* adam = nullptr;  // the fused optimizer step, or none
  // kge_train_step_adagrad: the caller's descriptor; train_impl checks it where
  // it checks Adam's and then carries it in `adam`'s fields (adagrad_view) with
  // `opt` naming the rule
  const kge_adagrad_desc* adagrad = nullptr;
  int opt = OPT_ADAM;  // OptKind
  struct Out {
    float *entity = nullptr, *relation = nullptr, *modulus = nullptr, *losses = nullptr;
  } out;
  int32_t phases = KGE_PHASE_ALL;
  int64_t e_begin = 0, e_end = -1;  // the entity rows an owner's step covers (-1: to the table's end)
  int xstage = XS_NONE;
  struct Rows {  // the exchange stages' per-row factors, in the caller's (gathered) buffers
    float *g = nullptr, *dq = nullptr, *stats = nullptr;
  } rows;
  int reg_relations = 1;             // 0: the caller counts the relation rows' regulariser elsewhere
  int64_t csr_lo = 0, csr_hi = -1;   // entity buckets the occurrence CSR builds (-1: to the table's end)
  // kge_train_step_lazy: the entity pass and its fused Adam cover the batch's
  // touched rows only; no entity gradient is written (out.entity may be null)
  bool lazy = false;
};

// A call's batch as every launch of it sees it.
struct Batch {
  const kge_model_desc* m;
  Geom geo;
  int kmode;  // HEAD_BATCH / TAIL_BATCH
  const int64_t* pos;
  Negatives neg;
  int64_t B, n;
  GradWs w;  // (with the caller's buffers in place of the carved ones where a stage brings its own)
  int32_t* err;
  hipStream_t s;
  LazyWs lz;  // (lazy step only)
};

// entity pass variant: column slices (k_entity_sl) when the row fits one
// 16-B slot per lane per slice (returns the slice count); 0 selects the
// row-per-wave pass (also forced by KGE_ENT_SLICES=0)
int entity_slices(const Geom& geo, int64_t B, int Le) {
  const int forced = env_int("KGE_ENT_SLICES", -1);  // read per call (tests switch it)
  const int S = geo.eg.S;
  auto fits = [&](int k) { return (S + k - 1) / k <= 64; };
  if (geo.vec != 4 || forced == 0) return 0;
  int k = forced;
  if (k < 0) {
    // smallest power of two that fits; doubled further while the q column
    // slice exceeds 2 MiB (half an XCD L2) only if the waves stay >= 3/4
    // busy (measured: a larger slice beats half-empty waves — global batch
    // of 2048 rows, 4 slices 0.54 ms vs 8 slices 0.73 ms)
    const double qslice = (double)B * Le * sizeof(float);
    k = 1;
    while (k < 8 && !fits(k)) k *= 2;
    while (k < 8 && qslice / k > 2.0 * 1024 * 1024 && (S + 2 * k - 1) / (2 * k) >= 48) k *= 2;
  }
  return ((k == 1 || k == 2 || k == 4 || k == 8) && fits(k)) ? k : 0;
}

// Line-aligned slicing for k_entity_sl (align_sl): the inner slice boundaries
// of a row move by the row's 16-B phase within its 128-B line so they fall on
// line boundaries of the row's first half.  Only when every stream of the pass
// (table = Adam param, gradient, moments) has the same phase, every row's
// phase is one the 64-slot slices absorb (last slice ≤ 64 slots) — d = 1000:
// phases 0 and 4.
int entity_slice_align(int nsl, int S, int Le, const float* ent, const float* grad, const AdamT& ad) {
  if (nsl < 2) return 0;
  const uintptr_t base = (uintptr_t)ent & 127;
  if (base & 15) return 0;
  for (const float* p : {grad, (const float*)ad.p, (const float*)ad.m, (const float*)ad.v})
    if (p && ((uintptr_t)p & 127) != base) return 0;
  if (S <= 64 * (nsl - 1)) return 0;
  int max_sh = 0;
  for (int e = 0; e < 8; ++e) {
    const int sh = (int)(((base + (uintptr_t)e * (uintptr_t)Le * 4u) >> 4) & 7);
    max_sh = sh > max_sh ? sh : max_sh;
  }
  return (S - 64 * (nsl - 1) + max_sh <= 64) ? 1 : 0;
}

// ---- argument blocks: one builder each, shared by run_grad and kge_ship_step

AdamK adam_k(const kge_adam_desc* adam) {
  AdamK k;
  k.b1 = adam ? adam->beta1 : 0.f;
  k.b2 = adam ? adam->beta2 : 0.f;
  k.eps = adam ? adam->eps : 0.f;
  return k;
}

AdamT adam_t(const kge_adam_desc* adam, const kge_adam_tensor* t) {
  AdamT o;
  o.p = (adam && t && t->param) ? t->param : nullptr;
  o.m = o.p ? t->exp_avg : nullptr;
  o.v = o.p ? t->exp_avg_sq : nullptr;
  o.step_size = o.p ? t->step_size : 0.f;
  o.bc2s = o.p ? t->bias_correction2_sqrt : 1.f;
  return o;
}

// Adagrad's descriptor in the fields the argument builders read (OptKind,
// kge_device.h): state_sum where exp_avg stands, lr as step_size.  exp_avg_sq
// repeats state_sum so the shared non-NULL and alignment checks see every
// streamed array; no kernel reads it.
kge_adam_desc adagrad_view(const kge_adagrad_desc& d) {
  kge_adam_desc v;
  memset(&v, 0, sizeof(v));
  auto tensor = [&](const kge_adagrad_tensor& t) {
    return kge_adam_tensor{t.param, t.state_sum, t.state_sum, d.lr, 1.f};
  };
  v.entity = tensor(d.entity);
  v.relation = tensor(d.relation);
  v.modulus = tensor(d.modulus);
  v.eps = d.eps;
  v.write_grad = d.write_grad;
  return v;
}

// the optimizer's part of a gradient pass's arguments
struct Opt {
  AdamT t;         // fused step of this pass's tensor (t.p == null: none)
  AdamK k;
  int write_grad;  // store the gradient (always, unless the optimizer is fused and asks not to)
};
Opt opt_for(const kge_adam_desc* adam, const kge_adam_tensor* t) {
  return {adam_t(adam, t), adam_k(adam), (!adam || adam->write_grad) ? 1 : 0};
}
// the gradient alone, whatever the call's optimizer (the shipped relation pass)
const Opt OPT_GRAD_ONLY = {AdamT{}, AdamK{}, 1};

// k_row's LDS: q (2 padded halves), the merge buffer, the raw scores, the
// wave states and, with the fused epilogue, the positive's element terms;
// wide rows (kge_wide.inc): one float per negative
size_t row_lds(const Geom& geo, int Le, const RowArgs& ra, bool wide) {
  if (wide) return wide_row_lds(ra.n);
  return sizeof(float) * (2 * 64 * (size_t)geo.ns * geo.vec + (size_t)vb_floats(Le) + (size_t)ra.n_lds + 32 +
                          (ra.fuse_epi ? 64 * (size_t)geo.ns * geo.vec : 0));
}
constexpr size_t LDS_MAX = 64 * 1024;

RowArgs row_args(const Batch& b) {
  const kge_model_desc* m = b.m;
  RowArgs ra;
  memset(&ra, 0, sizeof(ra));
  ra.ent = m->entity_embedding; ra.rel = m->relation_embedding; ra.modulus = m->modulus;
  ra.pos = b.pos; ra.neg = b.neg.ids; ra.neg_stride = b.neg.stride;
  ra.B = b.B; ra.n = b.n; ra.E = m->nentity; ra.R = m->nrelation;
  ra.Le = m->entity_dim; ra.Lr = m->relation_dim; ra.eg = b.geo.eg; ra.c = consts_of(m);
  ra.g_out = b.w.g; ra.q_out = b.w.q; ra.dq_out = b.w.dq; ra.ent_contrib = b.w.ent_contrib;
  ra.rel_contrib = b.w.rel_contrib; ra.row_stats = b.w.row_stats; ra.err = b.err;
  ra.fuse_epi = 1;  // measured +1 % over the separate k_row_epi launch
  return ra;
}

// the occurrence CSR of the batch, entity buckets [e_lo, e_hi)
CsrArgs csr_args(const Batch& b, int64_t e_lo, int64_t e_hi) {
  const GradWs& w = b.w;
  CsrArgs ca;
  ca.pos = b.pos; ca.neg = b.neg.ids; ca.neg_stride = b.neg.stride;
  ca.B = b.B; ca.n = b.n; ca.Bn = b.B * b.n; ca.E = b.m->nentity; ca.R = b.m->nrelation;
  ca.keys = w.keys; ca.cnt = w.cnt; ca.off = w.off; ca.tmp = w.tmp; ca.occ = w.occ; ca.err = b.err;
  ca.e_lo = e_lo; ca.e_hi = e_hi;
  ca.scan_tmp = w.scan_tmp; ca.scan_tmp_bytes = w.scan_tmp_bytes;
  return ca;
}

// ent_parts: the entity pass's reg_partial slots, which the relation rows' follow
RelArgs rel_args(const Batch& b, float reg3, int64_t ent_parts, float* grad_relation, const Opt& opt) {
  const kge_model_desc* m = b.m;
  RelArgs rl;
  memset(&rl, 0, sizeof(rl));
  rl.rel = m->relation_embedding; rl.R = m->nrelation; rl.E = m->nentity; rl.B = b.B; rl.Bn = b.B * b.n;
  rl.Lr = m->relation_dim;
  rl.off = b.w.off; rl.occ = b.w.occ; rl.rel_contrib = b.w.rel_contrib; rl.reg3 = reg3;
  rl.reg_partial = b.w.reg_partial + ent_parts; rl.grad_rel = grad_relation;
  rl.write_grad = opt.write_grad;
  rl.adam = opt.t;
  rl.adamk = opt.k;
  return rl;
}

// the entity rows a step covers, as column parts: nsl per row (1 for the
// row-per-wave pass), and whether the relation rows' regulariser counts here
struct EntRange {
  int64_t e_begin, e_end;
  int nsl;
  bool reg_relations;
  int64_t per() const { return nsl > 0 ? nsl : 1; }
};

// (align_sl, q_sl, the fused relation rows and finalisation stay off: run_grad
// alone turns them on)
EntArgs ent_args(const Batch& b, const EntRange& r, const float* g, float reg, float* grad_entity, const Opt& opt) {
  const kge_model_desc* m = b.m;
  EntArgs ea;
  memset(&ea, 0, sizeof(ea));
  ea.ent = m->entity_embedding; ea.modulus = m->modulus; ea.E = m->nentity; ea.Le = m->entity_dim; ea.eg = b.geo.eg;
  ea.e_begin = r.e_begin; ea.e_end = r.e_end;
  ea.c = consts_of(m); ea.off = b.w.off; ea.occ = b.w.occ; ea.Bn = b.B * b.n; ea.n = b.n;
  ea.g = g;
  ea.q = b.w.q; ea.ent_contrib = b.w.ent_contrib; ea.reg3 = 3.f * reg; ea.reg_partial = b.w.reg_partial;
  ea.grad_ent = grad_entity;
  ea.write_grad = opt.write_grad;
  ea.nsl = r.nsl;
  ea.slice_w = r.nsl > 0 ? (b.geo.eg.S + r.nsl - 1) / r.nsl : 0;  // (wide: elements per part)
  ea.adam = opt.t;
  ea.adamk = opt.k;
  ea.B = b.B;
  ea.rel_blocks = 0;
  return ea;
}

// the loss terms of the finalisation (every training form; kge_score_backward has none)
FinArgs fin_loss(const StepCall::Loss& l, int64_t B, float* losses, const int32_t* err) {
  FinArgs fa;
  memset(&fa, 0, sizeof(fa));
  fa.sub_w = l.subsampling_weight;
  fa.w_sum = l.weight_sum;
  fa.B = B;
  fa.uni_weight = l.uni_weight ? 1 : 0;
  fa.uni_n = (float)(l.uni_batch > 0 ? l.uni_batch : B);
  fa.losses = losses;
  fa.err = err;
  return fa;
}

// ... completed by what the step itself decides: the regulariser's partial
// sums over the entity rows [e_begin, e_end) (all of them unless an owner's
// range) and, unless counted elsewhere, the relation rows; pRotatE's modulus
FinArgs fin_args(FinArgs fa, const Batch& b, const EntRange& r, float reg, float* grad_modulus,
                 const kge_adam_desc* adam) {
  const kge_model_desc* m = b.m;
  const int64_t ent_parts = m->nentity * r.per();
  fa.row_stats = b.w.row_stats;
  fa.reg_partial = (reg != 0.f) ? b.w.reg_partial : nullptr;
  fa.reg_a0 = r.e_begin * r.per();
  fa.reg_a1 = r.e_end * r.per();
  fa.reg_b0 = ent_parts;
  fa.reg_b1 = ent_parts + (r.reg_relations ? m->nrelation : 0);
  fa.regularization = reg;
  fa.grad_modulus = (m->model == KGE_PROTATE) ? grad_modulus : nullptr;
  fa.adam = adam_t(adam, (adam && m->model == KGE_PROTATE) ? &adam->modulus : nullptr);
  fa.adamk = adam_k(adam);
  return fa;
}

// ---- run_grad: the shared body of backward and train.  Caller's stream: q
// build → gather loop → epilogue → entity pass → finalise; side stream: CSR ∥
// row pass, relation pass ∥ entity pass.

// Every switch of one call, derived once from the call and its batch.
struct StepPlan {
  bool wide;  // rows over 2048 floats (kge_wide.inc)
  size_t lds;
  bool all;   // the whole step in this call
  bool from_rows, csr_ready;
  // stage timing: a full call records all 7 marks; a phased ROWS call (the
  // data-parallel path) records the row-pass marks and pads the rest, so the
  // row pass is timed live on every rank either way
  bool timed;
  Side* sd;
  hipStream_t ss;  // the side stream (the caller's where there is none)
  // entity rows [e_begin, e_end) in nsl column slices (wide rows: WIDE_PARTS
  // column parts per entity, k_entity_w)
  EntRange ents;
  int64_t ent_parts;
  // relation pass: as trailing blocks of the sliced entity launch (one call,
  // no stream join); else beside the entity pass on the side stream (always
  // so in phased calls, and for wide rows)
  bool rel_fused, rel_side;
  // slice-major q: k_row also writes q as [slice][row][re | im] so each of
  // the entity pass's q reads is 2 KB contiguous and line-aligned (0.240 ->
  // 0.234 ms at the FB15k shape); the single-call step with even slices only
  // (the line-aligned slices shift a row's columns by its phase, so they are
  // off here)
  bool q_slm;
  // KGE_CSR_SERIAL=1 (diagnostic, same bits): the CSR on the caller's stream
  // before the row pass instead of beside it — what k_row gains without the
  // side stream's kernels competing for its CU slots
  bool csr_serial;
  bool use_csr;  // the CSR beside the row pass
  // the loss finalisation rides in the entity launch's last block when that
  // launch is the whole rest of the step and writes nothing the finalisation
  // reads (no regulariser partials, no pRotatE modulus update)
  bool fin_wanted, fin_fused;
  float* grad_modulus;  // (pRotatE only)
  // lazy step: the touched rows are compacted behind the CSR, on its stream,
  // and the entity launch covers `places` row places (the host-known bound
  // min(E, B·n + 2B) of the touched rows) in place of the table's E rows
  bool lazy;
  int64_t places;
  int opt;  // OptKind of the fused step (Adagrad: the lazy step only)
};

int plan_step(const StepCall& c, const Batch& b, const RowArgs& ra, StepPlan* out) {
  const kge_model_desc* m = b.m;
  const Geom& geo = b.geo;
  StepPlan p;
  p.wide = (geo.ns == 0);
  p.lds = row_lds(geo, m->entity_dim, ra, p.wide);
  if (p.lds > LDS_MAX) return KGE_ERR_DIM;
  p.all = (c.phases == KGE_PHASE_ALL);
  p.from_rows = (c.xstage == XS_FROM_ROWS || c.xstage == XS_FROM_ROWS_CSR);
  p.csr_ready = (c.xstage == XS_FROM_ROWS_CSR);
  p.timed = (c.phases & KGE_PHASE_ROWS) && !p.from_rows && c.xstage != XS_CSR_ONLY && g_timer.on && ra.op == ROW_TRAIN &&
            (g_timer.seen++ % (size_t)g_timer.period) == 0;
  p.sd = side_for_device();
  p.ss = p.sd ? p.sd->s : b.s;
  p.ents.e_begin = c.e_begin;
  p.ents.e_end = c.e_end < 0 ? m->nentity : c.e_end;
  p.ents.nsl = p.wide ? WIDE_PARTS : entity_slices(geo, b.B, m->entity_dim);
  // row-wise Adagrad needs a whole row's Σg² in one wave: the row-per-wave pass
  if (c.opt == OPT_ADAGRAD_ROW) p.ents.nsl = 0;
  p.opt = c.opt;
  p.ents.reg_relations = c.reg_relations != 0;
  p.ent_parts = m->nentity * p.ents.per();
  p.rel_fused = p.all && p.ents.nsl > 0 && !p.wide;
  p.rel_side = p.sd && !p.rel_fused;
  p.q_slm = p.all && p.ents.nsl > 0 && geo.vec == 4 && c.xstage == XS_NONE && ra.op == ROW_TRAIN &&
            (geo.eg.S + p.ents.nsl - 1) / p.ents.nsl <= 64;
  p.csr_serial = !p.csr_ready && env_int("KGE_CSR_SERIAL", 0) != 0;
  p.use_csr = !p.csr_ready && !p.csr_serial;
  p.grad_modulus = (m->model == KGE_PROTATE) ? c.out.modulus : nullptr;
  const bool fin_reads_step = c.loss.regularization != 0.f ||
                              adam_t(c.adam, (c.adam && m->model == KGE_PROTATE) ? &c.adam->modulus : nullptr).p;
  p.fin_wanted = (c.phases & KGE_PHASE_FINALIZE) && (c.out.losses || p.grad_modulus);
  p.fin_fused = p.fin_wanted && p.all && p.rel_fused && p.ents.e_end > p.ents.e_begin && !fin_reads_step &&
                env_int("KGE_FIN_SEPARATE", 0) == 0;
  p.lazy = c.lazy;
  p.places = c.lazy ? lazy_places(m, b.B, b.n) : 0;
  *out = p;
  return KGE_OK;
}

// XS_ROWS_ONLY: the negative-row pass alone (q build + k_row), dL/dq to global
// memory for the exchange; no epilogue, CSR or relation pass (kge_train_rows_slice)
int rows_only(const Batch& b, const StepPlan& p, const RowArgs& ra) {
  if (p.timed) g_timer.mark(b.s);
  const int st = launch_status(ops_for(b.m->model).row(b.kmode, b.geo.vec, b.geo.ns, RowStage::Pass, ra, p.lds, b.s));
  if (st) return st;
  if (p.timed) {
    g_timer.mark(b.s);
    g_timer.pad_after(b.s, TM_ROWS_END);
  }
  return KGE_OK;
}

// KGE_PHASE_ROWS: CSR fork, q build and gather loop, epilogue, and the relation
// pass where it runs beside the entity pass
int rows_phase(const Batch& b, const StepPlan& p, const RowArgs& ra, const CsrArgs& ca, const RelArgs& rl) {
  const ModelOps& op = ops_for(b.m->model);
  const Geom& geo = b.geo;
  Side* sd = p.sd;
  hipStream_t s = b.s, ss = p.ss;
  int st;
  auto touched_rows = [&](hipStream_t on) {  // (lazy) behind the CSR, on its stream
    return launch_status(launch_touched_rows(ca.off, ca.E, b.lz.rows, b.lz.nrows, b.lz.sel_tmp, b.lz.sel_tmp_bytes, on));
  };
  if (p.csr_serial) {
    st = launch_status(launch_csr(ca, s));
    if (st) return st;
    if (p.lazy && (st = touched_rows(s))) return st;
  }
  // fork point: the occurrence CSR needs only the batch indices (recorded
  // before anything else is queued, so the side stream never waits for the
  // row pass)
  if (sd && p.use_csr) hipEventRecord(sd->fork, s);

  // q build + gather loop on the caller's stream, launched first so the GPU
  // is on the long kernel while the host queues everything else
  if (p.timed) g_timer.mark(s);
  // (XS_FROM_ROWS: the row pass ran on the ranks; only q is rebuilt here)
  st = launch_status(op.row(b.kmode, geo.vec, geo.ns, p.from_rows ? RowStage::QOnly : RowStage::Pass, ra, p.lds, s));
  if (st) return st;
  if (p.timed) g_timer.mark(s);

  if (p.use_csr) {
    if (sd) hipStreamWaitEvent(ss, sd->fork, 0);
    st = launch_status(launch_csr(ca, ss));
    if (st) return st;
    if (p.lazy && (st = touched_rows(ss))) return st;
    if (sd) hipEventRecord(sd->csr_done, ss);
  }

  // epilogue (positive score, chain rule)
  st = launch_status(op.row(b.kmode, geo.vec, geo.ns, RowStage::Epilogue, ra, p.lds, s));
  if (st) return st;
  if (p.timed) g_timer.mark(s);

  // relation pass on the side stream once the epilogue's contributions exist
  if (p.rel_side) {
    hipEventRecord(sd->epi_done, s);
    hipStreamWaitEvent(ss, sd->epi_done, 0);
    st = launch_status(launch_rel_rows(rl, ss, p.opt));
    if (st) return st;
    hipEventRecord(sd->rel_done, ss);
  } else if (!p.all) {
    st = launch_status(launch_rel_rows(rl, s, p.opt));
    if (st) return st;
  }
  if (p.timed && !p.all) g_timer.pad_after(s, TM_EPI_END);
  return KGE_OK;
}

// KGE_PHASE_ENTITY
int entity_phase(const Batch& b, const StepPlan& p, const EntArgs& ea, const RelArgs& rl) {
  hipStream_t s = b.s;
  int st;
  if (p.sd && p.use_csr) hipStreamWaitEvent(s, p.sd->csr_done, 0);  // join 1: the entity pass reads the CSR
  if (p.timed) g_timer.mark(s);
  if (ea.e_end > ea.e_begin) {
    st = launch_status(ops_for(b.m->model).entity(b.kmode, b.geo.vec, b.geo.ns, ea, p.opt, s));
    if (st) return st;
  } else if (p.rel_fused) {
    // an owner with no entity rows (a trailing rank of a small table) still
    // owes the relation pass the entity launch would have carried
    st = launch_status(launch_rel_rows(rl, s, p.opt));
    if (st) return st;
  }
  if (p.timed) g_timer.mark(s);
  return KGE_OK;
}

// KGE_PHASE_FINALIZE
int finalize_phase(const Batch& b, const StepPlan& p, const RelArgs& rl, const FinArgs& fa) {
  hipStream_t s = b.s;
  int st;
  if (p.rel_side) {
    hipStreamWaitEvent(s, p.sd->rel_done, 0);  // join 2: everything the side stream wrote
  } else if (p.all && !p.rel_fused) {
    st = launch_status(launch_rel_rows(rl, s, p.opt));
    if (st) return st;
  }
  if (p.fin_wanted && !p.fin_fused) {
    st = launch_status(launch_finalize(fa, s, p.opt));
    if (st) return st;
  }
  if (p.timed) g_timer.mark(s);
  return KGE_OK;
}

// ra: the row pass's arguments; fa: the finalisation's loss terms (fin_loss)
int run_grad(const StepCall& c, const Batch& b, RowArgs ra, FinArgs fa) {
  const kge_model_desc* m = b.m;
  StepPlan p;
  int st = plan_step(c, b, ra, &p);
  if (st) return st;
  const float reg = c.loss.regularization;
  ra.timer_mid = p.timed ? &timer_mark : nullptr;
  ra.q_sl = p.q_slm ? b.w.q_sl : nullptr;
  ra.q_sl_w = p.q_slm ? (b.geo.eg.S + p.ents.nsl - 1) / p.ents.nsl : 0;
  // no fused epilogue where there is none (rows only), or where it reads the
  // gathered dL/dq (k_row_epi after the exchange)
  if (c.xstage == XS_ROWS_ONLY || p.from_rows) ra.fuse_epi = 0;
  if (c.xstage == XS_ROWS_ONLY) return rows_only(b, p, ra);
  const CsrArgs ca = csr_args(b, c.csr_lo, c.csr_hi < 0 ? m->nentity : c.csr_hi);
  if (c.xstage == XS_CSR_ONLY) return launch_status(launch_csr(ca, b.s));  // kge_train_csr

  const RelArgs rl =
      rel_args(b, 3.f * reg, p.ent_parts, c.out.relation, opt_for(c.adam, c.adam ? &c.adam->relation : nullptr));
  if (c.phases & KGE_PHASE_ROWS) {
    st = rows_phase(b, p, ra, ca, rl);
    if (st) return st;
  }
  fa = fin_args(fa, b, p.ents, reg, p.grad_modulus, c.adam);
  if (c.phases & KGE_PHASE_ENTITY) {
    Opt opt = opt_for(c.adam, c.adam ? &c.adam->entity : nullptr);
    if (p.lazy) opt.write_grad = 0;  // no dense entity gradient exists (the relation's follows write_grad)
    EntArgs ea = ent_args(b, p.ents, (ra.op == ROW_TRAIN) ? b.w.g : ra.g_in, reg, c.out.entity, opt);
    if (p.lazy) {  // the launch's extent is the row places; the kernels take their rows from rows[]
      ea.e_begin = 0;
      ea.e_end = p.places;
      ea.rows = b.lz.rows;
      ea.nrows = b.lz.nrows;
    }
    ea.align_sl = (p.q_slm || p.wide) ? 0
                                      : entity_slice_align(p.ents.nsl, b.geo.eg.S, m->entity_dim, m->entity_embedding,
                                                           opt.write_grad ? c.out.entity : nullptr, ea.adam);
    ea.q_sl = p.q_slm ? b.w.q_sl : nullptr;
    ea.rel = rl;
    ea.rel_blocks = p.rel_fused ? (m->nrelation + 3) / 4 : 0;
    ea.fin = fa;
    ea.fin_fused = p.fin_fused ? 1 : 0;
    st = entity_phase(b, p, ea, rl);
    if (st) return st;
  }
  if (!(c.phases & KGE_PHASE_FINALIZE)) return KGE_OK;
  return finalize_phase(b, p, rl, fa);
}

// neg: the call's candidates (its negatives, or 'single''s aliased tails); w: its carved workspace
Batch batch_of(const StepCall& c, const Geom& geo, const Negatives& neg, const GradWs& w) {
  return {c.in.m, geo, kernel_mode(c.in.mode), c.in.pos, neg, c.in.batch, c.in.nneg, w, c.ws.err_flag,
          as_stream(c.ws.stream), LazyWs{}};
}

int train_impl(const StepCall& call) {
  StepCall c = call;
  kge_adam_desc view;  // (kge_train_step_adagrad: c.adam once the descriptor has passed)
  const kge_model_desc* m = c.in.m;
  Geom geo;
  int st = check_model(m, &geo);
  if (st) return st;
  if (c.in.mode != KGE_HEAD_BATCH && c.in.mode != KGE_TAIL_BATCH) return KGE_ERR_MODE;
  const bool grads_given = (c.out.entity || c.lazy) && c.out.relation && c.out.losses;
  const bool rows_given = c.rows.g && c.rows.dq && c.rows.stats;
  if (c.xstage == XS_NONE && !grads_given) return KGE_ERR_ARG;
  const bool csr_only = (c.xstage == XS_CSR_ONLY);
  const bool from_rows = (c.xstage == XS_FROM_ROWS || c.xstage == XS_FROM_ROWS_CSR);
  const bool exchange = (c.xstage != XS_NONE && !csr_only);  // a stage of the per-row factor exchange
  if (exchange && !rows_given) return KGE_ERR_ARG;
  if (from_rows && !grads_given) return KGE_ERR_ARG;
  if (!c.in.pos || !c.in.neg || !c.ws.err_flag || c.in.batch < 1 || c.in.nneg < 1) return KGE_ERR_ARG;
  if (const kge_adam_desc* adam = c.adam) {
    if (!adam->entity.param || !adam->entity.exp_avg || !adam->entity.exp_avg_sq || !adam->relation.param ||
        !adam->relation.exp_avg || !adam->relation.exp_avg_sq)
      return KGE_ERR_ARG;
    if (adam->entity.param != m->entity_embedding || adam->relation.param != m->relation_embedding)
      return KGE_ERR_ARG;  // the update is in place on the model's own tables
    if (m->model == KGE_PROTATE && adam->modulus.param && adam->modulus.param != m->modulus) return KGE_ERR_ARG;
  }
  if (const kge_adagrad_desc* ag = c.adagrad) {
    if (ag->struct_size != (int32_t)sizeof(kge_adagrad_desc)) return KGE_ERR_ABI;
    if (!ag->entity.param || !ag->entity.state_sum || !ag->relation.param || !ag->relation.state_sum)
      return KGE_ERR_ARG;
    if (ag->entity.param != m->entity_embedding || ag->relation.param != m->relation_embedding) return KGE_ERR_ARG;
    if (m->model == KGE_PROTATE && ag->modulus.param && (ag->modulus.param != m->modulus || !ag->modulus.state_sum))
      return KGE_ERR_ARG;
    if (!(ag->eps > 0.f)) return KGE_ERR_ARG;  // (NaN too) eps = 0: an untouched all-zero row is NaN under the dense rule
    if (!(ag->lr >= 0.f) || isinf(ag->lr)) return KGE_ERR_ARG;
    if (ag->entity_rowwise != 0 && ag->entity_rowwise != 1) return KGE_ERR_ARG;
    view = adagrad_view(*ag);
    c.adam = &view;
    c.opt = ag->entity_rowwise ? OPT_ADAGRAD_ROW : OPT_ADAGRAD;
  }
  if (c.lazy) {
    // the lazy step's own refusals, behind the optimizer descriptor's (a
    // missing entity tensor is refused there): a whole single-process step
    // with its optimizer; no regulariser (its gradient is dense); no wide rows
    if (!c.adam || c.phases != KGE_PHASE_ALL || c.xstage != XS_NONE || c.e_begin != 0 || c.e_end >= 0)
      return KGE_ERR_ARG;
    if (c.loss.regularization != 0.f) return KGE_ERR_ARG;
    if (geo.ns == 0) return KGE_ERR_DIM;
  }
  {
    // (the row-wise entity state is one float per row, read and written by scalar accesses)
    kge_adam_desc streamed{};
    if (c.adam) streamed = *c.adam;
    if (c.opt == OPT_ADAGRAD_ROW) streamed.entity.exp_avg = streamed.entity.exp_avg_sq = nullptr;
    if (!grad_streams_aligned(geo, c.lazy ? nullptr : c.out.entity, c.out.relation, c.adam ? &streamed : nullptr))
      return KGE_ERR_ARG;
  }
  StepCall::Loss loss = c.loss;
  if (!loss.uni_weight && !loss.subsampling_weight) return KGE_ERR_ARG;
  if (m->model == KGE_PROTATE && !c.out.modulus && c.xstage != XS_ROWS_ONLY && !csr_only) return KGE_ERR_ARG;
  if (exchange && !loss.uni_weight && !loss.weight_sum) return KGE_ERR_ARG;  // the global Σw comes from the caller
  size_t need = 0;
  GradWs w = carve_grad(c.ws.workspace, m, c.in.batch, c.in.nneg, &need);
  LazyWs lz{};
  if (c.lazy) lz = carve_lazy(c.ws.workspace, m, c.in.batch, c.in.nneg, need, &need);
  if (!c.ws.workspace || c.ws.bytes < need) return KGE_ERR_WORKSPACE;
  if (exchange) {  // the exchanged per-row factors live in the caller's (gathered) buffers
    w.g = c.rows.g;
    w.dq = c.rows.dq;
    w.row_stats = c.rows.stats;
  }
  float* wsum_out = nullptr;
  if (!loss.uni_weight && !loss.weight_sum) {
    wsum_out = w.wsum;  // computed by k_build_q's first block, before k_row reads it
    loss.weight_sum = w.wsum;
  }
  Batch b = batch_of(c, geo, {c.in.neg, c.in.nneg}, w);
  b.lz = lz;
  RowArgs ra = row_args(b);
  ra.op = ROW_TRAIN;
  ra.adversarial = loss.adversarial ? 1 : 0;
  ra.adv_T = loss.adversarial_temperature;
  ra.uni_weight = loss.uni_weight ? 1 : 0;
  ra.uni_inv = 1.f / (float)(loss.uni_batch > 0 ? loss.uni_batch : c.in.batch);
  ra.sub_w = loss.subsampling_weight;
  ra.w_sum = loss.weight_sum;
  ra.wsum_out = wsum_out;
  ra.n_lds = (int)c.in.nneg;
  if (c.in.nneg > 8192) return KGE_ERR_DIM;
  if (c.phases < 1 || c.phases > KGE_PHASE_ALL) return KGE_ERR_ARG;
  const int64_t e_end = c.e_end < 0 ? m->nentity : c.e_end;
  if (c.e_begin < 0 || c.e_begin > e_end || e_end > m->nentity) return KGE_ERR_ARG;
  // (behind every argument check: rocPRIM's select always needs scratch, so 0 means
  // its size query failed — no usable device — and nothing can be launched)
  if (c.lazy && lz.sel_tmp_bytes == 0) return hip_status(hipErrorInvalidDevice);
  return run_grad(c, b, ra, fin_loss(loss, c.in.batch, c.out.losses, c.ws.err_flag));
}

// the range entries check their range before anything else
bool entity_range_ok(const kge_model_desc* m, int64_t begin, int64_t end) {
  return begin >= 0 && end >= begin && end <= (m ? m->nentity : 0);
}

// ================================================================= ranking

// Fast counting pass of the filtered ranking (path 0 = auto): the split-bf16
// MFMA tile for DistMult / ComplEx (path 1; the fp32 MFMA tile, path 4, when
// the split operands would pass 32-bit buffer offsets), the register tile for
// the others when the reduction length is a multiple of 4, the wave scan
// otherwise.  Every path ends in the same reference-order refinement, so all
// give the same ranks.
enum RankPath : int { RP_AUTO = 0, RP_MFMA = 1, RP_TILE = 2, RP_SCAN = 3, RP_MFMA32 = 4 };
int rank_path(const kge_model_desc* m, int requested) {
  const bool bil = (m->model == KGE_DISTMULT || m->model == KGE_COMPLEX);
  const bool cplx = (m->model == KGE_ROTATE || m->model == KGE_COMPLEX);
  const int K = cplx ? m->entity_dim / 2 : m->entity_dim;
  const bool al = aligned16(m->entity_embedding);
  // (the MFMA tiles address their operands through 32-bit buffer offsets)
  // (a table whose base is not 16-byte aligned takes the single-float paths
  // everywhere: the wave scan here, as DESIGN §3 has it for the other kernels)
  const bool x_ok = bil && al && (uint64_t)xsplit_elems(m->nentity, m->entity_dim) * 2u < 0x7FFFFFF0ull;
  const bool mfma_ok = bil && (m->entity_dim % 4 == 0) && al &&
                       (uint64_t)m->nentity * (uint64_t)m->entity_dim * 4u < 0xFFFFFF00ull;
  // (the register tile's counting pass reads a block's 64 rows — pRotatE:
  // their 2K-float phase rows — through one buffer descriptor)
  const bool tile_ok = (K % 4 == 0) && al && (uint64_t)64 * 2 * (uint64_t)m->entity_dim * 4u < 0x7FFFFFF0ull;
  if (requested == RP_MFMA) return x_ok ? RP_MFMA : -1;
  if (requested == RP_MFMA32) return mfma_ok ? RP_MFMA32 : -1;
  if (requested == RP_TILE) return tile_ok ? RP_TILE : -1;
  if (requested == RP_SCAN) return RP_SCAN;
  return x_ok ? RP_MFMA : mfma_ok ? RP_MFMA32 : (tile_ok ? RP_TILE : RP_SCAN);
}
constexpr int RANK_CAP = KGE_RANK_LIST_CAP;  // listed near-ties per query before the exact rescan takes over
static_assert(RANK_CAP <= 1024, "k_rank_refine's pRotatE screen holds 4 list entries per thread of 256");

struct RankWs {
  int64_t* tag;  // [8] what the table buffers below hold (k_rank_tag), then [3] the pRotatE list tag
  float *q, *qref, *s_true, *sref_true, *sref_hi, *delta, *stats;
  int64_t* true_id;
  int32_t *gt, *eq, *gtx, *eqx, *ucnt, *done, *ulist;
  uint32_t* bits;
  uint16_t *qs, *es;  // split-bf16 operands (DistMult / ComplEx)
  float *qph, *eph;   // pRotatE's phase tables for the register tile ([rows][K][2])
};
RankWs carve_rank(void* ws, const kge_model_desc* m, int64_t nq, size_t* bytes) {
  Carver c(ws);
  RankWs w;
  // the entity table's own buffers first, at offsets independent of nq, so a
  // later call on the same workspace can reuse them (KGE_RANK_REUSE_TABLE)
  w.tag = c.take<int64_t>(12);
  w.stats = c.take<float>(TS_NSTAT * (1 + TS_BLOCKS));  // [the TS_NSTAT maxima, per-block partials]
  // split-bf16 operands: only where the split tile can run (rank_path's x_ok)
  const bool xs = rank_path(m, RP_MFMA) == RP_MFMA;
  w.es = c.take<uint16_t>(xs ? xsplit_elems(m->nentity, m->entity_dim) : 0);
  // pRotatE's phase tables: only where its register tile can run
  const bool ph = m->model == KGE_PROTATE && rank_path(m, RP_TILE) == RP_TILE;
  w.eph = c.take<float>(ph ? 2 * m->nentity * (int64_t)m->entity_dim : 0);
  w.qs = c.take<uint16_t>(xs ? xsplit_elems(nq, m->entity_dim) : 0);
  w.qph = c.take<float>(ph ? 2 * nq * (int64_t)m->entity_dim : 0);
  w.q = c.take<float>(nq * (int64_t)m->entity_dim);
  w.qref = c.take<float>(nq * (int64_t)m->entity_dim);
  w.s_true = c.take<float>(nq);
  w.sref_true = c.take<float>(nq);
  w.sref_hi = c.take<float>(nq);
  w.delta = c.take<float>(nq);
  w.true_id = c.take<int64_t>(nq);
  w.gt = c.take<int32_t>(6 * nq);  // gt, eq, gtx, eqx, ucnt, done (zeroed by k_rank_prep)
  w.eq = w.gt ? w.gt + nq : nullptr;
  w.gtx = w.gt ? w.gt + 2 * nq : nullptr;
  w.eqx = w.gt ? w.gt + 3 * nq : nullptr;
  w.ucnt = w.gt ? w.gt + 4 * nq : nullptr;
  w.done = w.gt ? w.gt + 5 * nq : nullptr;
  w.ulist = c.take<int32_t>(nq * (int64_t)RANK_CAP);
  w.bits = c.take<uint32_t>(nq * ((m->nentity + 31) / 32));
  *bytes = c.off + 256;
  return w;
}

// Stages of one filtered-ranking call (kge_rank_filtered_ex, and pRotatE's
// three-call form with the caller's sin): RS_LIST runs everything up to the
// fast pass's near-tie lists and writes only listed_out; RS_ARGS writes the
// pRotatE phase sums of the listed items; RS_FINISH refines them with the
// caller's sin values, rescans overflowed windows and writes the ranks.
enum RankStage : int { RS_ALL = 0, RS_LIST = 1, RS_ARGS = 2, RS_FINISH = 3 };

// One ranking call as its entry describes it.
struct RankCall {
  const kge_model_desc* m;
  int64_t nq;
  void* workspace;
  size_t workspace_bytes;
  int32_t* err_flag;
  void* stream;
  RankStage stage = RS_ALL;
  int32_t mode = KGE_HEAD_BATCH;
  // both: head-batch then tail-batch of the same queries in one pass (kge_rank_filtered_both);
  // per-query arrays hold 2·nq entries, the head direction's first
  bool both = false;
  int32_t path = RP_AUTO;  // a RankPath, with the header's KGE_RANK_* flags
  const int64_t* queries = nullptr;
  const int64_t *filt_off = nullptr, *filt_ids = nullptr;
  const int64_t *filt_off_tail = nullptr, *filt_ids_tail = nullptr;  // (both) the tail direction's
  int64_t* ranks_out = nullptr;
  int32_t *ties_out = nullptr, *listed_out = nullptr;
  // pRotatE's three-call form
  const int64_t* item_off = nullptr;
  const float* sins = nullptr;
  float* args = nullptr;
};

// A validated ranking call: what its stages share.
struct RankRun {
  const kge_model_desc* m;
  Geom geo;
  const ModelOps* ops;
  hipStream_t s;
  RankStage stage;
  int mode;
  bool both, reuse, ftab;
  int rp;  // the fast pass (RankPath)
  int ndir;
  int64_t nq, nqt;  // queries per direction, and in the workspace
  int modes[2];
  const int64_t* queries;
  const int64_t* foff[2];
  const int64_t* fids[2];
  const float* trig;  // RotatE's reference cos | sin table (read with the row's slot geometry)
  int32_t* err;
  RankWs w;
  int K;
  int64_t Le, W;
  bool prot_tile;  // pRotatE on the register tile (its phase tables)
  // s_true in the reference's order after the window (k_rank_true_ref):
  // the split-bf16 path (instead of its gather pass), RotatE and pRotatE on
  // the register tile (after its gather pass, whose fast s_true sizes the
  // window's S; pRotatE: a point of the reference score's interval, the
  // window widened by its width); the window then covers the candidate's
  // error only
  bool true_ref;
  RankWin win;
  RankArgs a;   // 1. q, true ids (and, for the wave scan, s_true)
  RefArgs ra;   // the refinement's arguments (steps 4 and 6)
  EmitArgs ea;

  // the per-query arrays of direction d start o = d·nq entries in
  RankWin win_at(int64_t o) const {
    RankWin x = win;
    x.delta += o; x.ucnt += o; x.ulist += o * RANK_CAP;
    return x;
  }
  RankArgs rank_at(int d) const {
    RankArgs x = a;
    const int64_t o = d * nq;
    x.q += o * Le; x.s_true += o; x.true_id += o; x.gt += o; x.fbits += o * W; x.win = win_at(o);
    x.filt_off = foff[d]; x.filt_ids = fids[d];
    return x;
  }
  // a refinement stage: both directions' queries in one launch when both
  // (each block wholly in one direction, kge_kernels.inc ref_dir)
  int ref_stage(RefStage st) const { return launch_status(ops->rank_ref(both ? BOTH_DIRS : mode, st, ra, s)); }
  // one launch per direction of a mode-dependent stage (one direction unless both)
  template <typename F>
  int per_dir(F&& launch) const {
    for (int d = 0; d < ndir; ++d) {
      const int r = launch(d, modes[d]);
      if (r) return r;
    }
    return KGE_OK;
  }
};

// Argument checks and the workspace, in the order tests/test_capi_status.py
// pins.  An empty call (nq == 0) returns KGE_OK with nothing left to do.
int rank_validate(const RankCall& c, RankRun* r) {
  const kge_model_desc* m = c.m;
  int st = check_model(m, &r->geo);
  if (st) return st;
  if (!c.both && c.mode != KGE_HEAD_BATCH && c.mode != KGE_TAIL_BATCH) return KGE_ERR_MODE;
  if (!c.err_flag || c.nq < 0) return KGE_ERR_ARG;
  if (c.both && (c.stage != RS_ALL || !c.filt_off_tail)) return KGE_ERR_ARG;
  if (c.stage == RS_ALL || c.stage == RS_LIST) {
    if (!c.queries || !c.filt_off) return KGE_ERR_ARG;
  }
  if ((c.stage == RS_ALL || c.stage == RS_FINISH) && !c.ranks_out) return KGE_ERR_ARG;
  if (c.stage == RS_LIST && !c.listed_out) return KGE_ERR_ARG;
  if (c.stage == RS_ARGS && (!c.item_off || !c.args)) return KGE_ERR_ARG;
  if (c.stage == RS_FINISH && (!c.item_off || !c.sins)) return KGE_ERR_ARG;
  if (c.stage != RS_ALL && m->model != KGE_PROTATE) return KGE_ERR_MODEL;
  // KGE_RANK_REUSE_TABLE: the workspace already holds this entity table's
  // statistics and split operands from the previous call (the other direction)
  r->reuse = (c.path & KGE_RANK_REUSE_TABLE) != 0;
  r->ftab = (c.path & KGE_RANK_FILTER_TABLE) != 0;  // filt_off / filt_ids: the whole filter index
  const int path = c.path & ~(KGE_RANK_REUSE_TABLE | KGE_RANK_STAGE_LIST | KGE_RANK_FILTER_TABLE);
  if (path < RP_AUTO || path > RP_MFMA32) return KGE_ERR_ARG;
  if (c.nq == 0) return KGE_OK;
  if (c.nq > 65535) return KGE_ERR_DIM;  // the bitmap launch puts queries on grid.y
  r->rp = rank_path(m, path);
  if (r->rp < 0) return KGE_ERR_ARG;  // the requested fast pass cannot take these rows
  r->trig = (m->model == KGE_ROTATE) ? m->relation_trig : nullptr;
  if (r->trig && r->geo.vec == 4 && !aligned16(r->trig)) return KGE_ERR_ARG;
  r->ndir = c.both ? 2 : 1;
  r->nq = c.nq;
  r->nqt = r->ndir * c.nq;
  size_t need = 0;
  r->w = carve_rank(c.workspace, m, r->nqt, &need);
  if (!c.workspace || c.workspace_bytes < need) return KGE_ERR_WORKSPACE;
  return KGE_OK;
}

// the argument blocks of a validated call
void rank_bind(const RankCall& c, RankRun* r) {
  const kge_model_desc* m = c.m;
  const RankWs& w = r->w;
  r->m = m;
  r->ops = &ops_for(m->model);
  r->s = as_stream(c.stream);
  r->stage = c.stage;
  r->mode = c.mode;
  r->both = c.both;
  r->modes[0] = c.both ? (int)KGE_HEAD_BATCH : (int)c.mode;
  r->modes[1] = (int)KGE_TAIL_BATCH;
  r->queries = c.queries;
  r->foff[0] = c.filt_off; r->foff[1] = c.filt_off_tail;
  r->fids[0] = c.filt_ids; r->fids[1] = c.filt_ids_tail;
  r->err = c.err_flag;
  // (gt, eq, gtx, eqx, ucnt are zeroed by k_rank_prep: RankArgs.zero_counts)
  const bool cplx = (m->model == KGE_ROTATE || m->model == KGE_COMPLEX);
  r->K = cplx ? m->entity_dim / 2 : m->entity_dim;
  r->Le = m->entity_dim;
  r->W = (m->nentity + 31) / 32;
  r->prot_tile = m->model == KGE_PROTATE && r->rp == RP_TILE;
  r->true_ref = r->rp == RP_MFMA || (r->rp == RP_TILE && (m->model == KGE_ROTATE || r->prot_tile));
  r->win.delta = w.delta; r->win.ucnt = w.ucnt; r->win.ulist = w.ulist; r->win.cap = RANK_CAP;

  RankArgs& a = r->a;
  memset(&a, 0, sizeof(a));
  a.ent = m->entity_embedding; a.rel = m->relation_embedding; a.modulus = m->modulus;
  a.queries = c.queries; a.nq = c.nq; a.E = m->nentity; a.R = m->nrelation;
  a.Le = m->entity_dim; a.Lr = m->relation_dim; a.eg = r->geo.eg; a.c = consts_of(m);
  a.filt_off = c.filt_off; a.filt_ids = c.filt_ids;
  a.cpw = 64;
  a.q = w.q; a.s_true = w.s_true; a.true_id = w.true_id; a.gt = w.gt;
  a.fbits = w.bits; a.W = r->W; a.win = r->win; a.err = c.err_flag;
  a.prep_only = 1;
  a.zero_counts = 1;
  a.cstride = r->nqt;
  a.trig = r->trig;

  RefArgs& ra = r->ra;
  memset(&ra, 0, sizeof(ra));
  ra.ent = m->entity_embedding; ra.rel = m->relation_embedding; ra.modulus = m->modulus;
  ra.queries = c.queries; ra.nq = c.nq; ra.E = m->nentity; ra.R = m->nrelation;
  ra.Le = m->entity_dim; ra.Lr = m->relation_dim; ra.K = r->K; ra.c = a.c;
  ra.q = w.q; ra.qref = w.qref; ra.true_id = w.true_id; ra.s_true = w.s_true; ra.sref_true = w.sref_true;
  ra.s_true_w = w.s_true;
  ra.delta = w.delta; ra.stats = w.stats;
  ra.exact_fast = (m->model == KGE_TRANSE && r->rp == RP_TILE) ? 1 : 0;
  ra.ucnt = w.ucnt; ra.ulist = w.ulist; ra.cap = RANK_CAP;
  ra.fbits = w.bits; ra.W = a.W; ra.gt = w.gt; ra.eq = w.eq; ra.gtx = w.gtx; ra.eqx = w.eqx; ra.err = c.err_flag;
  ra.trig = r->trig;
  ra.item_off = c.item_off; ra.sins = c.sins; ra.args = c.args;
  ra.lib_sin = (c.stage != RS_ALL) ? 1 : 0;
  ra.sref_hi = w.sref_hi; ra.done = w.done;
  // the list tag of pRotatE's three-call form: the later stages must name the
  // list stage's mode, nq and table (a reused or switched
  // workspace gave wrong ranks with no error)
  const int64_t ltag_v[3] = {(int64_t)0x4B47454C00000000ll | (int64_t)c.mode, c.nq,
                             (int64_t)(uintptr_t)m->entity_embedding};
  ra.ltag = w.tag ? w.tag + 8 : nullptr;
  for (int k = 0; k < 3; ++k) ra.ltag_v[k] = ltag_v[k];
  // the split-bf16 tile's arithmetic error in units of u·‖q‖·max‖e‖ (kge_rank_mfma.hip): the
  // final add 1.2, the slab's three chained MFMAs 97.6, the running sum 1.02·nslab; the
  // split's own error is added per query from the pieces' norms (k_rank_window)
  const int64_t xns = xsplit_nslab(m->entity_dim);
  ra.fast_u = (r->rp != RP_MFMA) ? 0.f : (float)(98.8 + 1.02 * xns);

  EmitArgs& ea = r->ea;
  ea.gt = w.gt; ea.eq = w.eq; ea.gtx = w.gtx; ea.eqx = w.eqx; ea.ucnt = w.ucnt; ea.true_id = w.true_id;
  ea.nq = r->nqt; ea.cap = RANK_CAP; ea.ranks = c.ranks_out; ea.ties = c.ties_out; ea.listed = c.listed_out;
  ea.ltag = nullptr;
  for (int k = 0; k < 3; ++k) ea.ltag_v[k] = ltag_v[k];
}

// The entity table's work (tag, statistics, split or phase table): it depends
// on the table alone, and runs on ts — the caller's stream, or the side
// stream's between rk_fork and rk_join (rank_fast).  The statistics and split
// operands are reused only where the tag says this workspace already holds
// them for this table (k_rank_tag).
int rank_table(const RankRun& r, hipStream_t ts) {
  const kge_model_desc* m = r.m;
  const RankWs& w = r.w;
  const int rp = r.rp;
  const bool need_stats = (m->model == KGE_DISTMULT || m->model == KGE_COMPLEX || m->model == KGE_PROTATE);
  // the derived table: split-bf16 operands (kind 1) or pRotatE's phase table
  // (kind 2, tagged with its divisor's bits)
  const float kappa = r.a.c.kappa_p;
  int64_t kbits = 0;
  memcpy(&kbits, &kappa, sizeof(kappa));
  int st = launch_status(launch_rank_tag(w.tag, m->entity_embedding, m->nentity, m->entity_dim, r.reuse ? 1 : 0,
                                         need_stats ? 1 : 0, rp == RP_MFMA ? 1 : (r.prot_tile ? 2 : 0),
                                         r.prot_tile ? kbits : 0, ts));
  if (st) return st;
  if (rp == RP_MFMA && need_stats) {  // (DistMult, ComplEx) one read of the table for both
    st = launch_status(launch_split_stats(m->entity_embedding, m->nentity, m->entity_dim, w.es, w.stats, ts,
                                          w.tag + 5, w.tag + 6));
    if (st) return st;
  } else {
    if (need_stats) {
      st = launch_status(launch_table_stats(m->entity_embedding, m->nentity, m->entity_dim, w.stats, ts, w.tag + 5));
      if (st) return st;
    }
    if (rp == RP_MFMA) {
      st = launch_status(launch_split_bf16(m->entity_embedding, m->nentity, m->entity_dim, w.es, ts, w.tag + 6));
      if (st) return st;
    }
  }
  if (r.prot_tile) {
    st = launch_status(launch_prot_phase(m->entity_embedding, m->nentity, r.K, kappa, 1, w.eph, ts, w.tag + 6));
    if (st) return st;
  }
  return KGE_OK;
}

// The queries' work up to the fast pass, on the caller's stream (steps 1-5).
// rsd: the side stream the table's work runs on, joined here before the first
// launch that reads it, or null.
int rank_queries(RankRun& r, Side* rsd) {
  const kge_model_desc* m = r.m;
  const RankWs& w = r.w;
  const Geom& geo = r.geo;
  const ModelOps& ops = *r.ops;
  hipStream_t s = r.s;
  const int rp = r.rp;
  const int64_t nq = r.nq, nqt = r.nqt, W = r.W;
  int st;
  // 1. q, true ids (and, for the wave scan, s_true)
  if (r.both && geo.ns != 0) {  // both directions' q in one launch (rows ≤ 2048 floats)
    RankArgs x = r.a;
    x.both_dirs = 1;
    st = launch_status(ops.rank(KGE_HEAD_BATCH, geo.vec, geo.ns, x, s));
  } else {
    st = r.per_dir([&](int d, int md) { return launch_status(ops.rank(md, geo.vec, geo.ns, r.rank_at(d), s)); });
  }
  if (st) return st;
  // 2. excluded candidates (filtered ids + the true id) as a bitmap (both
  // directions in one launch where the row fits LDS)
  st = r.both ? launch_filter_bits_both(r.queries, r.ftab ? 1 : 0, r.foff[0], r.fids[0], r.foff[1], r.fids[1],
                                        w.true_id, nq, m->nentity, m->nrelation, w.bits, r.err, s)
              : -1;
  if (st > 0) return launch_status(st);
  if (st < 0) st = r.per_dir([&](int d, int md) {
    const int64_t o = d * nq;
    if (r.ftab)
      return launch_status(launch_filter_bits_tab(r.queries, md == KGE_HEAD_BATCH ? 1 : 0, r.foff[d], r.fids[d],
                                                  w.true_id + o, nq, m->nentity, m->nrelation, w.bits + o * W,
                                                  r.err, s));
    return launch_status(launch_filter_bits(r.foff[d], r.fids[d], w.true_id + o, nq, m->nentity, w.bits + o * W,
                                            r.err, s));
  });
  if (st) return st;
  // 3. the fast pass's own s_true (same instruction sequence as its candidates)
  TileArgs ta;
  ta.q = w.q; ta.ent = m->entity_embedding; ta.modulus = m->modulus;
  ta.nq = nq; ta.E = m->nentity; ta.Le = m->entity_dim; ta.K = r.K;
  ta.c = r.a.c; ta.true_id = w.true_id; ta.s_true = w.s_true;
  ta.fbits = w.bits; ta.W = W; ta.gt = w.gt; ta.win = r.win;
  ta.qph = w.qph; ta.eph = w.eph;
  auto tile_at = [&](int d) {
    TileArgs x = ta;
    const int64_t o = d * nq;
    x.q += o * r.Le; x.true_id += o; x.s_true += o; x.fbits += o * W; x.gt += o; x.win = r.win_at(o);
    if (x.qph) x.qph += o * 2 * (int64_t)r.K;
    return x;
  };
  if (r.prot_tile) {
    st = launch_status(launch_prot_phase(w.q, nqt, r.K, 0.f, 0, w.qph, s));
    if (st) return st;
  }
  if (rp == RP_MFMA) {
    // (q of both directions split in one launch: the tile is mode-independent)
    st = launch_status(launch_split_bf16(w.q, nqt, m->entity_dim, w.qs, s));
    if (!st && rsd) st = edge_wait(s, rsd->rk_join);  // join: everything below reads the table's work
    if (!st && !r.true_ref)
      st = launch_status(launch_rank_mfma_x(1, w.qs, w.es, nqt, m->nentity, m->entity_dim, w.true_id, w.s_true,
                                            w.bits, w.gt, r.win, s));
  } else {
    if (rsd && (st = edge_wait(s, rsd->rk_join))) return st;  // join: everything below reads the table's work
    if (rp == RP_MFMA32)
      st = launch_status(launch_rank_mfma(1, w.q, m->entity_embedding, nqt, m->nentity, m->entity_dim, w.true_id,
                                          w.s_true, w.bits, w.gt, r.win, s));
    else if (rp == RP_TILE)
      st = r.per_dir([&](int d, int md) { return launch_status(ops.rank_tile(md, 1, tile_at(d), s)); });
  }
  if (st) return st;
  // 4. near-tie windows and the reference-order q
  r.ra.true_exact = r.true_ref ? 1 : 0;
  st = r.ref_stage(RefStage::Window);
  if (st) return st;
  if (r.true_ref) {
    st = r.ref_stage(RefStage::TrueRef);
    if (st) return st;
  }
  // 5. fast counting pass: clear cases counted, near-ties listed (the MFMA
  // tiles take both directions' queries in one launch)
  g_rank_timer.mark(s, 1);  // (rank timer) 1: fast pass begins
  if (rp == RP_MFMA) {
    st = launch_status(launch_rank_mfma_x(0, w.qs, w.es, nqt, m->nentity, m->entity_dim, w.true_id, w.s_true,
                                          w.bits, w.gt, r.win, s));
  } else if (rp == RP_MFMA32) {
    st = launch_status(launch_rank_mfma(0, w.q, m->entity_embedding, nqt, m->nentity, m->entity_dim, w.true_id,
                                        w.s_true, w.bits, w.gt, r.win, s));
  } else if (rp == RP_TILE) {
    st = r.per_dir([&](int d, int md) { return launch_status(ops.rank_tile(md, 0, tile_at(d), s)); });
  } else {
    st = r.per_dir([&](int d, int md) {
      RankArgs x = r.rank_at(d);
      x.prep_only = 0;
      x.zero_counts = 0;
      return launch_status(ops.rank(md, geo.vec, geo.ns, x, s));
    });
  }
  if (st) return st;
  g_rank_timer.mark(s, 2);  // (rank timer) 2: fast pass ends
  return KGE_OK;
}

// Everything up to the near-tie lists (RS_ALL and RS_LIST).  KGE_RANK_SIDE=1
// (diagnostic, same bits) runs the table's work on the side stream beside the
// queries' q / bitmap / split (forked here, joined before the windows read the
// statistics): measured 1-2 % SLOWER than one stream (a ~130 µs dispatch gap
// before the counting tile after the cross-stream join; profiles/r06/rank), so
// the default is the caller's stream, the table's work queued first.
int rank_fast(RankRun& r) {
  g_rank_timer.mark(r.s, 0, r.ndir);  // (rank timer) 0: the call starts
  Side* rsd = env_int("KGE_RANK_SIDE", 0) != 0 ? side_for_device() : nullptr;
  int st;
  if (rsd && ((st = edge_record(rsd->rk_fork, r.s)) || (st = edge_wait(rsd->s, rsd->rk_fork)))) return st;
  st = rank_table(r, rsd ? rsd->s : r.s);
  if (st) return st;
  if (rsd && (st = edge_record(rsd->rk_join, rsd->s))) return st;
  return rank_queries(r, rsd);
}

// RS_LIST's tail: the lists stay in the workspace for RS_ARGS / RS_FINISH.
// pRotatE: every listed candidate's score as an interval under any library sin
// within one ulp, in the reference's order; those whose interval clears the
// true score's are decided now, only the rest go to the caller's sin.
// Overflowed windows: the same over every candidate (k_rank_exact_iv).
// KGE_RANK_SIN_SCREEN=0 (diagnostic): decide nothing.
int rank_list_tail(const RankRun& r) {
  RefArgs rs = r.ra;
  rs.screen = 1;
  rs.decide = env_int("KGE_RANK_SIN_SCREEN", 1) != 0 ? 1 : 0;
  rs.ucnt_w = r.w.ucnt;
  rs.ulist_w = r.w.ulist;
  int st = launch_status(r.ops->rank_ref(r.mode, RefStage::Refine, rs, r.s));
  if (st) return st;
  st = launch_status(r.ops->rank_ref(r.mode, RefStage::Interval, rs, r.s));
  if (st) return st;
  EmitArgs ea = r.ea;
  ea.ranks = nullptr;
  ea.ties = nullptr;
  ea.ltag = r.w.tag + 8;
  return launch_status(launch_rank_emit(ea, r.s));
}

// RS_ALL's and RS_FINISH's tail — 6. refinement in the reference's operation
// order; exact rescan on overflow (RS_FINISH: overflowed pRotatE windows were
// ranked by the list stage); the ranks
int rank_refine_tail(const RankRun& r) {
  int st = r.ref_stage(RefStage::Refine);
  if (st) return st;
  if (r.stage != RS_FINISH) {
    st = r.ref_stage(RefStage::Exact);
    if (st) return st;
  }
  st = launch_status(launch_rank_emit(r.ea, r.s));
  if (!st) g_rank_timer.mark(r.s, 3);  // (rank timer) 3: ranks written (the last of a call's marks counts)
  return st;
}

int rank_impl(const RankCall& c) {
  RankRun r;
  int st = rank_validate(c, &r);
  if (st || c.nq == 0) return st;
  rank_bind(c, &r);
  switch (c.stage) {
    case RS_ARGS:
      return launch_status(r.ops->rank_ref(c.mode, RefStage::SinArgs, r.ra, r.s));
    case RS_FINISH:
      return rank_refine_tail(r);
    case RS_LIST:
      st = rank_fast(r);
      return st ? st : rank_list_tail(r);
    case RS_ALL:
      st = rank_fast(r);
      return st ? st : rank_refine_tail(r);
  }
  return KGE_ERR_ARG;  // (not a RankStage)
}

// =================================================================== top-k

// The candidate parts of a top-k call: `parts` as asked (0: enough workgroups
// to fill the device's 256 CUs twice when the query blocks alone do not), at
// most 64 (a lane of the merge wave per part) and one per 64-candidate tile;
// span = candidates per part, a multiple of 64.
int topk_parts(const kge_model_desc* m, int64_t nq, int32_t parts, int64_t* span) {
  const int64_t tiles = (m->nentity + 63) / 64, qblocks = (nq + 63) / 64;
  int64_t p = parts > 0 ? parts : (512 + qblocks - 1) / (qblocks > 0 ? qblocks : 1);
  if (p > 64) p = 64;
  if (p > tiles) p = tiles;
  if (p < 1) p = 1;
  const int64_t tpp = (tiles + p - 1) / p;  // tiles per part
  *span = tpp * 64;
  return (int)((tiles + tpp - 1) / tpp);    // (no empty part)
}

struct TopkWs {
  float *q, *qph, *eph, *pscore;
  int64_t *qsan, *state;
  uint32_t* bits;
  int32_t* pid;
};
// v: the table the lists are taken over — the whole one (kge_topk, with qsan)
// or a shard's view (kge_topk_shard's LIST; no rows: nothing but q and the states)
TopkWs carve_topk(void* ws, const kge_model_desc* v, int64_t nq, int k, int parts, bool qsan, size_t* bytes) {
  Carver c(ws);
  TopkWs w;
  const bool ph = v->nentity > 0 && v->model == KGE_PROTATE && rank_path(v, RP_TILE) == RP_TILE;
  w.eph = c.take<float>(ph ? 2 * v->nentity * (int64_t)v->entity_dim : 0);
  w.qph = c.take<float>(ph ? 2 * nq * (int64_t)v->entity_dim : 0);
  w.q = c.take<float>(nq * (int64_t)v->entity_dim);
  w.qsan = qsan ? c.take<int64_t>(3 * nq) : nullptr;
  w.state = c.take<int64_t>(nq);
  w.bits = c.take<uint32_t>(nq * ((v->nentity + 31) / 32));
  w.pscore = c.take<float>(nq * (int64_t)parts * k);
  w.pid = c.take<int32_t>(nq * (int64_t)parts * k);
  *bytes = c.off + 256;
  return w;
}

// The partial lists of a top-k call over the table (or shard view) v, whose
// scan-kernel slots are vgeo's: each query's k best of every candidate part
// into w.pscore / w.pid, from w.q, the states and the bitmap — on the register
// tile (pRotatE: the phase tables first) or by the scan kernel.
int topk_lists(const kge_model_desc* v, const Geom& vgeo, const TopkWs& w, int md, int64_t nq, int k, int parts,
               int64_t span, bool tile, hipStream_t s) {
  const ModelOps& ops = ops_for(v->model);
  const int K = vgeo.cplx ? v->entity_dim / 2 : v->entity_dim;
  const int64_t W = (v->nentity + 31) / 32;
  const Consts c = consts_of(v);
  if (!tile) {
    TopkArgs a;
    memset(&a, 0, sizeof(a));
    a.ent = v->entity_embedding; a.modulus = v->modulus; a.nq = nq; a.E = v->nentity;
    a.Le = v->entity_dim; a.eg = vgeo.eg; a.c = c;
    a.q = w.q; a.state = w.state; a.fbits = w.bits; a.W = W;
    a.k = k; a.parts = parts; a.span = span; a.pscore = w.pscore; a.pid = w.pid;
    a.stage = 1;
    return launch_status(ops.topk(md, vgeo.vec, vgeo.ns, a, s));
  }
  if (v->model == KGE_PROTATE) {
    int st = launch_status(launch_prot_phase(v->entity_embedding, v->nentity, K, c.kappa_p, 1, w.eph, s));
    if (!st) st = launch_status(launch_prot_phase(w.q, nq, K, 0.f, 0, w.qph, s));
    if (st) return st;
  }
  TopkTileArgs b;
  memset(&b, 0, sizeof(b));
  b.t.q = w.q; b.t.ent = v->entity_embedding; b.t.modulus = v->modulus;
  b.t.nq = nq; b.t.E = v->nentity; b.t.Le = v->entity_dim; b.t.K = K;
  b.t.c = c; b.t.true_id = w.state; b.t.fbits = w.bits; b.t.W = W;
  b.t.qph = w.qph; b.t.eph = w.eph;
  b.k = k; b.parts = parts; b.span = span; b.pscore = w.pscore; b.pid = w.pid;
  return launch_status(ops.topk_tile(md, b, s));
}

int topk_impl(const kge_model_desc* m, int32_t mode, const int64_t* queries, int64_t nq, const int64_t* filt_off,
              const int64_t* filt_ids, int32_t k, int64_t* ids_out, float* scores_out, int32_t path_flags,
              int32_t parts_req, void* workspace, size_t workspace_bytes, int32_t* err_flag, void* stream) {
  Geom geo;
  int st = check_model(m, &geo);
  if (st) return st;
  if (mode != KGE_HEAD_BATCH && mode != KGE_TAIL_BATCH) return KGE_ERR_MODE;
  if (!queries || !ids_out || !scores_out || !err_flag || nq < 0 || parts_req < 0) return KGE_ERR_ARG;
  if (path_flags & ~(7 | KGE_RANK_FILTER_TABLE)) return KGE_ERR_ARG;
  const bool ftab = (path_flags & KGE_RANK_FILTER_TABLE) != 0;
  const int path = path_flags & 7;
  if (path != RP_AUTO && path != RP_TILE && path != RP_SCAN) return KGE_ERR_ARG;  // (no MFMA top-k)
  if (filt_off && !filt_ids) return KGE_ERR_ARG;
  if (nq == 0) return KGE_OK;
  if (k < 1 || k > KGE_TOPK_MAX_K) return KGE_ERR_DIM;
  if (nq > 65535) return KGE_ERR_DIM;  // the bitmap launch puts queries on grid.y
  if (geo.ns == 0) return KGE_ERR_DIM;  // rows over 2048 floats: not served
  const bool tile_ok = rank_path(m, RP_TILE) == RP_TILE;
  if (path == RP_TILE && !tile_ok) return KGE_ERR_ARG;
  const bool tile = (path == RP_SCAN) ? false : tile_ok;
  int64_t span = 0;
  const int parts = topk_parts(m, nq, parts_req, &span);
  size_t need = 0;
  const TopkWs w = carve_topk(workspace, m, nq, k, parts, true, &need);
  if (!workspace || workspace_bytes < need) return KGE_ERR_WORKSPACE;

  const ModelOps& ops = ops_for(m->model);
  hipStream_t s = as_stream(stream);
  const int md = kernel_mode(mode);
  const int64_t W = (m->nentity + 31) / 32;
  TopkArgs a;
  memset(&a, 0, sizeof(a));
  a.ent = m->entity_embedding; a.rel = m->relation_embedding; a.modulus = m->modulus;
  a.queries = queries; a.nq = nq; a.E = m->nentity; a.R = m->nrelation;
  a.Le = m->entity_dim; a.Lr = m->relation_dim; a.eg = geo.eg; a.c = consts_of(m);
  a.q = w.q; a.qsan = w.qsan; a.state = w.state; a.fbits = w.bits; a.W = W;
  a.k = k; a.parts = parts; a.span = span; a.pscore = w.pscore; a.pid = w.pid; a.err = err_flag;
  // 1. q and each query's state
  a.stage = 0;
  st = launch_status(ops.topk(md, geo.vec, geo.ns, a, s));
  if (st) return st;
  // 2. the excluded candidates as a bitmap (state stands in for the true id: negative, no bit)
  if (!filt_off)
    st = launch_status(launch_zero(w.bits, nq * W, s));
  else if (ftab)
    st = launch_status(launch_filter_bits_tab(w.qsan, mode == KGE_HEAD_BATCH ? 1 : 0, filt_off, filt_ids, w.state, nq,
                                              m->nentity, m->nrelation, w.bits, err_flag, s));
  else
    st = launch_status(launch_filter_bits(filt_off, filt_ids, w.state, nq, m->nentity, w.bits, err_flag, s));
  if (st) return st;
  // 3. the partial lists
  st = topk_lists(m, geo, w, md, nq, k, parts, span, tile, s);
  if (st) return st;
  // 4. the merge
  return launch_status(launch_topk_merge(w.pscore, w.pid, w.state, nq, parts, k, ids_out, scores_out, s));
}

// ---- sharded top-k (kge_topk_shard)
// LIST runs kge_topk's scan kernels on a shard-local view of the table: the
// entity pointer at the shard's first row, nentity = the shard's rows, ids local
// (ascending as the global ones, so the tie rule holds inside the shard); the
// shard's merge adds own_begin.  Alignment, and with it the path's fit and the
// 16-byte slots, is that of the shard's first row.
kge_model_desc shard_view(const kge_model_desc* m, int64_t own_begin, int64_t own_end) {
  kge_model_desc v = *m;
  v.entity_embedding = m->entity_embedding + own_begin * (int64_t)m->entity_dim;
  v.nentity = own_end - own_begin;
  return v;
}

// The model with `rows` (a shard entry's fixed_rows) for its entity table: *geo
// = the slots of the kernels that read those rows, by THEIR alignment and the
// relation table's.
int fixed_view(const kge_model_desc* m, const float* rows, Geom* geo) {
  kge_model_desc fv = *m;
  fv.entity_embedding = rows;
  return check_model(&fv, geo);
}

// The descriptor checks the shard entries share (D: kge_rank_shard_desc or
// kge_topk_shard_desc), in the order their statuses are documented in: a null
// descriptor, its struct_size, the entry's stage (stage_ok), the owned range,
// the flags outside flag_mask.
template <class D>
int check_shard_desc(const D* sh, bool stage_ok, int64_t nentity, int32_t flag_mask) {
  if (!sh) return KGE_ERR_ARG;
  if (sh->struct_size != (int32_t)sizeof(D)) return KGE_ERR_ABI;
  if (!stage_ok) return KGE_ERR_ARG;
  if (sh->own_begin < 0 || sh->own_end < sh->own_begin || sh->own_end > nentity) return KGE_ERR_ARG;
  if (sh->flags & ~flag_mask) return KGE_ERR_ARG;
  return KGE_OK;
}

// the shard's parts (topk_parts over its rows; an empty shard has none)
int topk_shard_parts(const kge_model_desc* v, int64_t rows, int64_t nq, int32_t parts, int64_t* span) {
  *span = 0;
  return rows > 0 ? topk_parts(v, nq, parts, span) : 0;
}

int topk_shard_impl(const kge_model_desc* m, int32_t mode, const kge_topk_shard_desc* sh, int32_t stage,
                    const int64_t* queries, int64_t nq, void* workspace, size_t workspace_bytes, int32_t* err_flag,
                    void* stream) {
  Geom geo;
  int st = check_model(m, &geo);
  if (st) return st;
  if (mode != KGE_HEAD_BATCH && mode != KGE_TAIL_BATCH) return KGE_ERR_MODE;
  const bool list = stage == KGE_TSHARD_LIST;
  st = check_shard_desc(sh, list || stage == KGE_TSHARD_MERGE, m->nentity, 7 | KGE_RANK_FILTER_TABLE);
  if (st) return st;
  const int path = sh->flags & 7;
  if (path != RP_AUTO && path != RP_TILE && path != RP_SCAN) return KGE_ERR_ARG;  // (no MFMA top-k)
  if (sh->parts < 0) return KGE_ERR_ARG;
  if (!queries || !err_flag) return KGE_ERR_ARG;
  if (list && (!sh->fixed_rows || !sh->list_scores || !sh->list_ids)) return KGE_ERR_ARG;
  if (!list && (!sh->lists_scores || !sh->lists_ids || !sh->ids_out || !sh->scores_out)) return KGE_ERR_ARG;
  if (sh->filt_off && !sh->filt_ids) return KGE_ERR_ARG;
  if (nq < 0) return KGE_ERR_ARG;
  if (nq == 0) return KGE_OK;
  const int k = sh->k;
  if (k < 1 || k > KGE_TOPK_MAX_K) return KGE_ERR_DIM;
  if (list && nq > 65535) return KGE_ERR_DIM;  // kge_topk's ceiling, kept: the two take the same blocks of queries
  if (!list && (sh->world < 1 || sh->world > 64)) return KGE_ERR_DIM;  // a lane of the merge wave per list
  if (geo.ns == 0) return KGE_ERR_DIM;  // rows over 2048 floats: not served
  hipStream_t s = as_stream(stream);
  const int md = kernel_mode(mode);

  if (!list) {
    if (!workspace || workspace_bytes < 256) return KGE_ERR_WORKSPACE;
    TopkShardMergeArgs g;
    memset(&g, 0, sizeof(g));
    g.ps = sh->lists_scores; g.pi = sh->lists_ids; g.nq = nq; g.stride_l = nq * (int64_t)k; g.stride_q = k;
    g.nlists = sh->world; g.k = k; g.final = 1; g.queries = queries; g.head = mode == KGE_HEAD_BATCH ? 1 : 0;
    g.E = m->nentity; g.R = m->nrelation; g.ids_out = sh->ids_out; g.scores_out = sh->scores_out;
    return launch_status(launch_topk_merge_shard(g, s));
  }

  const int64_t rows = sh->own_end - sh->own_begin;
  const kge_model_desc v = shard_view(m, sh->own_begin, sh->own_end);
  const bool tile_ok = rank_path(&v, RP_TILE) == RP_TILE;
  if (path == RP_TILE && !tile_ok) return KGE_ERR_ARG;
  const bool tile = (path == RP_SCAN) ? false : tile_ok;
  int64_t span = 0;
  const int parts = topk_shard_parts(&v, rows, nq, sh->parts, &span);
  size_t need = 0;
  const TopkWs w = carve_topk(workspace, &v, nq, k, parts, false, &need);
  if (!workspace || workspace_bytes < need) return KGE_ERR_WORKSPACE;

  const ModelOps& ops = ops_for(m->model);
  const int64_t W = (rows + 31) / 32;
  // 1. q and each query's state, from fixed_rows (16-byte slots by ITS alignment and the relation table's)
  Geom fgeo;
  st = fixed_view(m, sh->fixed_rows, &fgeo);
  if (st) return st;
  TopkArgs a;
  memset(&a, 0, sizeof(a));
  a.rel = m->relation_embedding; a.modulus = m->modulus; a.fixed_rows = sh->fixed_rows;
  a.queries = queries; a.nq = nq; a.E = m->nentity; a.R = m->nrelation;
  a.Le = m->entity_dim; a.Lr = m->relation_dim; a.eg = fgeo.eg; a.c = consts_of(m);
  a.q = w.q; a.state = w.state; a.err = err_flag;
  a.stage = 2;
  st = launch_status(ops.topk(md, fgeo.vec, fgeo.ns, a, s));
  if (st) return st;
  // 2. the excluded rows of the shard as a bitmap
  if (sh->filt_off)
    st = launch_status(launch_filter_bits_range(queries, mode == KGE_HEAD_BATCH ? 1 : 0,
                                                (sh->flags & KGE_RANK_FILTER_TABLE) ? 1 : 0, sh->filt_off,
                                                sh->filt_ids, nq, m->nentity, m->nrelation, sh->own_begin,
                                                sh->own_end, w.bits, err_flag, s));
  else
    st = launch_status(launch_zero(w.bits, nq * W, s));
  if (st) return st;
  // 3. the partial lists over the shard's view (an empty shard: none)
  if (rows > 0) {
    Geom vgeo;
    st = check_model(&v, &vgeo);
    if (!st) st = topk_lists(&v, vgeo, w, md, nq, k, parts, span, tile, s);
    if (st) return st;
  }
  // 4. the shard's list, global ids
  TopkShardMergeArgs g;
  memset(&g, 0, sizeof(g));
  g.ps = w.pscore; g.pi = w.pid; g.nq = nq; g.stride_l = k; g.stride_q = (int64_t)parts * k;
  g.nlists = parts; g.k = k; g.final = 0; g.id_base = (int32_t)sh->own_begin;
  g.ls = sh->list_scores; g.li = sh->list_ids;
  return launch_status(launch_topk_merge_shard(g, s));
}

// ---- the chunk rule of the row-walk entries (kge_rank_candidates,
// kge_rank_relations, kge_rank_shard's COUNT)
// The chunks of a query's n items (candidates of its list, relations, owned
// rows): one when the queries alone fill the device (256 CUs × 8 workgroups),
// else enough to, of at least 64 items each; *cpc = items per chunk, at most
// cpc_max (the chunk's scores sit in LDS).  equal_floor: never fewer chunks
// than cpc_max demands, so they come out of equal size (R = 1345 is 673 + 672,
// not 1024 + 321: every chunk stages its fixed rows once more) — the candidate
// lists go without it.  env_name (diagnostic): items per chunk; the counts are
// integer sums, so no geometry changes a result.
int64_t work_chunks(const char* env_name, int64_t nq, int64_t n, int cpc_max, bool equal_floor, int* cpc) {
  int64_t per = env_int(env_name, 0);
  if (per < 1) {
    const int64_t want = (2048 + nq - 1) / nq, most = (n + 63) / 64, least = (n + cpc_max - 1) / cpc_max;
    int64_t chunks = want < most ? want : most;
    if (equal_floor && chunks < least) chunks = least;
    per = (n + chunks - 1) / chunks;
  }
  if (per > cpc_max) per = cpc_max;
  *cpc = (int)per;
  return (n + per - 1) / per;
}

// ---- ranking against candidate lists (kge_rank_candidates)
struct CandWs {
  int32_t *gt, *eq;  // [nq] each, adjacent: one memset
  float* qref;       // [nq, Le], rows read in place only
};
CandWs carve_cand(void* ws, const kge_model_desc* m, int64_t nq, size_t* bytes) {
  Carver c(ws);
  CandWs w;
  w.gt = c.take<int32_t>(2 * nq);
  w.eq = w.gt ? w.gt + nq : nullptr;
  w.qref = c.take<float>(cand_slots(m->entity_dim) == 0 ? nq * (int64_t)m->entity_dim : 0);
  *bytes = c.off + 256;
  return w;
}

int rank_cand_impl(const kge_model_desc* m, int32_t mode, const int64_t* queries, int64_t nq, const int64_t* cand,
                   int64_t ncand, int64_t* ranks_out, int32_t* ties_out, void* workspace, size_t workspace_bytes,
                   int32_t* err_flag, void* stream) {
  Geom geo;
  int st = check_model(m, &geo);
  if (st) return st;
  if (mode != KGE_HEAD_BATCH && mode != KGE_TAIL_BATCH) return KGE_ERR_MODE;
  if (!queries || !cand || !ranks_out || !err_flag || nq < 0 || ncand < 1) return KGE_ERR_ARG;
  if (nq == 0) return KGE_OK;
  int cpc = 0;
  const int64_t chunks = work_chunks("KGE_RANK_CAND_CHUNK", nq, ncand, CAND_CPC_MAX, false, &cpc);
  if (nq > 0x7fffffff / chunks) return KGE_ERR_DIM;  // (query, chunk) work items on grid.x
  size_t need = 0;
  const CandWs w = carve_cand(workspace, m, nq, &need);
  if (!workspace || workspace_bytes < need) return KGE_ERR_WORKSPACE;

  hipStream_t s = as_stream(stream);
  CandArgs a;
  memset(&a, 0, sizeof(a));
  a.ent = m->entity_embedding; a.rel = m->relation_embedding; a.modulus = m->modulus;
  a.trig = (m->model == KGE_ROTATE) ? m->relation_trig : nullptr;
  a.queries = queries; a.cand = cand; a.nq = nq; a.C = ncand; a.E = m->nentity; a.R = m->nrelation;
  a.Le = m->entity_dim; a.Lr = m->relation_dim; a.K = geo.cplx ? m->entity_dim / 2 : m->entity_dim;
  a.c = consts_of(m);
  a.chunks = chunks; a.cpc = cpc;
  // 16-byte slots by the header's rule: the row span a multiple of 4, both tables aligned
  a.vec4 = (a.K % 4 == 0) && aligned16(m->entity_embedding) && aligned16(m->relation_embedding);
  a.nslot = cand_slots(a.Le);
  a.in_place = a.nslot == 0;
  a.qref = w.qref; a.gt = w.gt; a.eq = w.eq; a.err = err_flag;
  st = launch_status(launch_zero(w.gt, 2 * nq, s));  // (gt | eq)
  if (st) return st;
  st = launch_status(ops_for(m->model).rank_cand(kernel_mode(mode), a, s));
  if (st) return st;
  return launch_status(launch_rank_cand_emit(queries, nq, m->nentity, m->nrelation, w.gt, w.eq, ranks_out, ties_out, s));
}

// ---- relation prediction (kge_rank_relations)
struct RelWs {
  int32_t *gt, *eq;  // [nq] each, adjacent: one memset
  float* trig;       // [R, 2, Lr], RotatE without a caller's table only
};
RelWs carve_rel(void* ws, const kge_model_desc* m, int64_t nq, size_t* bytes) {
  Carver c(ws);
  RelWs w;
  w.gt = c.take<int32_t>(2 * nq);
  w.eq = w.gt ? w.gt + nq : nullptr;
  const bool table = m->model == KGE_ROTATE && !m->relation_trig;
  w.trig = c.take<float>(table ? (size_t)m->nrelation * 2 * (size_t)m->relation_dim : 0);
  *bytes = c.off + 256;
  return w;
}

int rank_rel_impl(const kge_model_desc* m, const int64_t* queries, int64_t nq, const int64_t* filt_off,
                  const int64_t* filt_ids, int64_t* ranks_out, int32_t* ties_out, float* scores_out, void* workspace,
                  size_t workspace_bytes, int32_t* err_flag, void* stream) {
  Geom geo;
  int st = check_model(m, &geo);
  if (st) return st;
  if (!queries || !ranks_out || !err_flag) return KGE_ERR_ARG;
  if (nq < 0) return KGE_ERR_ARG;
  if ((filt_off == nullptr) != (filt_ids == nullptr)) return KGE_ERR_ARG;
  if (nq == 0) return KGE_OK;
  int cpc = 0;
  const int64_t chunks = work_chunks("KGE_RANK_REL_CHUNK", nq, m->nrelation, REL_CPC_MAX, true, &cpc);
  if (nq > 0x7fffffff / chunks) return KGE_ERR_DIM;  // (query, chunk) work items on grid.x
  size_t need = 0;
  const RelWs w = carve_rel(workspace, m, nq, &need);
  if (!workspace || workspace_bytes < need) return KGE_ERR_WORKSPACE;

  hipStream_t s = as_stream(stream);
  RelRankArgs a;
  memset(&a, 0, sizeof(a));
  a.ent = m->entity_embedding; a.rel = m->relation_embedding; a.modulus = m->modulus;
  a.queries = queries; a.filt_off = filt_off; a.filt_ids = filt_ids;
  a.nq = nq; a.E = m->nentity; a.R = m->nrelation;
  a.Le = m->entity_dim; a.Lr = m->relation_dim; a.K = geo.cplx ? m->entity_dim / 2 : m->entity_dim;
  a.c = consts_of(m);
  a.chunks = chunks; a.cpc = cpc;
  if (m->model == KGE_ROTATE) {
    a.trig = m->relation_trig;
    if (!a.trig) {
      st = launch_status(launch_rel_trig_table(m->relation_embedding, m->nrelation, m->relation_dim, a.c.kappa, w.trig, s));
      if (st) return st;
      a.trig = w.trig;
    }
  }
  // 16-byte slots: the row span a multiple of 4, the entity table and the table
  // the relation rows come from (RotatE: the trig table) aligned
  a.vec4 = (a.K % 4 == 0) && aligned16(m->entity_embedding) &&
           aligned16(m->model == KGE_ROTATE ? a.trig : m->relation_embedding);
  a.nslot = rel_slots(a.Le);
  a.in_place = a.nslot == 0;
  a.scores = scores_out; a.gt = w.gt; a.eq = w.eq; a.err = err_flag;
  st = launch_status(launch_zero(w.gt, 2 * nq, s));  // (gt | eq)
  if (st) return st;
  st = launch_status(ops_for(m->model).rank_rel(a, s));
  if (st) return st;
  // (r = -1 is "not in [0, R)" to the emit kernel: rank 0, ties 0)
  return launch_status(launch_rank_cand_emit(queries, nq, m->nentity, m->nrelation, w.gt, w.eq, ranks_out, ties_out, s));
}

// ---- sharded filtered ranking (kge_rank_shard)
struct ShardWs {
  float* qref;  // [nq, Le], rows read in place only
};
ShardWs carve_shard(void* ws, const kge_model_desc* m, int64_t nq, size_t* bytes) {
  Carver c(ws);
  ShardWs w;
  w.qref = c.take<float>(shard_slots(m->entity_dim) == 0 ? nq * (int64_t)m->entity_dim : 0);
  *bytes = c.off + 256;
  return w;
}

int rank_shard_impl(const kge_model_desc* m, int32_t mode, const kge_rank_shard_desc* sh, int32_t stage,
                    const int64_t* queries, int64_t nq, void* workspace, size_t workspace_bytes, int32_t* err_flag,
                    void* stream) {
  Geom geo;
  int st = check_model(m, &geo);
  if (st) return st;
  if (mode != KGE_HEAD_BATCH && mode != KGE_TAIL_BATCH) return KGE_ERR_MODE;
  st = check_shard_desc(sh, stage == KGE_RSHARD_ROWS || stage == KGE_RSHARD_TRUE || stage == KGE_RSHARD_COUNT,
                        m->nentity, KGE_RANK_FILTER_TABLE);
  if (st) return st;
  if (!queries || !err_flag || nq < 0) return KGE_ERR_ARG;
  if (!sh->fixed_rows) return KGE_ERR_ARG;
  if (stage >= KGE_RSHARD_TRUE && !sh->s_true) return KGE_ERR_ARG;
  if (stage == KGE_RSHARD_COUNT && (!sh->counts || !sh->filt_off || !sh->filt_ids)) return KGE_ERR_ARG;
  if (nq == 0) return KGE_OK;
  const int64_t rows = sh->own_end - sh->own_begin;
  int cpc = 1;
  int64_t chunks = 1;  // (an empty shard: one chunk of no rows, which still flags the bad queries)
  if (stage == KGE_RSHARD_COUNT && rows > 0) 
    chunks = work_chunks("KGE_RANK_SHARD_CHUNK", nq, rows, SHARD_CPC_MAX, true, &cpc);
  if (nq > 0x7fffffff / chunks) return KGE_ERR_DIM;  // queries (COUNT: (chunk, query) work items) on grid.x
  size_t need = 0;
  const ShardWs w = carve_shard(workspace, m, nq, &need);
  if (!workspace || workspace_bytes < need) return KGE_ERR_WORKSPACE;

  hipStream_t s = as_stream(stream);
  ShardArgs a;
  memset(&a, 0, sizeof(a));
  a.ent = m->entity_embedding; a.rel = m->relation_embedding; a.modulus = m->modulus;
  a.trig = (m->model == KGE_ROTATE) ? m->relation_trig : nullptr;
  a.queries = queries; a.filt_off = sh->filt_off; a.filt_ids = sh->filt_ids;
  a.ftab = (sh->flags & KGE_RANK_FILTER_TABLE) ? 1 : 0;
  a.nq = nq; a.E = m->nentity; a.R = m->nrelation; a.own_lo = sh->own_begin; a.own_hi = sh->own_end;
  a.Le = m->entity_dim; a.Lr = m->relation_dim; a.K = geo.cplx ? m->entity_dim / 2 : m->entity_dim;
  a.c = consts_of(m);
  a.chunks = chunks; a.cpc = cpc;
  // 16-byte slots by the header's rule: the row span a multiple of 4, both tables aligned
  // (rows are then a multiple of 16 bytes, so the shard is aligned as its base pointer is)
  a.vec4 = (a.K % 4 == 0) && aligned16(m->entity_embedding) && aligned16(m->relation_embedding);
  a.nslot = shard_slots(a.Le);
  a.in_place = a.nslot == 0;
  a.qw = env_int("KGE_RANK_SHARD_QPW", 1);  // (diagnostic: queries per workgroup, 2 or 4; the same counts)
  a.fixed_rows = sh->fixed_rows; a.s_true = sh->s_true; a.qref = w.qref; a.counts = sh->counts; a.err = err_flag;
  if (stage == KGE_RSHARD_COUNT) {
    st = launch_status(launch_zero(sh->counts, 4 * nq, s));  // [2, nq] int64
    if (st) return st;
  }
  return launch_status(ops_for(m->model).rank_shard(kernel_mode(mode), stage, a, s));
}

// ---- sharded ranking against candidate lists (kge_rank_candidates_shard)
struct CandShardWs {
  float* qref;  // [nq, Le], rows read in place only
};
CandShardWs carve_cand_shard(void* ws, const kge_model_desc* m, int64_t nq, size_t* bytes) {
  Carver c(ws);
  CandShardWs w;
  w.qref = c.take<float>(cand_shard_slots(m->entity_dim) == 0 ? nq * (int64_t)m->entity_dim : 0);
  *bytes = c.off + 256;
  return w;
}

int rank_cand_shard_impl(const kge_model_desc* m, int32_t mode, const kge_rank_cand_shard_desc* sh,
                         const int64_t* queries, int64_t nq, const int64_t* cand, int64_t ncand, void* workspace,
                         size_t workspace_bytes, int32_t* err_flag, void* stream) {
  Geom geo;
  int st = check_model(m, &geo);
  if (st) return st;
  if (mode != KGE_HEAD_BATCH && mode != KGE_TAIL_BATCH) return KGE_ERR_MODE;
  st = check_shard_desc(sh, true, m->nentity, 0);
  if (st) return st;
  if (!queries || !cand || !err_flag || !sh->fixed_rows || !sh->s_true || !sh->counts || nq < 0 || ncand < 1)
    return KGE_ERR_ARG;
  if (nq == 0) return KGE_OK;
  int cpc = 0;
  const int64_t chunks = work_chunks("KGE_RANK_CAND_SHARD_CHUNK", nq, ncand, CAND_SHARD_CPC_MAX, false, &cpc);
  if (nq > 0x7fffffff / chunks) return KGE_ERR_DIM;  // (query, chunk) work items on grid.x
  size_t need = 0;
  const CandShardWs w = carve_cand_shard(workspace, m, nq, &need);
  if (!workspace || workspace_bytes < need) return KGE_ERR_WORKSPACE;

  hipStream_t s = as_stream(stream);
  CandShardArgs a;
  memset(&a, 0, sizeof(a));
  a.ent = m->entity_embedding; a.rel = m->relation_embedding; a.modulus = m->modulus;
  a.trig = (m->model == KGE_ROTATE) ? m->relation_trig : nullptr;
  a.queries = queries; a.cand = cand; a.nq = nq; a.C = ncand; a.E = m->nentity; a.R = m->nrelation;
  a.own_lo = sh->own_begin; a.own_hi = sh->own_end;
  a.Le = m->entity_dim; a.Lr = m->relation_dim; a.K = geo.cplx ? m->entity_dim / 2 : m->entity_dim;
  a.c = consts_of(m);
  a.chunks = chunks; a.cpc = cpc;
  // 16-byte slots by the header's rule: the row span a multiple of 4, both tables aligned
  // (rows are then a multiple of 16 bytes, so the shard is aligned as its base pointer is)
  a.vec4 = (a.K % 4 == 0) && aligned16(m->entity_embedding) && aligned16(m->relation_embedding);
  a.nslot = cand_shard_slots(a.Le);
  a.in_place = a.nslot == 0;
  a.fixed_rows = sh->fixed_rows; a.s_true = sh->s_true; a.qref = w.qref; a.counts = sh->counts; a.err = err_flag;
  st = launch_status(launch_zero(sh->counts, 4 * nq, s));  // [2, nq] int64
  if (st) return st;
  return launch_status(ops_for(m->model).rank_cand_shard(kernel_mode(mode), a, s));
}

// ---- sharded filtered ranking, the fast counting pass (kge_rank_shard_fast)
// KGE_RSHARD_COUNT's counts from the single-table pipeline's fast pass on the
// shard's view (shard_view, as kge_topk_shard): rank_path's rules applied to
// the shard's first row.  pRotatE, rows the register prep kernel does not hold
// and a trig table its 16-byte slots cannot read resolve to the exact stage.
// fgeo: the prep kernel's slots (fixed_rows' alignment and the relation table's).
int shard_fast_path(const kge_model_desc* m, const kge_rank_shard_desc* sh, int requested, Geom* fgeo) {
  if (requested == RP_SCAN) return RP_SCAN;
  if (requested < RP_AUTO || requested > RP_TILE) return -1;  // (the fp32 MFMA tile is not offered)
  const kge_model_desc v = shard_view(m, sh->own_begin, sh->own_end);
  Geom g;
  bool fast = m->model != KGE_PROTATE && fixed_view(m, sh->fixed_rows, &g) == KGE_OK && g.ns != 0;
  if (fast && m->model == KGE_ROTATE && m->relation_trig && g.vec == 4 && !aligned16(m->relation_trig)) fast = false;
  if (fgeo) *fgeo = g;
  const bool x_ok = fast && rank_path(&v, RP_MFMA) == RP_MFMA;
  const bool tile_ok = fast && rank_path(&v, RP_TILE) == RP_TILE;
  if (requested == RP_MFMA) return x_ok ? RP_MFMA : -1;
  if (requested == RP_TILE) return tile_ok ? RP_TILE : -1;
  return x_ok ? RP_MFMA : (tile_ok ? RP_TILE : RP_SCAN);
}

struct ShardFastWs {
  float *stats, *q, *qref, *s_true, *delta;
  uint16_t *es, *qs;  // split-bf16 operands of the own rows and of q (path 1)
  int64_t* state;
  int32_t *gt, *ucnt, *ulist;
  uint32_t* bits;
};
ShardFastWs carve_shard_fast(void* ws, const kge_model_desc* m, int64_t rows, int64_t nq, int rp, size_t* bytes) {
  Carver c(ws);
  ShardFastWs w;
  const bool xs = rp == RP_MFMA;
  w.stats = c.take<float>(TS_NSTAT * (1 + TS_BLOCKS));
  w.es = c.take<uint16_t>(xs ? xsplit_elems(rows, m->entity_dim) : 0);
  w.qs = c.take<uint16_t>(xs ? xsplit_elems(nq, m->entity_dim) : 0);
  w.q = c.take<float>(nq * (int64_t)m->entity_dim);
  w.qref = c.take<float>(nq * (int64_t)m->entity_dim);
  w.s_true = c.take<float>(nq);
  w.delta = c.take<float>(nq);
  w.state = c.take<int64_t>(nq);
  w.gt = c.take<int32_t>(2 * nq);  // gt | ucnt (zeroed by k_rsf_prep)
  w.ucnt = w.gt ? w.gt + nq : nullptr;
  w.ulist = c.take<int32_t>(nq * (int64_t)RANK_CAP);
  w.bits = c.take<uint32_t>(nq * ((rows + 31) / 32));
  *bytes = c.off + 256;
  return w;
}

// The checks every call of the entry makes before it resolves the path, in
// kge_rank_shard's order; *path = the requested path.
int shard_fast_check(const kge_model_desc* m, int32_t mode, const kge_rank_shard_desc* sh, Geom* geo, int* path) {
  int st = check_model(m, geo);
  if (st) return st;
  if (mode != KGE_HEAD_BATCH && mode != KGE_TAIL_BATCH) return KGE_ERR_MODE;
  st = check_shard_desc(sh, true, m->nentity, 7 | KGE_RANK_FILTER_TABLE);
  if (st) return st;
  *path = sh->flags & 7;
  if (*path > RP_MFMA32) return KGE_ERR_ARG;
  return KGE_OK;
}

int rank_shard_fast_impl(const kge_model_desc* m, int32_t mode, const kge_rank_shard_desc* sh, const int64_t* queries,
                         int64_t nq, int32_t* listed_out, void* workspace, size_t workspace_bytes, int32_t* err_flag,
                         void* stream) {
  Geom geo, fgeo;
  int path = 0;
  int st = shard_fast_check(m, mode, sh, &geo, &path);
  if (st) return st;
  if (!queries || !err_flag || nq < 0) return KGE_ERR_ARG;
  if (!sh->fixed_rows || !sh->s_true || !sh->counts || !sh->filt_off || !sh->filt_ids) return KGE_ERR_ARG;
  if (nq == 0) return KGE_OK;
  const int rp = shard_fast_path(m, sh, path, &fgeo);
  hipStream_t s = as_stream(stream);
  if (rp == RP_SCAN) {  // the exact stage's own kernel, grid rule and workspace
    kge_rank_shard_desc x = *sh;
    x.flags = sh->flags & KGE_RANK_FILTER_TABLE;
    st = rank_shard_impl(m, mode, &x, KGE_RSHARD_COUNT, queries, nq, workspace, workspace_bytes, err_flag, stream);
    if (st || !listed_out) return st;
    return launch_status(launch_zero(listed_out, nq, s));
  }
  if (rp > 0 && nq > 65535) return KGE_ERR_DIM;  // the bitmap and tile launches put queries on grid.y
  if (rp < 0) return KGE_ERR_ARG;                // the requested fast pass cannot take these rows
  const int64_t rows = sh->own_end - sh->own_begin;
  const kge_model_desc v = shard_view(m, sh->own_begin, sh->own_end);
  size_t need = 0;
  const ShardFastWs w = carve_shard_fast(workspace, m, rows, nq, rp, &need);
  if (!workspace || workspace_bytes < need) return KGE_ERR_WORKSPACE;

  const ModelOps& ops = ops_for(m->model);
  const int md = kernel_mode(mode);
  const int K = geo.cplx ? m->entity_dim / 2 : m->entity_dim;
  const int64_t W = (rows + 31) / 32;
  ShardFastArgs a;
  memset(&a, 0, sizeof(a));
  RefArgs& f = a.r;
  f.ent = v.entity_embedding; f.rel = m->relation_embedding; f.modulus = m->modulus;
  f.queries = queries; f.nq = nq; f.E = rows; f.R = m->nrelation;
  f.Le = m->entity_dim; f.Lr = m->relation_dim; f.K = K; f.c = consts_of(m);
  f.q = w.q; f.qref = w.qref; f.true_id = w.state; f.s_true = w.s_true;
  f.true_exact = 1;  // s_true is the reduced reference-order score: δ covers the candidate's error only
  f.delta = w.delta; f.stats = w.stats;
  // TransE on the register tile: q from the same row bits by the same build_q, the tile's sequential sum
  // from 0 — the bits ref_score_half gave s_true: δ = 0, exact ties are listed
  f.exact_fast = (m->model == KGE_TRANSE && rp == RP_TILE) ? 1 : 0;
  f.ucnt = w.ucnt; f.ulist = w.ulist; f.cap = RANK_CAP;
  f.fbits = w.bits; f.W = W; f.gt = w.gt; f.err = err_flag;
  f.trig = (m->model == KGE_ROTATE) ? m->relation_trig : nullptr;
  f.fast_u = (rp != RP_MFMA) ? 0.f : (float)(98.8 + 1.02 * xsplit_nslab(m->entity_dim));  // (as rank_bind)
  a.eg = fgeo.eg; a.fixed_rows = sh->fixed_rows; a.s_true_in = sh->s_true;
  a.own_lo = sh->own_begin; a.E_glob = m->nentity;
  a.q_w = w.q; a.s_true_w = w.s_true; a.state_w = w.state; a.gt_w = w.gt; a.ucnt_w = w.ucnt; a.bits_w = w.bits;
  a.counts = sh->counts; a.listed = listed_out;
  auto stage = [&](int k) { return launch_status(ops.rank_shard_fast(md, fgeo.vec, fgeo.ns, k, a, s)); };
  // 1. the states, the fast q, zeroed counters
  st = stage(0);
  if (st) return st;
  if (rows > 0) {  // (an empty shard: bad queries flagged above, zero counts below)
    // 2. the shard's excluded rows (an id outside the table is no error here, as in the exact stage)
    st = launch_status(launch_filter_bits_range(queries, mode == KGE_HEAD_BATCH ? 1 : 0,
                                                (sh->flags & KGE_RANK_FILTER_TABLE) ? 1 : 0, sh->filt_off,
                                                sh->filt_ids, nq, m->nentity, m->nrelation, sh->own_begin,
                                                sh->own_end, w.bits, nullptr, s));
    if (st) return st;
    // 3. the shard's statistics (and split operands), recomputed every call
    if (rp == RP_MFMA) {
      st = launch_status(launch_split_stats(v.entity_embedding, rows, m->entity_dim, w.es, w.stats, s, nullptr, nullptr));
      if (!st) st = launch_status(launch_split_bf16(w.q, nq, m->entity_dim, w.qs, s));
    } else if (m->model == KGE_DISTMULT || m->model == KGE_COMPLEX) {
      st = launch_status(launch_table_stats(v.entity_embedding, rows, m->entity_dim, w.stats, s));
    }
    if (st) return st;
    // 4. the true row's bit, the windows and the reference-order q
    st = stage(1);
    if (st) return st;
    // 5. counting on the view: clear cases counted, near-ties listed
    const RankWin win{w.delta, w.ucnt, w.ulist, RANK_CAP};
    if (rp == RP_MFMA) {
      st = launch_status(launch_rank_mfma_x(0, w.qs, w.es, nq, rows, m->entity_dim, w.state, w.s_true, w.bits, w.gt,
                                            win, s));
    } else {
      TileArgs ta;
      memset(&ta, 0, sizeof(ta));
      ta.q = w.q; ta.ent = v.entity_embedding; ta.modulus = m->modulus;
      ta.nq = nq; ta.E = rows; ta.Le = m->entity_dim; ta.K = K;
      ta.c = f.c; ta.true_id = w.state; ta.s_true = w.s_true;
      ta.fbits = w.bits; ta.W = W; ta.gt = w.gt; ta.win = win;
      st = launch_status(ops.rank_tile(md, 0, ta, s));
    }
    if (st) return st;
  }
  // 6, 7. the listed candidates (an overflowed list: the own rows) in reference order; the counts
  return stage(2);
}

}  // namespace
}  // namespace kge

using namespace kge;

extern "C" {

const char* kge_version(void) { return "knowledgegraphembedding_amd " KGE_ABI_VERSION " gfx950"; }

const char* kge_status_string(int status) {
  switch (status) {
    case KGE_OK: return "ok";
    case KGE_ERR_MODEL: return "model not supported";
    case KGE_ERR_MODE: return "mode not supported";
    case KGE_ERR_SHAPE: return "entity/relation dims inconsistent with the model";
    case KGE_ERR_ARG: return "invalid argument";
    case KGE_ERR_WORKSPACE: return "workspace too small";
    case KGE_ERR_DIM: return "size outside the kernels' range (negatives per row, queries per call, LDS; wide rows under query shipping)";
    case KGE_ERR_ABI: return "kge_model_desc.struct_size does not match this library (built against another kge_hip.h)";
    default:
      if (status >= KGE_ERR_HIP_BASE) return hipGetErrorString((hipError_t)(status - KGE_ERR_HIP_BASE));
      return "unknown";
  }
}

int kge_score(const kge_model_desc* m, int32_t mode, const int64_t* pos, const int64_t* neg, int64_t batch,
              int64_t nneg, float* out, int32_t* err_flag, void* stream) {
  Geom geo;
  int st = check_model(m, &geo);
  if (st) return st;
  if (mode != KGE_SINGLE && mode != KGE_HEAD_BATCH && mode != KGE_TAIL_BATCH) return KGE_ERR_MODE;
  if (batch == 0 && nneg >= 1) return KGE_OK;  // empty batch: nothing to score (buffers may be empty/NULL)
  if (!pos || !out || !err_flag || batch < 0 || nneg < 1) return KGE_ERR_ARG;
  Negatives cand;
  st = negatives_of(mode, pos, neg, nneg, &cand);
  if (st) return st;
  ScoreArgs a;
  a.ent = m->entity_embedding; a.rel = m->relation_embedding; a.modulus = m->modulus;
  a.pos = pos; a.neg = cand.ids; a.neg_stride = cand.stride;
  a.B = batch; a.n = nneg; a.E = m->nentity; a.R = m->nrelation;
  a.Le = m->entity_dim; a.Lr = m->relation_dim; a.eg = geo.eg; a.c = consts_of(m);
  a.jpw = nneg < 16 ? nneg : 16;
  a.out = out; a.err = err_flag;
  const int64_t units = batch * ((nneg + a.jpw - 1) / a.jpw);
  return launch_status(ops_for(m->model).score(kernel_mode(mode), geo.vec, geo.ns, a, units, as_stream(stream)));
}

size_t kge_backward_workspace_bytes(const kge_model_desc* m, int32_t mode, int64_t batch, int64_t nneg) {
  (void)mode;
  size_t b = 0;
  carve_grad(nullptr, m, batch, nneg, &b);
  return b;
}

int kge_score_backward(const kge_model_desc* m, int32_t mode, const int64_t* pos, const int64_t* neg, int64_t batch,
                       int64_t nneg, const float* grad_scores, float* grad_entity, float* grad_relation,
                       float* grad_modulus, void* workspace, size_t workspace_bytes, int32_t* err_flag,
                       void* stream) {
  Geom geo;
  int st = check_model(m, &geo);
  if (st) return st;
  if (mode != KGE_SINGLE && mode != KGE_HEAD_BATCH && mode != KGE_TAIL_BATCH) return KGE_ERR_MODE;
  if (!pos || !grad_scores || !grad_entity || !grad_relation || !err_flag || batch < 1 || nneg < 1)
    return KGE_ERR_ARG;
  if (!grad_streams_aligned(geo, grad_entity, grad_relation, nullptr)) return KGE_ERR_ARG;
  Negatives cand;
  st = negatives_of(mode, pos, neg, nneg, &cand);
  if (st) return st;
  size_t need = 0;
  const GradWs w = carve_grad(workspace, m, batch, nneg, &need);
  if (!workspace || workspace_bytes < need) return KGE_ERR_WORKSPACE;
  StepCall c;  // the whole step, no loss terms, no optimizer
  c.in = {m, mode, pos, neg, batch, nneg};
  c.ws = {workspace, workspace_bytes, err_flag, stream};
  c.out = {grad_entity, grad_relation, grad_modulus};
  const Batch b = batch_of(c, geo, cand, w);
  RowArgs ra = row_args(b);
  ra.op = ROW_GIVEN;
  ra.g_in = grad_scores;
  ra.n_lds = 0;
  FinArgs fa;
  memset(&fa, 0, sizeof(fa));
  fa.B = batch;
  fa.uni_weight = 1;
  fa.uni_n = 1.f;
  return run_grad(c, b, ra, fa);
}

size_t kge_train_workspace_bytes(const kge_model_desc* m, int64_t batch, int64_t nneg) {
  size_t b = 0;
  carve_grad(nullptr, m, batch, nneg, &b);
  return b;
}

int kge_train_step(const kge_model_desc* m, int32_t mode, const int64_t* pos, const int64_t* neg, int64_t batch,
                   int64_t nneg, const float* subsampling_weight, const float* weight_sum, int32_t uni_weight,
                   int64_t uni_batch, int32_t adversarial, float adversarial_temperature, float regularization,
                   const kge_adam_desc* adam, float* grad_entity, float* grad_relation, float* grad_modulus,
                   float* losses_out, void* workspace, size_t workspace_bytes, int32_t* err_flag, void* stream) {
  if (!adam) return KGE_ERR_ARG;
  StepCall c;
  c.in = {m, mode, pos, neg, batch, nneg};
  c.ws = {workspace, workspace_bytes, err_flag, stream};
  c.loss = {subsampling_weight, weight_sum, uni_weight, uni_batch, adversarial, adversarial_temperature, regularization};
  c.adam = adam;
  c.out = {grad_entity, grad_relation, grad_modulus, losses_out};
  return train_impl(c);
}

size_t kge_train_lazy_workspace_bytes(const kge_model_desc* m, int64_t batch, int64_t nneg) {
  size_t b = 0;
  carve_grad(nullptr, m, batch, nneg, &b);
  carve_lazy(nullptr, m, batch, nneg, b, &b);
  return b;
}

int kge_train_step_lazy(const kge_model_desc* m, int32_t mode, const int64_t* pos, const int64_t* neg, int64_t batch,
                        int64_t nneg, const float* subsampling_weight, const float* weight_sum, int32_t uni_weight,
                        int64_t uni_batch, int32_t adversarial, float adversarial_temperature, float regularization,
                        const kge_adam_desc* adam, float* grad_entity, float* grad_relation, float* grad_modulus,
                        float* losses_out, void* workspace, size_t workspace_bytes, int32_t* err_flag, void* stream) {
  if (!adam) return KGE_ERR_ARG;
  StepCall c;
  c.in = {m, mode, pos, neg, batch, nneg};
  c.ws = {workspace, workspace_bytes, err_flag, stream};
  c.loss = {subsampling_weight, weight_sum, uni_weight, uni_batch, adversarial, adversarial_temperature, regularization};
  c.adam = adam;
  c.out = {grad_entity, grad_relation, grad_modulus, losses_out};
  c.lazy = true;
  return train_impl(c);
}

size_t kge_train_adagrad_workspace_bytes(const kge_model_desc* m, int64_t batch, int64_t nneg) {
  return kge_train_lazy_workspace_bytes(m, batch, nneg);
}

int kge_train_step_adagrad(const kge_model_desc* m, int32_t mode, const int64_t* pos, const int64_t* neg,
                           int64_t batch, int64_t nneg, const float* subsampling_weight, const float* weight_sum,
                           int32_t uni_weight, int64_t uni_batch, int32_t adversarial, float adversarial_temperature,
                           float regularization, const kge_adagrad_desc* opt, float* grad_entity,
                           float* grad_relation, float* grad_modulus, float* losses_out, void* workspace,
                           size_t workspace_bytes, int32_t* err_flag, void* stream) {
  if (!opt) return KGE_ERR_ARG;
  StepCall c;
  c.in = {m, mode, pos, neg, batch, nneg};
  c.ws = {workspace, workspace_bytes, err_flag, stream};
  c.loss = {subsampling_weight, weight_sum, uni_weight, uni_batch, adversarial, adversarial_temperature, regularization};
  c.adagrad = opt;
  c.out = {grad_entity, grad_relation, grad_modulus, losses_out};
  c.lazy = true;
  return train_impl(c);
}

int kge_train_step_grads(const kge_model_desc* m, int32_t mode, const int64_t* pos, const int64_t* neg,
                         int64_t batch, int64_t nneg, const float* subsampling_weight, const float* weight_sum,
                         int32_t uni_weight, int64_t uni_batch, int32_t adversarial,
                         float adversarial_temperature, float regularization, float* grad_entity,
                         float* grad_relation, float* grad_modulus, float* losses_out, void* workspace,
                         size_t workspace_bytes, int32_t* err_flag, void* stream) {
  StepCall c;
  c.in = {m, mode, pos, neg, batch, nneg};
  c.ws = {workspace, workspace_bytes, err_flag, stream};
  c.loss = {subsampling_weight, weight_sum, uni_weight, uni_batch, adversarial, adversarial_temperature, regularization};
  c.out = {grad_entity, grad_relation, grad_modulus, losses_out};
  return train_impl(c);
}

int kge_train_step_grads_phased(const kge_model_desc* m, int32_t mode, const int64_t* pos, const int64_t* neg,
                                int64_t batch, int64_t nneg, const float* subsampling_weight,
                                const float* weight_sum, int32_t uni_weight, int64_t uni_batch, int32_t adversarial,
                                float adversarial_temperature, float regularization, float* grad_entity,
                                float* grad_relation, float* grad_modulus, float* losses_out, void* workspace,
                                size_t workspace_bytes, int32_t* err_flag, void* stream, int32_t phases,
                                int64_t entity_begin, int64_t entity_end) {
  StepCall c;
  c.in = {m, mode, pos, neg, batch, nneg};
  c.ws = {workspace, workspace_bytes, err_flag, stream};
  c.loss = {subsampling_weight, weight_sum, uni_weight, uni_batch, adversarial, adversarial_temperature, regularization};
  c.out = {grad_entity, grad_relation, grad_modulus, losses_out};
  c.phases = phases;
  c.e_begin = entity_begin;
  c.e_end = entity_end;
  return train_impl(c);
}

int kge_train_rows_slice(const kge_model_desc* m, int32_t mode, const int64_t* pos, const int64_t* neg,
                         int64_t nrows, int64_t nneg, const float* subsampling_weight, const float* weight_sum,
                         int32_t uni_weight, int64_t uni_batch, int32_t adversarial, float adversarial_temperature,
                         float* g_out, float* dq_out, float* stats_out, void* workspace, size_t workspace_bytes,
                         int32_t* err_flag, void* stream) {
  StepCall c;
  c.in = {m, mode, pos, neg, nrows, nneg};
  c.ws = {workspace, workspace_bytes, err_flag, stream};
  c.loss = {subsampling_weight, weight_sum, uni_weight, uni_batch, adversarial, adversarial_temperature};
  c.phases = KGE_PHASE_ROWS;
  c.xstage = XS_ROWS_ONLY;
  c.rows = {g_out, dq_out, stats_out};
  return train_impl(c);
}

int kge_train_csr(const kge_model_desc* m, int32_t mode, const int64_t* pos, const int64_t* neg, int64_t batch,
                  int64_t nneg, void* workspace, size_t workspace_bytes, int32_t* err_flag, void* stream) {
  StepCall c;
  c.in = {m, mode, pos, neg, batch, nneg};
  c.ws = {workspace, workspace_bytes, err_flag, stream};
  c.xstage = XS_CSR_ONLY;
  return train_impl(c);
}

int kge_train_csr_range(const kge_model_desc* m, int32_t mode, const int64_t* pos, const int64_t* neg,
                        int64_t batch, int64_t nneg, int64_t entity_begin, int64_t entity_end, void* workspace,
                        size_t workspace_bytes, int32_t* err_flag, void* stream) {
  if (!m || !entity_range_ok(m, entity_begin, entity_end)) return KGE_ERR_ARG;
  StepCall c;
  c.in = {m, mode, pos, neg, batch, nneg};
  c.ws = {workspace, workspace_bytes, err_flag, stream};
  c.xstage = XS_CSR_ONLY;
  c.csr_lo = entity_begin;
  c.csr_hi = entity_end;
  return train_impl(c);
}

// The four kge_train_step_from_rows* entries: the step after the exchange, on
// the gathered per-row factors (the row pass ran on the ranks).
int kge_train_step_from_rows_phased(const kge_model_desc* m, int32_t mode, const int64_t* pos, const int64_t* neg,
                                    int64_t batch, int64_t nneg, const float* subsampling_weight,
                                    const float* weight_sum, int32_t uni_weight, int64_t uni_batch,
                                    float regularization, const float* g_in, const float* dq_in, float* stats_inout,
                                    const kge_adam_desc* adam, float* grad_entity, float* grad_relation,
                                    float* grad_modulus, float* losses_out, void* workspace, size_t workspace_bytes,
                                    int32_t* err_flag, void* stream, int32_t phases, int64_t entity_begin,
                                    int64_t entity_end, int32_t csr_ready, int32_t reg_relations) {
  if (phases <= 0 || phases > KGE_PHASE_ALL) return KGE_ERR_ARG;
  if (!entity_range_ok(m, entity_begin, entity_end)) return KGE_ERR_ARG;
  StepCall c;
  c.in = {m, mode, pos, neg, batch, nneg};
  c.ws = {workspace, workspace_bytes, err_flag, stream};
  c.loss = {subsampling_weight, weight_sum, uni_weight, uni_batch};
  c.loss.regularization = regularization;
  c.adam = adam;
  c.out = {grad_entity, grad_relation, grad_modulus, losses_out};
  c.phases = phases;
  c.e_begin = entity_begin;
  c.e_end = entity_end;
  c.xstage = csr_ready ? XS_FROM_ROWS_CSR : XS_FROM_ROWS;
  c.rows = {const_cast<float*>(g_in), const_cast<float*>(dq_in), stats_inout};
  c.reg_relations = reg_relations ? 1 : 0;
  return train_impl(c);
}

int kge_train_step_from_rows_range(const kge_model_desc* m, int32_t mode, const int64_t* pos, const int64_t* neg,
                                   int64_t batch, int64_t nneg, const float* subsampling_weight,
                                   const float* weight_sum, int32_t uni_weight, int64_t uni_batch,
                                   float regularization, const float* g_in, const float* dq_in, float* stats_inout,
                                   const kge_adam_desc* adam, float* grad_entity, float* grad_relation,
                                   float* grad_modulus, float* losses_out, void* workspace, size_t workspace_bytes,
                                   int32_t* err_flag, void* stream, int64_t entity_begin, int64_t entity_end,
                                   int32_t csr_ready, int32_t reg_relations) {
  if (!entity_range_ok(m, entity_begin, entity_end)) return KGE_ERR_ARG;
  StepCall c;
  c.in = {m, mode, pos, neg, batch, nneg};
  c.ws = {workspace, workspace_bytes, err_flag, stream};
  c.loss = {subsampling_weight, weight_sum, uni_weight, uni_batch};
  c.loss.regularization = regularization;
  c.adam = adam;
  c.out = {grad_entity, grad_relation, grad_modulus, losses_out};
  c.e_begin = entity_begin;
  c.e_end = entity_end;
  c.xstage = csr_ready ? XS_FROM_ROWS_CSR : XS_FROM_ROWS;
  c.rows = {const_cast<float*>(g_in), const_cast<float*>(dq_in), stats_inout};
  c.reg_relations = reg_relations ? 1 : 0;
  return train_impl(c);
}

int kge_train_step_from_rows(const kge_model_desc* m, int32_t mode, const int64_t* pos, const int64_t* neg,
                             int64_t batch, int64_t nneg, const float* subsampling_weight, const float* weight_sum,
                             int32_t uni_weight, int64_t uni_batch, float regularization, const float* g_in,
                             const float* dq_in, float* stats_inout, const kge_adam_desc* adam, float* grad_entity,
                             float* grad_relation, float* grad_modulus, float* losses_out, void* workspace,
                             size_t workspace_bytes, int32_t* err_flag, void* stream) {
  StepCall c;
  c.in = {m, mode, pos, neg, batch, nneg};
  c.ws = {workspace, workspace_bytes, err_flag, stream};
  c.loss = {subsampling_weight, weight_sum, uni_weight, uni_batch};
  c.loss.regularization = regularization;
  c.adam = adam;
  c.out = {grad_entity, grad_relation, grad_modulus, losses_out};
  c.xstage = XS_FROM_ROWS;
  c.rows = {const_cast<float*>(g_in), const_cast<float*>(dq_in), stats_inout};
  return train_impl(c);
}

int kge_train_step_from_rows_csr(const kge_model_desc* m, int32_t mode, const int64_t* pos, const int64_t* neg,
                                 int64_t batch, int64_t nneg, const float* subsampling_weight, const float* weight_sum,
                                 int32_t uni_weight, int64_t uni_batch, float regularization, const float* g_in,
                                 const float* dq_in, float* stats_inout, const kge_adam_desc* adam, float* grad_entity,
                                 float* grad_relation, float* grad_modulus, float* losses_out, void* workspace,
                                 size_t workspace_bytes, int32_t* err_flag, void* stream) {
  StepCall c;
  c.in = {m, mode, pos, neg, batch, nneg};
  c.ws = {workspace, workspace_bytes, err_flag, stream};
  c.loss = {subsampling_weight, weight_sum, uni_weight, uni_batch};
  c.loss.regularization = regularization;
  c.adam = adam;
  c.out = {grad_entity, grad_relation, grad_modulus, losses_out};
  c.xstage = XS_FROM_ROWS_CSR;
  c.rows = {const_cast<float*>(g_in), const_cast<float*>(dq_in), stats_inout};
  return train_impl(c);
}

int kge_ship_step(const kge_model_desc* m, int32_t mode, const kge_ship_desc* sh, int32_t stage,
                  const kge_adam_desc* adam, float* grad_entity, float* grad_relation, float* grad_modulus,
                  float* losses_out, void* workspace, size_t workspace_bytes, int32_t* err_flag, void* stream) {
  Geom geo;
  int st = check_model(m, &geo);
  if (st) return st;
  if (mode != KGE_HEAD_BATCH && mode != KGE_TAIL_BATCH) return KGE_ERR_MODE;
  if (!sh || stage < KGE_SHIP_Q || stage > KGE_SHIP_ENTITY || !err_flag) return KGE_ERR_ARG;
  const int64_t B = sh->batch, n = sh->nneg;
  if (!sh->pos || !sh->neg || B < 1 || n < 1 || n > 8192) return KGE_ERR_ARG;
  if (sh->world < 1 || sh->world > 4096 || sh->rank < 0 || sh->rank >= sh->world) return KGE_ERR_ARG;
  if (sh->own_begin < 0 || sh->own_end < sh->own_begin || sh->own_end > m->nentity) return KGE_ERR_ARG;
  if (!sh->uni_weight && (!sh->subsampling_weight || !sh->weight_sum)) return KGE_ERR_ARG;
  const bool head = (mode == KGE_HEAD_BATCH);
  if (!sh->q || !sh->part || !sh->parts || !sh->scores || !sh->g || !sh->dq || !sh->pstats || !sh->ent_contrib ||
      !sh->rel_contrib || !sh->row_stats || (head && (!sh->qp || !sh->pq)))
    return KGE_ERR_ARG;
  if (stage >= KGE_SHIP_CHAIN && !grad_relation) return KGE_ERR_ARG;
  if (stage == KGE_SHIP_ENTITY && (!grad_entity || !losses_out || (m->model == KGE_PROTATE && !grad_modulus)))
    return KGE_ERR_ARG;
  if (adam && (!adam->entity.param || !adam->entity.exp_avg || !adam->entity.exp_avg_sq ||
               adam->entity.param != m->entity_embedding))
    return KGE_ERR_ARG;
  if (!grad_streams_aligned(geo, grad_entity, grad_relation, adam)) return KGE_ERR_ARG;
  size_t need = 0;
  GradWs w = carve_grad(workspace, m, B, n, &need);
  if (!workspace || workspace_bytes < need) return KGE_ERR_WORKSPACE;
  // the shipped per-row buffers are the caller's (they cross the ranks between the stages)
  w.q = sh->q; w.dq = sh->dq; w.g = sh->g;
  w.ent_contrib = sh->ent_contrib; w.rel_contrib = sh->rel_contrib; w.row_stats = sh->row_stats;
  hipStream_t s = as_stream(stream);
  const ModelOps& op = ops_for(m->model);
  const int kmode = kernel_mode(mode);
  const Batch b = {m, geo, kmode, sh->pos, {sh->neg, n}, B, n, w, err_flag, s};
  StepCall::Loss loss;
  loss.subsampling_weight = sh->subsampling_weight;
  loss.weight_sum = sh->weight_sum;
  loss.uni_weight = sh->uni_weight;
  loss.uni_batch = sh->uni_batch;

  RowArgs ra = row_args(b);
  ra.op = ROW_TRAIN;
  ra.adversarial = sh->adversarial ? 1 : 0;
  ra.adv_T = sh->adversarial_temperature;
  ra.uni_weight = sh->uni_weight ? 1 : 0;
  ra.uni_inv = 1.f / (float)(sh->uni_batch > 0 ? sh->uni_batch : B);
  ra.sub_w = sh->subsampling_weight;
  ra.w_sum = sh->weight_sum;
  ra.n_lds = 0; ra.fuse_epi = 0;
  ra.sh.own_lo = sh->own_begin; ra.sh.own_hi = sh->own_end;
  ra.sh.world = sh->world; ra.sh.me = sh->rank;
  ra.sh.q_in = sh->q; ra.sh.qp_in = sh->qp; ra.sh.qp_out = sh->qp;
  ra.sh.part_out = sh->part; ra.sh.parts_in = sh->parts; ra.sh.s_out = sh->scores;
  ra.sh.pq = sh->pq; ra.sh.pstats = sh->pstats;
  Side* sd = side_for_device();
  // this shard's entity rows; the relation table is replicated: its regulariser once, on rank 0
  const EntRange own = {sh->own_begin, sh->own_end, entity_slices(geo, B, m->entity_dim), sh->rank == 0};
  const float reg = sh->regularization;

  switch (stage) {
    case KGE_SHIP_Q:
      return launch_status(op.row(kmode, geo.vec, geo.ns, RowStage::ShipQ, ra, 0, s));
    case KGE_SHIP_ROWS: {
      // the occurrence CSR of the global batch beside the row pass (it needs only the ids);
      // only this shard's rows are visited by its entity pass
      const CsrArgs ca = csr_args(b, sh->own_begin, sh->own_end);
      hipStream_t ss = sd ? sd->s : s;
      if (sd && ((st = edge_record(sd->fork, s)) || (st = edge_wait(ss, sd->fork)))) return st;
      st = launch_status(launch_csr(ca, ss));
      if (st) return st;
      if (sd && (st = edge_record(sd->csr_done, ss))) return st;
      const size_t lds = row_lds(geo, m->entity_dim, ra, false);  // (wide rows: refused by the launch)
      if (lds > LDS_MAX) return KGE_ERR_DIM;
      return launch_status(op.row(kmode, geo.vec, geo.ns, RowStage::ShipRows, ra, lds, s));
    }
    case KGE_SHIP_MERGE:
      return launch_status(op.row(kmode, geo.vec, geo.ns, RowStage::ShipMerge, ra, 0, s));
    case KGE_SHIP_CHAIN:
      st = launch_status(op.row(kmode, geo.vec, geo.ns, RowStage::ShipChain, ra, 0, s));
      if (st) return st;
      if (sd && (st = edge_wait(s, sd->csr_done))) return st;  // the relation pass reads the CSR
      return launch_status(launch_rel_rows(
          rel_args(b, own.reg_relations ? 3.f * reg : 0.f, m->nentity * own.per(), grad_relation, OPT_GRAD_ONLY), s));
    case KGE_SHIP_ENTITY:
      if (own.e_end > own.e_begin) {
        const EntArgs ea = ent_args(b, own, sh->g, reg, grad_entity, opt_for(adam, adam ? &adam->entity : nullptr));
        st = launch_status(op.entity(kmode, geo.vec, geo.ns, ea, OPT_ADAM, s));
        if (st) return st;
      }
      return launch_status(launch_finalize(
          fin_args(fin_loss(loss, B, losses_out, err_flag), b, own, reg, grad_modulus, adam), s));
  }
  return KGE_ERR_ARG;  // (stage was checked above)
}

int kge_weight_sum(const float* w, int64_t n, float* out, void* stream) {
  if (!w || !out || n < 0) return KGE_ERR_ARG;
  return launch_status(launch_weight_sum(w, n, out, as_stream(stream)));
}

int kge_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t numel, float beta1,
                  float beta2, float eps, float step_size, float bias_correction2_sqrt, void* stream) {
  if (!param || !grad || !exp_avg || !exp_avg_sq || numel < 0) return KGE_ERR_ARG;
  if (numel == 0) return KGE_OK;
  if (!aligned16(param) || !aligned16(grad) || !aligned16(exp_avg) || !aligned16(exp_avg_sq)) return KGE_ERR_ARG;
  return launch_status(launch_adam(param, grad, exp_avg, exp_avg_sq, numel, beta1, beta2, eps, step_size,
                                   bias_correction2_sqrt, as_stream(stream)));
}

int kge_adagrad_step(float* param, const float* grad, float* state_sum, int64_t numel, float lr, float eps,
                     void* stream) {
  if (!param || !grad || !state_sum || numel < 0) return KGE_ERR_ARG;
  if (!(eps > 0.f) || !(lr >= 0.f) || isinf(lr)) return KGE_ERR_ARG;
  if (numel == 0) return KGE_OK;
  if (!aligned16(param) || !aligned16(grad) || !aligned16(state_sum)) return KGE_ERR_ARG;
  return launch_status(launch_adagrad(param, grad, state_sum, numel, lr, eps, as_stream(stream)));
}

size_t kge_rank_workspace_bytes(const kge_model_desc* m, int64_t nq) {
  size_t b = 0;
  carve_rank(nullptr, m, nq, &b);
  return b;
}

int kge_rank_filtered_ex(const kge_model_desc* m, int32_t mode, const int64_t* queries, int64_t nq,
                         const int64_t* filt_off, const int64_t* filt_ids, int64_t* ranks_out, int32_t* ties_out,
                         int32_t* listed_out, int32_t path, void* workspace, size_t workspace_bytes,
                         int32_t* err_flag, void* stream) {
  RankCall c = {m, nq, workspace, workspace_bytes, err_flag, stream};
  c.stage = (path & KGE_RANK_STAGE_LIST) ? RS_LIST : RS_ALL;
  c.mode = mode;
  c.path = path;
  c.queries = queries;
  c.filt_off = filt_off;
  c.filt_ids = filt_ids;
  c.ranks_out = ranks_out;
  c.ties_out = ties_out;
  c.listed_out = listed_out;
  return rank_impl(c);
}

int kge_rank_filtered(const kge_model_desc* m, int32_t mode, const int64_t* queries, int64_t nq,
                      const int64_t* filt_off, const int64_t* filt_ids, int64_t* ranks_out, int32_t* ties_out,
                      void* workspace, size_t workspace_bytes, int32_t* err_flag, void* stream) {
  return kge_rank_filtered_ex(m, mode, queries, nq, filt_off, filt_ids, ranks_out, ties_out, nullptr, RP_AUTO,
                              workspace, workspace_bytes, err_flag, stream);
}

int kge_rank_filtered_both(const kge_model_desc* m, const int64_t* queries, int64_t nq,
                           const int64_t* filt_off_head, const int64_t* filt_ids_head, const int64_t* filt_off_tail,
                           const int64_t* filt_ids_tail, int64_t* ranks_out, int32_t* ties_out, int32_t* listed_out,
                           int32_t path, void* workspace, size_t workspace_bytes, int32_t* err_flag, void* stream) {
  if (path & KGE_RANK_STAGE_LIST) return KGE_ERR_ARG;  // pRotatE's three-call form is per direction
  RankCall c = {m, nq, workspace, workspace_bytes, err_flag, stream};
  c.both = true;
  c.path = path;
  c.queries = queries;
  c.filt_off = filt_off_head;
  c.filt_ids = filt_ids_head;
  c.filt_off_tail = filt_off_tail;
  c.filt_ids_tail = filt_ids_tail;
  c.ranks_out = ranks_out;
  c.ties_out = ties_out;
  c.listed_out = listed_out;
  return rank_impl(c);
}

size_t kge_topk_workspace_bytes(const kge_model_desc* m, int64_t nq, int32_t k, int32_t parts) {
  Geom geo;
  if (check_model(m, &geo) || nq < 0 || k < 1 || k > KGE_TOPK_MAX_K || parts < 0) return 0;
  int64_t span = 0;
  size_t b = 0;
  carve_topk(nullptr, m, nq, k, topk_parts(m, nq, parts, &span), true, &b);
  return b;
}

int kge_topk(const kge_model_desc* m, int32_t mode, const int64_t* queries, int64_t nq, const int64_t* filt_off,
             const int64_t* filt_ids, int32_t k, int64_t* ids_out, float* scores_out, int32_t path, int32_t parts,
             void* workspace, size_t workspace_bytes, int32_t* err_flag, void* stream) {
  return topk_impl(m, mode, queries, nq, filt_off, filt_ids, k, ids_out, scores_out, path, parts, workspace,
                   workspace_bytes, err_flag, stream);
}

size_t kge_rank_candidates_workspace_bytes(const kge_model_desc* m, int64_t nq, int64_t ncand) {
  Geom geo;
  if (check_model(m, &geo) || nq < 0 || ncand < 1) return 0;
  size_t b = 0;
  carve_cand(nullptr, m, nq, &b);
  return b;
}

int kge_rank_candidates(const kge_model_desc* m, int32_t mode, const int64_t* queries, int64_t nq,
                        const int64_t* cand, int64_t ncand, int64_t* ranks_out, int32_t* ties_out, void* workspace,
                        size_t workspace_bytes, int32_t* err_flag, void* stream) {
  return rank_cand_impl(m, mode, queries, nq, cand, ncand, ranks_out, ties_out, workspace, workspace_bytes, err_flag,
                        stream);
}

size_t kge_rank_relations_workspace_bytes(const kge_model_desc* m, int64_t nq) {
  Geom geo;
  if (check_model(m, &geo) || nq < 0) return 0;
  size_t b = 0;
  carve_rel(nullptr, m, nq, &b);
  return b;
}

int kge_rank_relations(const kge_model_desc* m, const int64_t* queries, int64_t nq, const int64_t* filt_off,
                       const int64_t* filt_ids, int64_t* ranks_out, int32_t* ties_out, float* scores_out,
                       void* workspace, size_t workspace_bytes, int32_t* err_flag, void* stream) {
  return rank_rel_impl(m, queries, nq, filt_off, filt_ids, ranks_out, ties_out, scores_out, workspace, workspace_bytes,
                       err_flag, stream);
}

size_t kge_rank_shard_workspace_bytes(const kge_model_desc* m, int64_t nq) {
  Geom geo;
  if (check_model(m, &geo) || nq < 0) return 0;
  size_t b = 0;
  carve_shard(nullptr, m, nq, &b);
  return b;
}

int kge_rank_shard(const kge_model_desc* m, int32_t mode, const kge_rank_shard_desc* sh, int32_t stage,
                   const int64_t* queries, int64_t nq, void* workspace, size_t workspace_bytes, int32_t* err_flag,
                   void* stream) {
  return rank_shard_impl(m, mode, sh, stage, queries, nq, workspace, workspace_bytes, err_flag, stream);
}

size_t kge_rank_candidates_shard_workspace_bytes(const kge_model_desc* m, int64_t nq, int64_t ncand) {
  Geom geo;
  if (check_model(m, &geo) || nq < 0 || ncand < 1) return 0;
  size_t b = 0;
  carve_cand_shard(nullptr, m, nq, &b);
  return b;
}

int kge_rank_candidates_shard(const kge_model_desc* m, int32_t mode, const kge_rank_cand_shard_desc* sh,
                              const int64_t* queries, int64_t nq, const int64_t* cand, int64_t ncand, void* workspace,
                              size_t workspace_bytes, int32_t* err_flag, void* stream) {
  return rank_cand_shard_impl(m, mode, sh, queries, nq, cand, ncand, workspace, workspace_bytes, err_flag, stream);
}

// 1, 2 or 3; refused: minus the status the call returns for it
int kge_rank_shard_fast_path(const kge_model_desc* m, const kge_rank_shard_desc* sh) {
  Geom geo;
  int path = 0;
  // (the mode plays no part in the path)
  const int st = shard_fast_check(m, KGE_HEAD_BATCH, sh, &geo, &path);
  if (st) return -st;
  if (!sh->fixed_rows) return -KGE_ERR_ARG;
  const int rp = shard_fast_path(m, sh, path, nullptr);
  return rp < 0 ? -KGE_ERR_ARG : rp;
}

// 0: a bad model, descriptor, range, flags, path or nq (the call itself says which)
size_t kge_rank_shard_fast_workspace_bytes(const kge_model_desc* m, const kge_rank_shard_desc* sh, int64_t nq) {
  const int rp = kge_rank_shard_fast_path(m, sh);
  if (rp < 0 || nq < 0) return 0;
  size_t b = 0;
  if (rp == RP_SCAN) carve_shard(nullptr, m, nq, &b);
  else carve_shard_fast(nullptr, m, sh->own_end - sh->own_begin, nq, rp, &b);
  return b;
}

int kge_rank_shard_fast(const kge_model_desc* m, int32_t mode, const kge_rank_shard_desc* sh, const int64_t* queries,
                        int64_t nq, int32_t* listed_out, void* workspace, size_t workspace_bytes, int32_t* err_flag,
                        void* stream) {
  return rank_shard_fast_impl(m, mode, sh, queries, nq, listed_out, workspace, workspace_bytes, err_flag, stream);
}

// 0: a bad model, descriptor, stage, range, k or nq (the call itself says which)
size_t kge_topk_shard_workspace_bytes(const kge_model_desc* m, const kge_topk_shard_desc* sh, int32_t stage,
                                      int64_t nq) {
  Geom geo;
  if (check_model(m, &geo) || nq < 0) return 0;
  if (!sh || sh->struct_size != (int32_t)sizeof(kge_topk_shard_desc)) return 0;
  if (stage == KGE_TSHARD_MERGE) return 256;
  if (stage != KGE_TSHARD_LIST) return 0;
  if (sh->own_begin < 0 || sh->own_end < sh->own_begin || sh->own_end > m->nentity) return 0;
  if (sh->k < 1 || sh->k > KGE_TOPK_MAX_K || sh->parts < 0) return 0;
  const int64_t rows = sh->own_end - sh->own_begin;
  const kge_model_desc v = shard_view(m, sh->own_begin, sh->own_end);
  int64_t span = 0;
  size_t b = 0;
  carve_topk(nullptr, &v, nq, sh->k, topk_shard_parts(&v, rows, nq, sh->parts, &span), false, &b);
  return b;
}

int kge_topk_shard(const kge_model_desc* m, int32_t mode, const kge_topk_shard_desc* sh, int32_t stage,
                   const int64_t* queries, int64_t nq, void* workspace, size_t workspace_bytes, int32_t* err_flag,
                   void* stream) {
  return topk_shard_impl(m, mode, sh, stage, queries, nq, workspace, workspace_bytes, err_flag, stream);
}

int kge_rank_sin_args(const kge_model_desc* m, int32_t mode, int64_t nq, const int64_t* item_off, float* args_out,
                      void* workspace, size_t workspace_bytes, int32_t* err_flag, void* stream) {
  RankCall c = {m, nq, workspace, workspace_bytes, err_flag, stream};
  c.stage = RS_ARGS;
  c.mode = mode;
  c.item_off = item_off;
  c.args = args_out;
  return rank_impl(c);
}

int kge_rank_finish_sin(const kge_model_desc* m, int32_t mode, int64_t nq, const int64_t* item_off,
                        const float* sin_values, int64_t* ranks_out, int32_t* ties_out, int32_t* listed_out,
                        void* workspace, size_t workspace_bytes, int32_t* err_flag, void* stream) {
  RankCall c = {m, nq, workspace, workspace_bytes, err_flag, stream};
  c.stage = RS_FINISH;
  c.mode = mode;
  c.item_off = item_off;
  c.sins = sin_values;
  c.ranks_out = ranks_out;
  c.ties_out = ties_out;
  c.listed_out = listed_out;
  return rank_impl(c);
}

int kge_selftest_sin(float range, int32_t* max_dist_out, void* stream) {
  if (!max_dist_out) return KGE_ERR_ARG;
  return launch_status(launch_selftest_sin(range, max_dist_out, as_stream(stream)));
}

int kge_stage_timer(int32_t command, float* stage_ms_out, int32_t n_out) {
  if (command == 0 || command == 1) {
    g_timer.on = (command == 1);
    g_timer.pool.used = 0;
    g_timer.seen = 0;
    g_timer.period = (command == 1 && n_out > 0) ? n_out : 1;
    if (command == 0) {
      g_rank_timer.on = false;
      g_rank_timer.pool.used = 0;
    }
    return KGE_OK;
  }
  if (command == 4) {  // ranking calls: enable and reset
    g_rank_timer.on = true;
    g_rank_timer.pool.used = 0;
    return KGE_OK;
  }
  if (command == 5) {  // ranking calls: summed stage times + the number of directions ranked
    constexpr int NR = KGE_RANK_TIMER_STAGES + 1;
    if (!stage_ms_out || n_out < NR) return KGE_ERR_ARG;
    for (int k = 0; k < NR; ++k) stage_ms_out[k] = 0.f;
    const RankTimer& t = g_rank_timer;
    const std::vector<hipEvent_t>& ev = t.pool.ev;
    const size_t used = t.pool.used;
    size_t i = 0;
    int dirs = 0;
    while (i < used) {
      if (t.slot[i] != 0) {  // (marks before the first call start: none are recorded so)
        ++i;
        continue;
      }
      size_t j = i + 1;
      while (j < used && t.slot[j] != 0) ++j;
      // the call's marks [i, j): first and last event of each slot
      long first[NR], last[NR];
      for (int k = 0; k < NR; ++k) first[k] = last[k] = -1;
      for (size_t x = i; x < j; ++x) {
        const int sl = t.slot[x];
        if (sl < 0 || sl >= NR) continue;
        if (first[sl] < 0) first[sl] = (long)x;
        last[sl] = (long)x;
      }
      if (last[NR - 1] >= 0) {  // the call wrote its ranks
        hipError_t err = hipEventSynchronize(ev[last[NR - 1]]);
        if (err != hipSuccess) return hip_status(err);
        for (int k = 0; k < KGE_RANK_TIMER_STAGES; ++k) {
          if (first[k] < 0 || last[k + 1] < 0) continue;
          float ms = 0.f;
          err = hipEventElapsedTime(&ms, ev[first[k]], ev[last[k + 1]]);
          if (err != hipSuccess) return hip_status(err);
          stage_ms_out[k] += ms;
        }
        dirs += t.ndir[i];
      }
      i = j;
    }
    stage_ms_out[KGE_RANK_TIMER_STAGES] = (float)dirs;
    return KGE_OK;
  }
  // training calls, TM_COUNT marks each — 2: the stage times summed over the
  // timed calls, then their number; 3: per timed call, its stage times, then
  // its start relative to the first timed call's start (ms, device clock)
  if (command != 2 && command != 3) return KGE_ERR_ARG;
  const bool per_call = (command == 3);
  const hipEvent_t* ev = g_timer.pool.ev.data();
  const size_t calls = g_timer.pool.used / TM_COUNT;
  if (!stage_ms_out || (per_call ? (size_t)n_out < calls * TM_COUNT : n_out < TM_COUNT)) return KGE_ERR_ARG;
  for (size_t k = 0; k < (per_call ? calls : 1) * TM_COUNT; ++k) stage_ms_out[k] = 0.f;
  for (size_t c = 0; c < calls; ++c) {
    float* ms = stage_ms_out + (per_call ? c * TM_COUNT : 0);
    hipError_t err = add_stage_ms(ev + c * TM_COUNT, ms);
    if (err == hipSuccess && per_call) err = hipEventElapsedTime(&ms[KGE_TIMER_STAGES], ev[0], ev[c * TM_COUNT]);
    if (err != hipSuccess) return hip_status(err);
  }
  if (!per_call) stage_ms_out[KGE_TIMER_STAGES] = (float)calls;
  return KGE_OK;
}

}  // extern "C"
