// kge_kernels.inc — model-templated HIP kernels (included once per model TU).
//
// Kernels (see DESIGN.md for the roofline of each):
//   k_score        forward scores              model.py:72-249
//   k_row          per-positive-row pass:      model.py:268-288 (+ the q-side backward)
//                  op = TRAIN: fused negative scoring + self-adversarial loss with an
//                  online softmax (one read of every gathered row) + positive score;
//                  op = GIVEN: backward of forward() for a given dL/dscore.
//   k_entity       entity-major gradient pass: one wave per entity row, sums its
//                  occurrences in a fixed (sorted) order and writes the DENSE gradient
//                  row (the reference's IndexSelectBackward zero-fill + index_add_).
//   k_rank_prep / k_rank_tile / k_rank_scan   filtered ranking, model.py:383-418 (fast
//                  fp32 passes counting the clear cases, listing near-ties)
//   k_rank_window / k_rank_refine / k_rank_exact   the near-tie refinement in the
//                  reference's own fp32 operation order (kge_rank_ref.h)
//   k_topk_prep / k_topk_tile / k_topk_scan   top-k link prediction (kge_topk): the
//                  ranking's all-entity passes with a selecting epilogue
//   k_topk_prep_rows   kge_topk_shard's prep: q from the caller's fixed_rows; the two
//                  scan kernels then run unchanged on a shard-local view of the table
#include "kge_internal.h"
#include "kge_rank_ref.h"
#include "kge_rel.h"


namespace kge {

// ------------------------------------------------------------------ forward
template <int M, int MODE, int VEC, int NS>
__global__ __launch_bounds__(256) void k_score(ScoreArgs a) {
  constexpr bool CPLX = Traits<M>::cplx;
  using R_ = Row<NS, VEC, CPLX>;
  const int lane = threadIdx.x & 63;
  const int64_t unit = (int64_t)blockIdx.x * 4 + wave_id();
  const int64_t chunks = (a.n + a.jpw - 1) / a.jpw;
  if (unit >= a.B * chunks) return;
  const int64_t i = unit / chunks;
  const int64_t j0 = (unit - i * chunks) * a.jpw;
  const int64_t j1 = (j0 + a.jpw < a.n) ? (j0 + a.jpw) : a.n;
  Consts c = a.c;
  if constexpr (M == PROTATE) c.modulus = a.modulus[0];

  const int64_t h = a.pos[i * 3], r = a.pos[i * 3 + 1], t = a.pos[i * 3 + 2];
  const int64_t x = (MODE == HEAD_BATCH) ? t : h;
  float* out = a.out + i * a.n;
  if (x < 0 || x >= a.E || r < 0 || r >= a.R) {
    if (lane == 0) atomicOr(a.err, KGE_DEVERR_INDEX);
    for (int64_t j = j0 + lane; j < j1; j += 64) out[j] = 0.f;
    return;
  }
  R_ q;
  {
    R_ xr, rr;
    load_row<NS, VEC, CPLX>(a.ent + x * a.Le, a.eg, lane, xr);
    load_rel<M, NS, VEC, CPLX>(a.rel + r * a.Lr, a.eg, lane, rr);
    build_q<M, MODE, NS, VEC, CPLX>(xr, rr, c, q);
  }
  const int64_t* nb = a.neg + i * a.neg_stride;
  int64_t j = j0;
  for (; j + 1 < j1; j += 2) {
    int64_t e0 = nb[j], e1 = nb[j + 1];
    const bool b0 = (e0 < 0 || e0 >= a.E), b1 = (e1 < 0 || e1 >= a.E);
    if ((b0 || b1) && lane == 0) atomicOr(a.err, KGE_DEVERR_INDEX);
    e0 = b0 ? 0 : e0;
    e1 = b1 ? 0 : e1;
    R_ r0, r1;
    load_row<NS, VEC, CPLX>(a.ent + e0 * a.Le, a.eg, lane, r0);
    load_row<NS, VEC, CPLX>(a.ent + e1 * a.Le, a.eg, lane, r1);
    const float t0 = wave_sum(lane_total<M, MODE, NS, VEC, CPLX>(q, r0, c));
    const float t1 = wave_sum(lane_total<M, MODE, NS, VEC, CPLX>(q, r1, c));
    if (lane == 0) {
      out[j] = Elem<M, MODE>::finish(t0, c);
      out[j + 1] = Elem<M, MODE>::finish(t1, c);
    }
  }
  if (j < j1) {
    int64_t e0 = nb[j];
    if (e0 < 0 || e0 >= a.E) {
      if (lane == 0) atomicOr(a.err, KGE_DEVERR_INDEX);
      e0 = 0;
    }
    R_ r0;
    load_row<NS, VEC, CPLX>(a.ent + e0 * a.Le, a.eg, lane, r0);
    const float t0 = wave_sum(lane_total<M, MODE, NS, VEC, CPLX>(q, r0, c));
    if (lane == 0) out[j] = Elem<M, MODE>::finish(t0, c);
  }
}

// ------------------------------------------------------------- row pass
//   k_row      one workgroup (4 waves) per positive row: q_i (tail/single:
//              f(h, r), head: f(r, t)) in its prologue, the gather loop below,
//              and (fused) the epilogue
//   k_build_q  one wave per row: q_i alone (the factor exchange's global step)
//   k_row_epi  one workgroup per row: positive score + chain rule q → (h|t, r)
//              (when the epilogue is not fused: phased / exchanged steps)

template <int M, int MODE, int VEC, int NS>
__global__ __launch_bounds__(256) void k_build_q(RowArgs a) {
  constexpr bool CPLX = Traits<M>::cplx;
  using R_ = Row<NS, VEC, CPLX>;
  const int lane = threadIdx.x & 63;
  if (a.wsum_out && blockIdx.x == 0) {
    // Σ subsampling_weight, for k_row / finalize
    __shared__ float red[256];
    const float tot = block_weight_sum(a.sub_w, a.B, red);
    if (threadIdx.x == 0) a.wsum_out[0] = tot;
  }
  const int64_t i = (int64_t)blockIdx.x * 4 + wave_id();
  if (i >= a.B) return;
  Consts c = a.c;
  if constexpr (M == PROTATE) c.modulus = a.modulus[0];
  const int64_t h = a.pos[i * 3], r = a.pos[i * 3 + 1], t = a.pos[i * 3 + 2];
  const int64_t x = (MODE == HEAD_BATCH) ? t : h;
  R_ q;
  if (h < 0 || h >= a.E || t < 0 || t >= a.E || r < 0 || r >= a.R) {
    if (lane == 0) atomicOr(a.err, KGE_DEVERR_INDEX);
    zero_row<NS, VEC, CPLX>(q);
  } else {
    R_ xr, rr;
    load_row<NS, VEC, CPLX>(a.ent + x * a.Le, a.eg, lane, xr);
    load_rel<M, NS, VEC, CPLX>(a.rel + r * a.Lr, a.eg, lane, rr);
    build_q<M, MODE, NS, VEC, CPLX>(xr, rr, c, q);
  }
  store_row<NS, VEC, CPLX>(a.q_out + i * a.Le, a.eg, lane, q);
}

// Positive score + chain rule q → (h|t, r) for row i (model.py:268-301), with
// dL/dq of the negatives read from DQ (global dq_out for k_row_epi, the LDS
// merge buffer for k_row's fused tail).  Called by all 256 threads.  W4: the
// elementwise chain rule on float4 groups (k_row_epi with float4-aligned rows;
// the same per-element operations, so the same bits as the scalar loop the
// fused tail keeps for its register budget).
// PP: the positive's per-element terms come from k_row's prologue (pphi)
template <int M, int MODE, int VEC, int NS, bool W4 = false, bool PP = false>
__device__ __forceinline__ void row_epilogue(const RowArgs& a, int64_t i, const float* DQ, float* gp_slot,
                                             float ci_known = -1.f, const float* pphi = nullptr) {
  constexpr bool CPLX = Traits<M>::cplx;
  using R_ = Row<NS, VEC, CPLX>;
  using EL = Elem<M, MODE>;
  using ELT = Elem<M, TAIL_BATCH>;
  const int tid = threadIdx.x, lane = tid & 63, w = wave_id();
  const bool train = (a.op == ROW_TRAIN);
  Consts c = a.c;
  if constexpr (M == PROTATE) c.modulus = a.modulus[0];
  const int64_t h = a.pos[i * 3], r = a.pos[i * 3 + 1], t = a.pos[i * 3 + 2];
  float* D0 = a.ent_contrib + (2 * i) * a.Le;      // head slot
  float* D1 = a.ent_contrib + (2 * i + 1) * a.Le;  // tail slot
  float* DR = a.rel_contrib + i * a.Lr;
  if (h < 0 || h >= a.E || t < 0 || t >= a.E || r < 0 || r >= a.R) {
    for (int k = tid; k < a.Le; k += 256) { D0[k] = 0.f; D1[k] = 0.f; }
    for (int k = tid; k < a.Lr; k += 256) DR[k] = 0.f;
    if (tid < 4) a.row_stats[i * 4 + tid] = 0.f;
    return;
  }
  if (train && w == 0) {
    // c_i: from the caller when it has it (k_row's fused tail: the global Σw
    // is published by block 0 of the SAME launch, so it must not be read here)
    const float ci = (ci_known >= 0.f) ? ci_known : (a.uni_weight ? a.uni_inv : (a.sub_w[i] / a.w_sum[0]));
    // lane_total's sequential (slot group, element) order, one slot group of
    // h, r, t at a time: a quarter of the registers of whole rows (the fused
    // k_row tail spilled with them)
    using R1 = Row<1, VEC, CPLX>;
    float accp = 0.f;
    if constexpr (PP) {
      // the per-element terms the prologue's four waves evaluated (k_row,
      // FE): summed here in the same order
#pragma unroll
      for (int sg = 0; sg < NS; ++sg)
#pragma unroll
        for (int v = 0; v < VEC; ++v) accp += pphi[(sg * 64 + lane) * VEC + v];
    } else
#pragma unroll
    for (int sg = 0; sg < (NS > 0 ? NS : (a.eg.S + 63) / 64); ++sg) {  // NS = 0: wide rows (kge_wide.inc)
      const int ln = lane + 64 * sg;
      R1 hr, rr, tr, qp;
      load_row<1, VEC, CPLX>(a.ent + h * a.Le, a.eg, ln, hr);
      load_rel<M, 1, VEC, CPLX>(a.rel + r * a.Lr, a.eg, ln, rr);
      load_row<1, VEC, CPLX>(a.ent + t * a.Le, a.eg, ln, tr);
      build_q<M, TAIL_BATCH, 1, VEC, CPLX>(hr, rr, c, qp);
#pragma unroll
      for (int v = 0; v < VEC; ++v) {
        if constexpr (CPLX) accp += ELT::phi(qp.a[0][v], qp.b[0][v], tr.a[0][v], tr.b[0][v], c);
        else accp += ELT::phi(qp.a[0][v], 0.f, tr.a[0][v], 0.f, c);
      }
    }
    const float totp = wave_sum(accp);
    const float sp = ELT::finish(totp, c);
    if (lane == 0) {
      const float gp = -0.5f * ci * sigmoidf(-sp);
      *gp_slot = gp;
      a.row_stats[i * 4 + 0] = log_sigmoid(sp);
      a.row_stats[i * 4 + 2] += gp * (-totp);
      a.row_stats[i * 4 + 3] = sp;
    }
  }
  if (!train && tid == 0) {
    a.row_stats[i * 4 + 0] = 0.f;
    a.row_stats[i * 4 + 3] = 0.f;
  }
  __syncthreads();
  const float gp = train ? *gp_slot : 0.f;
  const float* H = a.ent + h * a.Le;
  const float* Tt = a.ent + t * a.Le;
  const float* Rr = a.rel + r * a.Lr;
  const int K = CPLX ? (a.Le / 2) : a.Le;
  if constexpr (W4 && VEC == 4) {
    // one element: positive-side grads (tail formulas, x = head, e = tail) and
    // the chain rule of the negatives' dL/dq
    auto elem = [&](float ha, float hb, float ta, float tb, float ra, float rb, float dqa, float dqb, float& d0a,
                    float& d0b, float& d1a, float& d1b, float& dra, float& drb) {
      float pqa = 0.f, pqb = 0.f, pta = 0.f, ptb = 0.f;
      if (train) {
        float qa, qb, gqa, gqb, gea, geb;
        ELT::make_q(ha, hb, ra, rb, c, qa, qb);
        ELT::grads(qa, qb, ta, tb, c, gqa, gqb, gea, geb);
        pqa = gp * gqa; pqb = gp * gqb; pta = gp * gea; ptb = gp * geb;
      }
      if constexpr (MODE == HEAD_BATCH) {
        float dta, dtb, rna, rnb;
        EL::chain(ta, tb, ra, rb, dqa, dqb, c, dta, dtb, rna, rnb);
        float dha = 0.f, dhb = 0.f, rpa = 0.f, rpb = 0.f;
        if (train) ELT::chain(ha, hb, ra, rb, pqa, pqb, c, dha, dhb, rpa, rpb);
        d0a = dha; d0b = dhb;
        d1a = dta + pta; d1b = dtb + ptb;
        dra = rna + rpa; drb = rnb + rpb;
      } else {
        float dha, dhb;
        EL::chain(ha, hb, ra, rb, dqa + pqa, dqb + pqb, c, dha, dhb, dra, drb);
        d0a = dha; d0b = dhb;
        d1a = pta; d1b = ptb;
      }
    };
    constexpr bool RB = CPLX && !Traits<M>::rel_phase;  // the relation row has an imaginary half
    for (int k = tid * 4; k < K; k += 1024) {
      float ha[4], hb[4], ta[4], tb[4], ra[4], rb[4], qa[4], qb[4];
      float o0a[4], o0b[4], o1a[4], o1b[4], ora[4], orb[4];
      ldv<4>(H + k, ha);
      ldv<4>(Tt + k, ta);
      ldv<4>(Rr + k, ra);
      ldv<4>(DQ + k, qa);
      if constexpr (CPLX) {
        ldv<4>(H + K + k, hb);
        ldv<4>(Tt + K + k, tb);
        ldv<4>(DQ + K + k, qb);
      } else {
        zv<4>(hb); zv<4>(tb); zv<4>(qb);
      }
      if constexpr (RB) ldv<4>(Rr + K + k, rb);
      else zv<4>(rb);
#pragma unroll
      for (int e = 0; e < 4; ++e)
        elem(ha[e], hb[e], ta[e], tb[e], ra[e], rb[e], qa[e], qb[e], o0a[e], o0b[e], o1a[e], o1b[e], ora[e], orb[e]);
      stv<4>(D0 + k, o0a);
      stv<4>(D1 + k, o1a);
      stv<4>(DR + k, ora);
      if constexpr (CPLX) {
        stv<4>(D0 + K + k, o0b);
        stv<4>(D1 + K + k, o1b);
      }
      if constexpr (RB) stv<4>(DR + K + k, orb);
    }
    return;
  }
  // four elements per thread and pass, all their loads issued before the
  // first store (the stores may alias the rows as far as the compiler knows)
  constexpr int UE = 4;
  for (int k0 = tid; k0 < K; k0 += 256 * UE) {
  float Ha[UE], Hb[UE], Ta[UE], Tb[UE], Ra[UE], Rb[UE], Qa[UE], Qb[UE];
#pragma unroll
  for (int u = 0; u < UE; ++u) {
    const int k = k0 + 256 * u < K ? k0 + 256 * u : k0;
    const int kb = CPLX ? (K + k) : k;
    Ha[u] = H[k]; Hb[u] = CPLX ? H[kb] : 0.f;
    Ta[u] = Tt[k]; Tb[u] = CPLX ? Tt[kb] : 0.f;
    if constexpr (Traits<M>::rel_phase) { Ra[u] = Rr[k]; Rb[u] = 0.f; }
    else { Ra[u] = Rr[k]; Rb[u] = CPLX ? Rr[kb] : 0.f; }
    Qa[u] = DQ[k]; Qb[u] = CPLX ? DQ[kb] : 0.f;
  }
#pragma unroll
  for (int u = 0; u < UE; ++u) {
    const int k = k0 + 256 * u;
    if (k >= K) break;
    const int kb = CPLX ? (K + k) : k;
    const float ha = Ha[u], hb = Hb[u], ta = Ta[u], tb = Tb[u], ra = Ra[u], rb = Rb[u];
    const float dqa = Qa[u], dqb = Qb[u];
    // positive-side grads (tail formulas, x = head, e = tail)
    float pqa = 0.f, pqb = 0.f, pta = 0.f, ptb = 0.f;
    if (train) {
      float qa, qb, gqa, gqb, gea, geb;
      ELT::make_q(ha, hb, ra, rb, c, qa, qb);
      ELT::grads(qa, qb, ta, tb, c, gqa, gqb, gea, geb);
      pqa = gp * gqa; pqb = gp * gqb; pta = gp * gea; ptb = gp * geb;
    }
    float d0a, d0b, d1a, d1b, dra, drb;
    if constexpr (MODE == HEAD_BATCH) {
      float dta, dtb, rna, rnb;
      EL::chain(ta, tb, ra, rb, dqa, dqb, c, dta, dtb, rna, rnb);
      float dha = 0.f, dhb = 0.f, rpa = 0.f, rpb = 0.f;
      if (train) ELT::chain(ha, hb, ra, rb, pqa, pqb, c, dha, dhb, rpa, rpb);
      d0a = dha; d0b = dhb;
      d1a = dta + pta; d1b = dtb + ptb;
      dra = rna + rpa; drb = rnb + rpb;
    } else {
      float dha, dhb;
      EL::chain(ha, hb, ra, rb, dqa + pqa, dqb + pqb, c, dha, dhb, dra, drb);
      d0a = dha; d0b = dhb;
      d1a = pta; d1b = ptb;
    }
    D0[k] = d0a; D1[k] = d1a;
    if constexpr (CPLX) { D0[kb] = d0b; D1[kb] = d1b; }
    DR[k] = dra;
    if constexpr (CPLX && !Traits<M>::rel_phase) DR[kb] = drb;
  }
  }
}

// Wave w scores negatives j = w, w+4, ... of row i, reading q_i from LDS and
// the gathered rows from HBM with the next row already in flight.  Each
// element is evaluated once (phi_dir): the score term, and in place the
// direction ∂s/∂q needs.  Every wave keeps an online-softmax state (m, Z) and
// V = Σ_j p_j σ(s_j) ∂s_j/∂q in registers, so each gathered row is read
// exactly once; the four states merge through LDS as (V0 + V2) + (V1 + V3).
// The block builds q_i (and Σw) itself in its prologue; FE: the epilogue
// (positive score, chain rule) runs in its tail instead of k_row_epi.
// SH (query shipping, kge_ship_step): q_i is the shipped vector, only the
// negatives this rank owns are scored, and the row's partial state — (max,
// Z, NL, MG) and V relative to this shard's max, unnormalised — goes to
// global memory for the cross-shard merge (k_ship_merge) instead of dL/ds.
template <int M, int MODE, int VEC, int NS, bool FE, bool SH = false>
__global__ __launch_bounds__(256, 4) void k_row(RowArgs a) {
  constexpr bool CPLX = Traits<M>::cplx;
  using R_ = Row<NS, VEC, CPLX>;
  using EL = Elem<M, MODE>;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int QP = 64 * NS * VEC;        // padded slot span of one (half-)row
  float* qs = smem;                        // [2*QP]   q_i, zero-padded per half
  float* Vb = smem + 2 * QP;               // [2][Le]  V merge buffer (>= 256 floats: also the Σw tree)
  float* s_lds = Vb + vb_floats(a.Le); // [n]      raw negative scores (TRAIN)
  float* st = s_lds + a.n_lds;             // [16]     per-wave (m, Z, NL, MG)
  float* pphi = st + 32;                   // [64*NS*VEC] FE: the positive triple's per-element terms

  const int tid = threadIdx.x, lane = tid & 63, w = wave_id();
  const int64_t i = blockIdx.x;
  const bool train = (a.op == ROW_TRAIN);
  const bool adv = train && a.adversarial;
  Consts c = a.c;
  if constexpr (M == PROTATE) c.modulus = a.modulus[0];

  const int64_t* nb = a.neg + i * a.neg_stride;
  auto row_ptr = [&](int64_t j) -> const float* {
    int64_t e = nb[j];
    if (e < 0 || e >= a.E) {
      if (lane == 0) atomicOr(a.err, KGE_DEVERR_INDEX);
      e = 0;
    }
    return a.ent + e * a.Le;
  };
  // negative rows through buffer descriptors (VEC = 4): the re and im halves
  // (or the whole real row) are separate buffers, so the slots past the row
  // end read 0 from the hardware range check — no per-slot selects, and the
  // slot offsets are per-lane constants
  const uint32_t hb = (uint32_t)(CPLX ? a.eg.half : a.Le) * 4u;
  auto load_neg = [&](int64_t j, R_& r) {
    const float* base = row_ptr(j);
    if constexpr (VEC == 4) {
      const auto ra = buf_rsrc(base, hb);
#pragma unroll
      for (int k = 0; k < NS; ++k) buf_ld4(ra, (uint32_t)(lane + 64 * k) * 16u, r.a[k]);
      if constexpr (CPLX) {
        const auto rb = buf_rsrc(base + a.eg.half, hb);
#pragma unroll
        for (int k = 0; k < NS; ++k) buf_ld4(rb, (uint32_t)(lane + 64 * k) * 16u, r.b[k]);
      }
    } else {
      load_row<NS, VEC, CPLX>(base, a.eg, lane, r);
    }
  };
  // the wave's first negative row is requested before the prologue, so its
  // gather overlaps the Σw reduction and the q build (MALL latency, once per
  // wave, at a moment when every block of the launch is in its prologue)
  R_ er0;
  const bool pre = !SH && w < a.n;
  if (pre) load_neg(w, er0);
  float ci = 1.f;
  // Σw (every block, same order; block 0 publishes it)
  if (SH) {
    // c_i enters at the merge
  } else if (train && !a.uni_weight) {
    float wsum;
    if (a.wsum_out) {
      wsum = block_weight_sum(a.sub_w, a.B, Vb);  // Vb is free until the merge
      if (blockIdx.x == 0 && tid == 0) a.wsum_out[0] = wsum;
    } else {
      wsum = a.w_sum[0];
    }
    ci = a.sub_w[i] / wsum;
  } else if (train) {
    ci = a.uni_inv;
  }
  {
    // q build: wave w builds q's slot groups w (and w + 4) straight
    // into the zero-padded LDS copy and the global q buffer (entity pass)
    using R1 = Row<1, VEC, CPLX>;
    const int64_t h = a.pos[i * 3], r = a.pos[i * 3 + 1], t = a.pos[i * 3 + 2];
    const int64_t x = (MODE == HEAD_BATCH) ? t : h;
    const bool bad = (h < 0 || h >= a.E || t < 0 || t >= a.E || r < 0 || r >= a.R);
    if (bad && tid == 0) atomicOr(a.err, KGE_DEVERR_INDEX);
#pragma unroll
    for (int k = w; k < NS; k += 4) {
      const int ln = lane + 64 * k;  // slot of this lane in group k
      R1 q1, xr, rr;
      if constexpr (SH) {
        load_row<1, VEC, CPLX>(a.sh.q_in + i * a.Le, a.eg, ln, q1);
      } else if (bad) {
        zero_row<1, VEC, CPLX>(q1);
      } else {
        load_row<1, VEC, CPLX>(a.ent + x * a.Le, a.eg, ln, xr);
        load_rel<M, 1, VEC, CPLX>(a.rel + r * a.Lr, a.eg, ln, rr);
        build_q<M, MODE, 1, VEC, CPLX>(xr, rr, c, q1);
      }
      if constexpr (FE && !SH) {
        // the positive triple's per-element terms (tail form, x = head, e =
        // tail; model.py:277-279), in parallel here instead of on one wave
        // in the epilogue; row_epilogue sums them in lane_total's order
        if (train && !bad) {
          using ELT = Elem<M, TAIL_BATCH>;
          R1 tq, yr;
          if constexpr (MODE == TAIL_BATCH) {
            tq = q1;
            load_row<1, VEC, CPLX>(a.ent + t * a.Le, a.eg, ln, yr);
          } else {
            R1 hr1;
            load_row<1, VEC, CPLX>(a.ent + h * a.Le, a.eg, ln, hr1);
            build_q<M, TAIL_BATCH, 1, VEC, CPLX>(hr1, rr, c, tq);
            yr = xr;
          }
#pragma unroll
          for (int v = 0; v < VEC; ++v) {
            if constexpr (CPLX) pphi[ln * VEC + v] = ELT::phi(tq.a[0][v], tq.b[0][v], yr.a[0][v], yr.b[0][v], c);
            else pphi[ln * VEC + v] = ELT::phi(tq.a[0][v], 0.f, yr.a[0][v], 0.f, c);
          }
        }
      }
      if constexpr (!SH) store_row<1, VEC, CPLX>(a.q_out + i * a.Le, a.eg, ln, q1);
      if constexpr (!SH && VEC == 4) {
        // the entity pass's copy: slice-major, each (slice, row) 2 KB contiguous
        if (a.q_sl && ln < a.eg.S) {
          const int sl = ln / a.q_sl_w, p = ln - sl * a.q_sl_w;
          float* dst = a.q_sl + (((int64_t)sl * a.B + i) * 2) * 256 + p * 4;
          stv<4>(dst, q1.a[0]);
          if constexpr (CPLX) stv<4>(dst + 256, q1.b[0]);
        }
      }
      const bool in = ln < a.eg.S;
#pragma unroll
      for (int v = 0; v < VEC; ++v) {
        qs[ln * VEC + v] = in ? q1.a[0][v] : 0.f;
        if constexpr (CPLX) qs[QP + ln * VEC + v] = in ? q1.b[0][v] : 0.f;
      }
    }
  }
  __syncthreads();

  R_ V;
  zero_row<NS, VEC, CPLX>(V);
  float m = -INFINITY, Z = 0.f, NL = 0.f, MG = 0.f;
  const float T = a.adv_T;

  for (int64_t j = w; j < a.n; j += 4) {
    if constexpr (SH) {  // another shard's row: scored there (wave-uniform skip)
      const int64_t e = nb[j];
      if (e < a.sh.own_lo || e >= a.sh.own_hi) {
        if ((e < 0 || e >= a.E) && lane == 0) atomicOr(a.err, KGE_DEVERR_INDEX);
        continue;
      }
    }
    R_ er;
    if (pre && j == w) er = er0;
    else load_neg(j, er);
    float part = 0.f;
    constexpr bool PK = (M == ROTATE && VEC == 4);  // explicit register-pair (v_pk_*) form
#pragma unroll
    for (int k = 0; k < NS && PK; ++k) {
      // Elem<ROTATE>::phi_dir on element pairs (v, v+1): the same IEEE
      // operations in the same order, so bit-identical to the scalar loop
      const int slot = lane + 64 * k;
      float qa[VEC], qb[VEC];
      ldv<VEC>(qs + slot * VEC, qa);
      ldv<VEC>(qs + QP + slot * VEC, qb);
#pragma unroll
      for (int v = 0; v < VEC; v += 2) {
        const tf2 dr = tf2{qa[v], qa[v + 1]} - tf2{er.a[k][v], er.a[k][v + 1]};
        const tf2 di = tf2{qb[v], qb[v + 1]} - tf2{er.b[k][v], er.b[k][v + 1]};
        const tf2 s2 = dr * dr + di * di;
        const float r0 = fsqrt(s2.x), r1 = fsqrt(s2.y);
        const tf2 inv = tf2{(r0 > 0.f) ? frcp(r0) : 0.f, (r1 > 0.f) ? frcp(r1) : 0.f};
        const tf2 ur = dr * inv, ui = di * inv;
        er.a[k][v] = ur.x; er.a[k][v + 1] = ur.y;
        er.b[k][v] = ui.x; er.b[k][v + 1] = ui.y;
        part += r0;
        part += r1;
      }
    }
#pragma unroll
    for (int k = 0; k < NS && !PK; ++k) {
      // q is zero-padded in LDS to the full slot span: lanes past the row end
      // see q = 0 against a zeroed row, so they add 0 and need no select
      const int slot = lane + 64 * k;
      float qa[VEC], qb[VEC];
      ldv<VEC>(qs + slot * VEC, qa);
      if constexpr (CPLX) ldv<VEC>(qs + QP + slot * VEC, qb);
      else zv<VEC>(qb);
#pragma unroll
      for (int v = 0; v < VEC; ++v) {
        if constexpr (CPLX) part += EL::phi_dir(qa[v], qb[v], er.a[k][v], er.b[k][v], c);
        else {
          float dummy = 0.f;
          part += EL::phi_dir(qa[v], 0.f, er.a[k][v], dummy, c);
        }
      }
    }
    const float tot = wave_sum(part);
    const float s = EL::finish(tot, c);
    float cv;
    if (train) {
      if (lane == 0) {
        if constexpr (SH) a.sh.s_out[i * a.n + j] = s;
        else s_lds[j] = s;
      }
      float p = 1.f;
      if (adv) {
        const float xs = T * s;  // negative_score * adversarial_temperature, model.py:272
        if (xs > m) {
          const float sc = (m == -INFINITY) ? 0.f : __expf(m - xs);
#pragma unroll
          for (int k = 0; k < NS; ++k)
#pragma unroll
            for (int v = 0; v < VEC; ++v) {
              V.a[k][v] *= sc;
              if constexpr (CPLX) V.b[k][v] *= sc;
            }
          Z *= sc; NL *= sc; MG *= sc;
          m = xs;
        }
        p = __expf(xs - m);
      }
      Z += p;
      NL += p * log_sigmoid(-s);
      cv = p * sigmoidf(s);
    } else {
      cv = a.g_in[i * a.n + j];
    }
    MG += cv * (-tot);
    if constexpr (PK) {  // Elem<ROTATE>::dq_of + accumulate, on register pairs
      const tf2 nw = tf2{-cv, -cv};
#pragma unroll
      for (int k = 0; k < NS; ++k) {
#pragma unroll
        for (int v = 0; v < VEC; v += 2) {
          const tf2 va = tf2{V.a[k][v], V.a[k][v + 1]} + nw * tf2{er.a[k][v], er.a[k][v + 1]};
          V.a[k][v] = va.x; V.a[k][v + 1] = va.y;
          const tf2 vb = tf2{V.b[k][v], V.b[k][v + 1]} + nw * tf2{er.b[k][v], er.b[k][v + 1]};
          V.b[k][v] = vb.x; V.b[k][v + 1] = vb.y;
        }
      }
      continue;
    }
#pragma unroll
    for (int k = 0; k < NS; ++k)
#pragma unroll
      for (int v = 0; v < VEC; ++v) {
        float da, db;
        if constexpr (CPLX) {
          EL::dq_of(er.a[k][v], er.b[k][v], cv, c, da, db);
          V.b[k][v] += db;
        } else {
          EL::dq_of(er.a[k][v], 0.f, cv, c, da, db);
        }
        V.a[k][v] += da;
      }
  }

  // ---- merge the four wave states: (V0 + V2) + (V1 + V3), each scaled by
  // its softmax rescale factor exp(m_w - max m)
  if (lane == 0) {
    st[w * 4 + 0] = m; st[w * 4 + 1] = Z; st[w * 4 + 2] = NL; st[w * 4 + 3] = MG;
  }
  __syncthreads();
  float f[4];
  float Mx = -INFINITY;
  if (adv) {
#pragma unroll
    for (int u = 0; u < 4; ++u) Mx = fmaxf(Mx, st[u * 4]);
#pragma unroll
    for (int u = 0; u < 4; ++u) f[u] = (st[u * 4] == -INFINITY) ? 0.f : expf(st[u * 4] - Mx);
  } else {
#pragma unroll
    for (int u = 0; u < 4; ++u) f[u] = 1.f;
  }
  float Zt = 0.f, NLt = 0.f, MGt = 0.f;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    Zt += f[u] * st[u * 4 + 1];
    NLt += f[u] * st[u * 4 + 2];
    MGt += f[u] * st[u * 4 + 3];
  }
  const float nf = (float)a.n;
  // dL/dq (negatives) = 0.5 c_i Σ_j a_ij σ(s_ij) ∂s/∂q, a_ij = p_j / Z (adv) or 1/n
  const float vscale = (train && !SH) ? (adv ? (0.5f * ci / Zt) : (0.5f * ci / nf)) : 1.f;
  const float fw = f[w];
#pragma unroll
  for (int k = 0; k < NS; ++k)
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
      V.a[k][v] *= fw;
      if constexpr (CPLX) V.b[k][v] *= fw;
    }
  if (w >= 2) store_row<NS, VEC, CPLX>(Vb + (w - 2) * a.Le, a.eg, lane, V);
  __syncthreads();
  if (w < 2) {
    R_ o;
    load_row<NS, VEC, CPLX>(Vb + w * a.Le, a.eg, lane, o);
#pragma unroll
    for (int k = 0; k < NS; ++k)
#pragma unroll
      for (int v = 0; v < VEC; ++v) {
        V.a[k][v] += o.a[k][v];
        if constexpr (CPLX) V.b[k][v] += o.b[k][v];
      }
  }
  __syncthreads();
  if (w == 1) store_row<NS, VEC, CPLX>(Vb, a.eg, lane, V);
  __syncthreads();
  if (w == 0) {
    R_ o;
    load_row<NS, VEC, CPLX>(Vb, a.eg, lane, o);
#pragma unroll
    for (int k = 0; k < NS; ++k)
#pragma unroll
      for (int v = 0; v < VEC; ++v) {
        V.a[k][v] = (V.a[k][v] + o.a[k][v]) * vscale;
        if constexpr (CPLX) V.b[k][v] = (V.b[k][v] + o.b[k][v]) * vscale;
      }
    // dL/dq of the negatives: to the epilogue (fused: through LDS)
    store_row<NS, VEC, CPLX>(FE ? Vb : a.dq_out + i * a.Le, a.eg, lane, V);
    if (lane == 0) {
      if constexpr (SH) {
        a.sh.part_out[i * 4 + 0] = Mx;
        a.sh.part_out[i * 4 + 1] = Zt;
        a.sh.part_out[i * 4 + 2] = NLt;
        a.sh.part_out[i * 4 + 3] = MGt;
      } else {
        a.row_stats[i * 4 + 1] = train ? (adv ? (NLt / Zt) : (NLt / nf)) : 0.f;
        a.row_stats[i * 4 + 2] = train ? (0.5f * ci * MGt / (adv ? Zt : nf)) : MGt;
      }
    }
  }
  if (train && !SH) {
    // dL/ds_ij for the entity-major pass (model.py:272-288, closed form)
    for (int64_t j = tid; j < a.n; j += 256) {
      const float s = s_lds[j];
      const float aij = adv ? (expf(T * s - Mx) / Zt) : (1.f / nf);
      a.g_out[i * a.n + j] = 0.5f * ci * aij * sigmoidf(s);
    }
  }
  if constexpr (FE) {
    // fused k_row_epi: the same device function, dq from the merge buffer
    __syncthreads();
    row_epilogue<M, MODE, VEC, NS, false, true>(a, i, Vb, st, ci, pphi);
  }
}

// Positive triple ('single' mode, model.py:277-279) and the elementwise chain
// rule from dL/dq to the rows' head / tail / relation contributions.
template <int M, int MODE, int VEC, int NS>
__global__ __launch_bounds__(256) void k_row_epi(RowArgs a) {
  __shared__ float gp_s;
  row_epilogue<M, MODE, VEC, NS, true>(a, blockIdx.x, a.dq_out + (int64_t)blockIdx.x * a.Le, &gp_s);
}

// ------------------------------------------------------- query shipping
// kge_ship_step: the entity table is split into row shards, one per rank, and
// no rank holds another's rows.  The ranks ship the q vectors of the global
// batch instead of rows: each shard scores the negatives it owns for every
// row (k_row<SH>), the partial softmax states are merged across shards in
// shard order (k_ship_merge), and every row-side term is computed where its
// row lives (k_ship_q, k_ship_chain).  Row slots of the same launch read
// only owned rows; everything else arrives through the host's collectives.

__device__ __forceinline__ bool owned(const ShipArgs& s, int64_t e) { return e >= s.own_lo && e < s.own_hi; }

// One wave per row: q_i from the owner of its x row (zero on the other
// shards, so the all-reduce that follows yields q on every rank); head-batch
// also the positive's tail-form q (h∘r) from the owner of h.
template <int M, int MODE, int VEC, int NS>
__global__ __launch_bounds__(256) void k_ship_q(RowArgs a) {
  constexpr bool CPLX = Traits<M>::cplx;
  using R_ = Row<NS, VEC, CPLX>;
  const int lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * 4 + wave_id();
  if (i >= a.B) return;
  Consts c = a.c;
  if constexpr (M == PROTATE) c.modulus = a.modulus[0];
  const int64_t h = a.pos[i * 3], r = a.pos[i * 3 + 1], t = a.pos[i * 3 + 2];
  const bool bad = (h < 0 || h >= a.E || t < 0 || t >= a.E || r < 0 || r >= a.R);
  if (bad && lane == 0) atomicOr(a.err, KGE_DEVERR_INDEX);
  const int64_t x = (MODE == HEAD_BATCH) ? t : h;
  R_ q, xr, rr;
  zero_row<NS, VEC, CPLX>(q);
  const bool ox = !bad && owned(a.sh, x), oh = !bad && owned(a.sh, h);
  if (ox || (MODE == HEAD_BATCH && oh)) load_rel<M, NS, VEC, CPLX>(a.rel + r * a.Lr, a.eg, lane, rr);
  if (ox) {
    load_row<NS, VEC, CPLX>(a.ent + x * a.Le, a.eg, lane, xr);
    build_q<M, MODE, NS, VEC, CPLX>(xr, rr, c, q);
  }
  store_row<NS, VEC, CPLX>(a.q_out + i * a.Le, a.eg, lane, q);
  if constexpr (MODE == HEAD_BATCH) {
    zero_row<NS, VEC, CPLX>(q);
    if (oh) {
      load_row<NS, VEC, CPLX>(a.ent + h * a.Le, a.eg, lane, xr);
      build_q<M, TAIL_BATCH, NS, VEC, CPLX>(xr, rr, c, q);
    }
    store_row<NS, VEC, CPLX>(a.sh.qp_out + i * a.Le, a.eg, lane, q);
  }
}

// One workgroup per row, after the all-gather of every shard's partial state:
// the row's softmax max / normaliser in shard order (the same bits on every
// rank), this shard's V rescaled to them, dL/ds of its negatives, and — on
// the owner of t — the positive triple (model.py:277-279): its statistics,
// dL/dq of the positive (added to V; head-batch: its own buffer) and dL/dt.
template <int M, int MODE, int VEC, int NS>
__global__ __launch_bounds__(256) void k_ship_merge(RowArgs a) {
  constexpr bool CPLX = Traits<M>::cplx;
  using R_ = Row<NS, VEC, CPLX>;
  using ELT = Elem<M, TAIL_BATCH>;
  __shared__ float gp_s;
  const int tid = threadIdx.x, lane = tid & 63, w = wave_id();
  const int64_t i = blockIdx.x;
  const bool adv = a.adversarial;
  Consts c = a.c;
  if constexpr (M == PROTATE) c.modulus = a.modulus[0];
  float Mx = -INFINITY;
  if (adv)
    for (int o = 0; o < a.sh.world; ++o) Mx = fmaxf(Mx, a.sh.parts_in[((int64_t)o * a.B + i) * 4]);
  float Zt = 0.f, NLt = 0.f, MGt = 0.f, fme = 0.f;
  for (int o = 0; o < a.sh.world; ++o) {
    const float* p = a.sh.parts_in + ((int64_t)o * a.B + i) * 4;
    const float f = adv ? ((p[0] == -INFINITY) ? 0.f : expf(p[0] - Mx)) : 1.f;
    Zt += f * p[1];
    NLt += f * p[2];
    MGt += f * p[3];
    if (o == a.sh.me) fme = f;
  }
  const float ci = a.uni_weight ? a.uni_inv : (a.sub_w[i] / a.w_sum[0]);
  const float nf = (float)a.n;
  const float vscale = adv ? (0.5f * ci / Zt) : (0.5f * ci / nf);
  if (tid == 0) {
    a.row_stats[i * 4 + 1] = adv ? (NLt / Zt) : (NLt / nf);
    a.row_stats[i * 4 + 2] = 0.5f * ci * MGt / (adv ? Zt : nf);
  }
  float* V = a.dq_out + i * a.Le;
  const float sc = fme * vscale;
  for (int k = tid; k < a.Le; k += 256) V[k] *= sc;
  const int64_t* nb = a.neg + i * a.neg_stride;
  for (int64_t j = tid; j < a.n; j += 256) {
    if (!owned(a.sh, nb[j])) continue;
    const float s = a.sh.s_out[i * a.n + j];
    const float aij = adv ? (expf(a.adv_T * s - Mx) / Zt) : (1.f / nf);
    a.g_out[i * a.n + j] = 0.5f * ci * aij * sigmoidf(s);
  }

  const int64_t h = a.pos[i * 3], r = a.pos[i * 3 + 1], t = a.pos[i * 3 + 2];
  const bool bad = (h < 0 || h >= a.E || t < 0 || t >= a.E || r < 0 || r >= a.R);
  const bool ot = !bad && owned(a.sh, t);
  const float* QP = ((MODE == HEAD_BATCH) ? a.sh.qp_in : a.sh.q_in) + i * a.Le;
  if (w == 0) {
    float ps0 = 0.f, ps2 = 0.f, ps3 = 0.f, gp = 0.f;
    if (ot) {
      R_ qp, tr;
      load_row<NS, VEC, CPLX>(QP, a.eg, lane, qp);
      load_row<NS, VEC, CPLX>(a.ent + t * a.Le, a.eg, lane, tr);
      const float totp = wave_sum(lane_total<M, TAIL_BATCH, NS, VEC, CPLX>(qp, tr, c));
      const float sp = ELT::finish(totp, c);
      gp = -0.5f * ci * sigmoidf(-sp);
      ps0 = log_sigmoid(sp);
      ps2 = gp * (-totp);
      ps3 = sp;
    }
    if (lane == 0) {
      float* ps = a.sh.pstats + i * 4;
      ps[0] = ps0; ps[1] = 0.f; ps[2] = ps2; ps[3] = ps3;
      gp_s = gp;
    }
  }
  __syncthreads();
  const float gp = gp_s;
  const int K = CPLX ? (a.Le / 2) : a.Le;
  const float* Tt = a.ent + t * a.Le;
  float* D1 = a.ent_contrib + (2 * i + 1) * a.Le;
  float* PQ = a.sh.pq + i * a.Le;
  for (int k = tid; k < K; k += 256) {
    const int kb = CPLX ? (K + k) : k;
    float pqa = 0.f, pqb = 0.f;
    if (ot) {
      const float qa = QP[k], qb = CPLX ? QP[kb] : 0.f;
      const float ta = Tt[k], tb = CPLX ? Tt[kb] : 0.f;
      float gqa, gqb, gea, geb;
      ELT::grads(qa, qb, ta, tb, c, gqa, gqb, gea, geb);
      pqa = gp * gqa; pqb = gp * gqb;
      D1[k] = gp * gea;
      if constexpr (CPLX) D1[kb] = gp * geb;
      if constexpr (MODE == TAIL_BATCH) {
        V[k] += pqa;
        if constexpr (CPLX) V[kb] += pqb;
      }
    }
    if constexpr (MODE == HEAD_BATCH) {
      PQ[k] = pqa;
      if constexpr (CPLX) PQ[kb] = pqb;
    }
  }
}

// One workgroup per row, after the all-reduce of dL/dq: the positive's
// statistics into the row statistics, and the chain rule q → (x, r) on the
// owner of x (head-batch: also h∘r → (h, r) on the owner of h).  The
// relation contribution is this shard's part of it (the ranks all-reduce
// the relation gradient).
template <int M, int MODE, int VEC, int NS>
__global__ __launch_bounds__(256) void k_ship_chain(RowArgs a) {
  constexpr bool CPLX = Traits<M>::cplx;
  using EL = Elem<M, MODE>;
  using ELT = Elem<M, TAIL_BATCH>;
  const int tid = threadIdx.x;
  const int64_t i = blockIdx.x;
  Consts c = a.c;
  if constexpr (M == PROTATE) c.modulus = a.modulus[0];
  if (tid == 0) {
    const float* ps = a.sh.pstats + i * 4;
    a.row_stats[i * 4 + 0] = ps[0];
    a.row_stats[i * 4 + 2] += ps[2];
    a.row_stats[i * 4 + 3] = ps[3];
  }
  const int64_t h = a.pos[i * 3], r = a.pos[i * 3 + 1], t = a.pos[i * 3 + 2];
  const bool bad = (h < 0 || h >= a.E || t < 0 || t >= a.E || r < 0 || r >= a.R);
  float* D0 = a.ent_contrib + (2 * i) * a.Le;
  float* D1 = a.ent_contrib + (2 * i + 1) * a.Le;
  float* DR = a.rel_contrib + i * a.Lr;
  const bool oh = owned(a.sh, h), ot = owned(a.sh, t);
  if (bad) {
    for (int k = tid; k < a.Le; k += 256) {
      if (oh) D0[k] = 0.f;
      if (ot) D1[k] = 0.f;
    }
    for (int k = tid; k < a.Lr; k += 256) DR[k] = 0.f;
    return;
  }
  if (!oh && !(MODE == HEAD_BATCH && ot)) {  // no row of this triple here: no relation share either
    for (int k = tid; k < a.Lr; k += 256) DR[k] = 0.f;
    return;
  }
  const float* H = a.ent + h * a.Le;
  const float* Tt = a.ent + t * a.Le;
  const float* Rr = a.rel + r * a.Lr;
  const float* DQ = a.dq_out + i * a.Le;
  const float* PQ = a.sh.pq + i * a.Le;
  const int K = CPLX ? (a.Le / 2) : a.Le;
  for (int k = tid; k < K; k += 256) {
    const int kb = CPLX ? (K + k) : k;
    float ra, rb;
    if constexpr (Traits<M>::rel_phase) { ra = Rr[k]; rb = 0.f; }
    else { ra = Rr[k]; rb = CPLX ? Rr[kb] : 0.f; }
    const float dqa = DQ[k], dqb = CPLX ? DQ[kb] : 0.f;
    float dra = 0.f, drb = 0.f;
    if constexpr (MODE == HEAD_BATCH) {
      float rna = 0.f, rnb = 0.f, rpa = 0.f, rpb = 0.f;
      if (ot) {
        const float ta = Tt[k], tb = CPLX ? Tt[kb] : 0.f;
        float dta, dtb;
        EL::chain(ta, tb, ra, rb, dqa, dqb, c, dta, dtb, rna, rnb);
        D1[k] = dta + D1[k];
        if constexpr (CPLX) D1[kb] = dtb + D1[kb];
      }
      if (oh) {
        const float ha = H[k], hb = CPLX ? H[kb] : 0.f;
        const float pqa = PQ[k], pqb = CPLX ? PQ[kb] : 0.f;
        float dha, dhb;
        ELT::chain(ha, hb, ra, rb, pqa, pqb, c, dha, dhb, rpa, rpb);
        D0[k] = dha;
        if constexpr (CPLX) D0[kb] = dhb;
      }
      dra = rna + rpa;
      drb = rnb + rpb;
    } else if (oh) {
      const float ha = H[k], hb = CPLX ? H[kb] : 0.f;
      float dha, dhb;
      EL::chain(ha, hb, ra, rb, dqa, dqb, c, dha, dhb, dra, drb);
      D0[k] = dha;
      if constexpr (CPLX) D0[kb] = dhb;
    }
    DR[k] = dra;
    if constexpr (CPLX && !Traits<M>::rel_phase) DR[kb] = drb;
  }
}

// ------------------------------------------------------- entity-major pass
// One wave per entity row e: d_ent[e] = Σ_{negative occurrences (i,j) of e}
// g_ij ∂s_ij/∂e  +  Σ_{row slots naming e} ent_contrib  (+ 3λ e|e|), written
// densely, then (optionally) the fused Adam update of the row.
// Latency structure: the bucket's occurrence ids and g values are loaded as
// one vector per 64 occurrences and read back with readlane (no dependent
// scalar load per occurrence); the entity's own row sits in LDS (zero-padded
// like q in k_row) so two q rows can be in flight in registers.
// (3 waves/SIMD: measured, 4 spills and runs slower)
// LAZY (kge_train_step_lazy): the wave's row is rows[place] of the batch's
// touched rows instead of e_begin + place; a place at or past *nrows has no row
// and returns before it reads or writes anything.  Everything after the row is
// chosen is the dense pass's, so a touched row's bits are too.
// OPT (OptKind, the LAZY instantiations of kge_train_step_adagrad): the fused
// step is Adagrad's, element-wise (the state streamed like one Adam moment) or
// row-wise (one state float per row: the row's Σg² is reduced lane-local over
// the lane's elements in slot order, a then b per element as the regulariser's
// partial is, then wave_sum; lane 0 writes G').
template <int M, int MODE, int VEC, int NS, bool LAZY = false, int OPT = OPT_ADAM>
__global__ __launch_bounds__(256, 3) void k_entity(EntArgs a) {
  constexpr bool CPLX = Traits<M>::cplx;
  using R_ = Row<NS, VEC, CPLX>;
  using EL = Elem<M, MODE>;
  constexpr int QP = 64 * NS * VEC;
  __shared__ __attribute__((aligned(16))) float es_all[4][2 * QP];
  const int lane = threadIdx.x & 63;
  const int w = wave_id();
  float* es = es_all[w];
  int64_t e = a.e_begin + (int64_t)blockIdx.x * 4 + w;
  if constexpr (LAZY) {
    const int64_t place = (int64_t)blockIdx.x * 4 + w;
    if (place >= (int64_t)a.nrows[0]) return;
    e = a.rows[place];
  } else {
    if (e >= a.e_end) return;
  }
  Consts c = a.c;
  if constexpr (M == PROTATE) c.modulus = a.modulus[0];
  {
    R_ er;
    load_row<NS, VEC, CPLX>(a.ent + e * a.Le, a.eg, lane, er);
#pragma unroll
    for (int k = 0; k < NS; ++k) {
      stv<VEC>(es + (lane + 64 * k) * VEC, er.a[k]);
      if constexpr (CPLX) stv<VEC>(es + QP + (lane + 64 * k) * VEC, er.b[k]);
    }
  }
  R_ acc;
  zero_row<NS, VEC, CPLX>(acc);
  const int32_t b0 = a.off[e], b1 = a.off[e + 1];
  const uint32_t n32 = (uint32_t)a.n;

  auto accumulate = [&](const R_& qr, float g) {
#pragma unroll
    for (int k = 0; k < NS; ++k) {
      float ea[VEC], eb[VEC];
      ldv<VEC>(es + (lane + 64 * k) * VEC, ea);
      if constexpr (CPLX) ldv<VEC>(es + QP + (lane + 64 * k) * VEC, eb);
#pragma unroll
      for (int v = 0; v < VEC; ++v) {
        float gqa, gqb, gea, geb;
        if constexpr (CPLX) {
          EL::grads(qr.a[k][v], qr.b[k][v], ea[v], eb[v], c, gqa, gqb, gea, geb);
          acc.b[k][v] += g * geb;
        } else {
          EL::grads(qr.a[k][v], 0.f, ea[v], 0.f, c, gqa, gqb, gea, geb);
        }
        acc.a[k][v] += g * gea;
      }
    }
  };

  for (int32_t c0 = b0; c0 < b1; c0 += 64) {
    const int cnt = (b1 - c0 < 64) ? (b1 - c0) : 64;
    // lane l holds occurrence c0 + l: its id, and for a negative its row i and g
    const int32_t o_l = (lane < cnt) ? a.occ[c0 + lane] : 0x7fffffff;
    const bool neg_l = o_l < a.Bn;
    const uint32_t i_l = neg_l ? ((uint32_t)o_l / n32) : 0u;
    const float g_l = neg_l ? a.g[o_l] : 0.f;
    // ids ascend inside a bucket, so the negatives come first
    const int nneg = __popcll(__ballot(neg_l && lane < cnt));
    auto q_of = [&](int p) -> const float* {
      const uint32_t ip = (uint32_t)__builtin_amdgcn_readlane((int)i_l, p);
      return a.q + (int64_t)ip * a.Le;
    };
    // ping-pong: row p+1 is in flight while row p is accumulated
    R_ ra_, rb_;
    if (nneg > 0) load_row<NS, VEC, CPLX>(q_of(0), a.eg, lane, ra_);
    for (int p = 0; p < nneg; p += 2) {
      if (p + 1 < nneg) load_row<NS, VEC, CPLX>(q_of(p + 1), a.eg, lane, rb_);
      // keep the own-row LDS reads inside the loop (hoisting them would pin
      // 32 more VGPRs and cost a wave per SIMD)
      asm volatile("" ::: "memory");
      accumulate(ra_, readlanef(g_l, p));
      if (p + 1 < nneg) {
        if (p + 2 < nneg) load_row<NS, VEC, CPLX>(q_of(p + 2), a.eg, lane, ra_);
        asm volatile("" ::: "memory");
        accumulate(rb_, readlanef(g_l, p + 1));
      }
    }
    for (int p = nneg; p < cnt; ++p) {
      const int32_t o = __builtin_amdgcn_readlane(o_l, p);
      R_ cr;
      load_row<NS, VEC, CPLX>(a.ent_contrib + (int64_t)(o - a.Bn) * a.Le, a.eg, lane, cr);
#pragma unroll
      for (int k = 0; k < NS; ++k)
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
          acc.a[k][v] += cr.a[k][v];
          if constexpr (CPLX) acc.b[k][v] += cr.b[k][v];
        }
    }
  }

  if (a.reg3 != 0.f) {
    float part = 0.f;
#pragma unroll
    for (int k = 0; k < NS; ++k) {
      float xa[VEC], xb[VEC];
      ldv<VEC>(es + (lane + 64 * k) * VEC, xa);
      if constexpr (CPLX) ldv<VEC>(es + QP + (lane + 64 * k) * VEC, xb);
#pragma unroll
      for (int v = 0; v < VEC; ++v) {
        acc.a[k][v] += a.reg3 * (xa[v] * fabsf(xa[v]));
        part += fabsf(xa[v]) * xa[v] * xa[v];
        if constexpr (CPLX) {
          acc.b[k][v] += a.reg3 * (xb[v] * fabsf(xb[v]));
          part += fabsf(xb[v]) * xb[v] * xb[v];
        }
      }
    }
    part = wave_sum(part);
    if (lane == 0) a.reg_partial[e] = part;
  }
  if (a.write_grad) store_row<NS, VEC, CPLX>(a.grad_ent + e * a.Le, a.eg, lane, acc);
  if constexpr (OPT != OPT_ADAM) {
    if (!a.adam.p) return;
    const float lr = a.adam.step_size, eps = a.adamk.eps;
    float std_row = 0.f;
    if constexpr (OPT == OPT_ADAGRAD_ROW) {
      float part = 0.f;
#pragma unroll
      for (int k = 0; k < NS; ++k) {
        if (lane + 64 * k >= a.eg.S) continue;  // (a slot past the row's end)
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
          part += acc.a[k][v] * acc.a[k][v];
          if constexpr (CPLX) part += acc.b[k][v] * acc.b[k][v];
        }
      }
      part = wave_sum(part);
      const float G = a.adam.m[e] + part / (float)a.Le;
      if (lane == 0) a.adam.m[e] = G;
      std_row = sqrtf(G) + eps;
    }
#pragma unroll
    for (int k = 0; k < NS; ++k) {
      const int slot = lane + 64 * k;
      if (slot >= a.eg.S) continue;
#pragma unroll
      for (int h2 = 0; h2 < (CPLX ? 2 : 1); ++h2) {
        const int64_t off = e * a.Le + (h2 ? a.eg.half : 0) + slot * VEC;
        float sv[VEC], pv[VEC];
        if constexpr (OPT == OPT_ADAGRAD) ldv<VEC>(a.adam.m + off, sv);
        ldv<VEC>(es + (h2 ? QP : 0) + slot * VEC, pv);
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
          float g;
          if constexpr (CPLX) g = h2 ? acc.b[k][v] : acc.a[k][v];
          else g = acc.a[k][v];
          if constexpr (OPT == OPT_ADAGRAD) adagrad_elem(pv[v], g, sv[v], lr, eps);
          else pv[v] = adagrad_move(pv[v], g, std_row, lr);
        }
        stv<VEC>(a.adam.p + off, pv);
        if constexpr (OPT == OPT_ADAGRAD) stv<VEC>(a.adam.m + off, sv);
      }
    }
    return;
  }
  if (a.adam.p) {
    // fused dense Adam on this row (optimizer.step(), model.py:303)
#pragma unroll
    for (int k = 0; k < NS; ++k) {
      const int slot = lane + 64 * k;
      if (slot >= a.eg.S) continue;
#pragma unroll
      for (int h2 = 0; h2 < (CPLX ? 2 : 1); ++h2) {
        const int64_t off = e * a.Le + (h2 ? a.eg.half : 0) + slot * VEC;
        float mv[VEC], vv[VEC], pv[VEC];
        ldv<VEC>(a.adam.m + off, mv);
        ldv<VEC>(a.adam.v + off, vv);
        ldv<VEC>(es + (h2 ? QP : 0) + slot * VEC, pv);
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
          float g;
          if constexpr (CPLX) g = h2 ? acc.b[k][v] : acc.a[k][v];
          else g = acc.a[k][v];
          adam_elem(pv[v], g, mv[v], vv[v], a.adamk, a.adam.step_size, a.adam.bc2s);
        }
        stv<VEC>(a.adam.p + off, pv);
        stv<VEC>(a.adam.m + off, mv);
        stv<VEC>(a.adam.v + off, vv);
      }
    }
  }
}

// Column-sliced entity pass (VEC = 4 rows).  The gradient of every model is
// elementwise in the entity row, so the row can be cut into `nsl` column
// slices handled independently: block b works on slice b % nsl of entities
// 4·(b / nsl) .. +3.  Blocks are dealt to the 8 XCDs round-robin (b and b+8
// share one), so each XCD touches one column slice of the q buffer
// (B·Le·4 / nsl bytes) and keeps it in its own 4 MiB L2 instead of
// re-fetching random q rows from the fabric (the unsliced pass moved
// ≈2.1 GB/launch across L2 ↔ MALL/HBM).  Placement is a speed property
// only; the result does not depend on it.  Lane l owns slot slice·W + l
// (16 bytes; for complex rows the re and im slots of the same dims), so each
// occurrence is one 16-B (+16-B) load per lane with four rows in flight.
// Per element the arithmetic and the occurrence order are k_entity's, so the
// gradient and Adam update are bit-identical to it; only the regulariser's
// per-row partial sums are split per slice.
// streaming (non-temporal) float4 access for the once-touched Adam/gradient
// rows, so they do not push the q column slice out of the XCD's L2
__device__ __forceinline__ void ldv_nt(const float* __restrict__ p, float (&x)[4]) {
  const tf4 v = __builtin_nontemporal_load(reinterpret_cast<const tf4*>(p));
  x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
}
__device__ __forceinline__ void stv_nt(float* __restrict__ p, const float (&x)[4]) {
  __builtin_nontemporal_store(tf4{x[0], x[1], x[2], x[3]}, reinterpret_cast<tf4*>(p));
}

// QSL: q read from k_row's slice-major copy (2 KB contiguous per (slice,
// row)) instead of the row-major q buffer.  Measured and rejected (DESIGN §4,
// profiles/r03/entity/, profiles/r04/entity/): q slices by LDS-DMA, 2 / 6 / 8
// q rows in flight, the moments loaded after the occurrence loop,
// occurrence buckets filled by k_row in place of the CSR, wave-specialised
// gather / stream waves.
// LAZY: as in k_entity — the block's entity group addresses rows[] (same block
// → (slice, group) → XCD mapping, same leading blocks).
// OPT: OPT_ADAGRAD streams the element-wise state in the place of Adam's two
// moments (two arrays per row where Adam streams three) and its leading blocks
// apply the same rule to the relation rows and the modulus.  The row-wise kind
// needs a whole row's Σg², which no block of this kernel holds: it runs
// k_entity (plan_step).
template <int M, int MODE, bool QSL = false, bool LAZY = false, int OPT = OPT_ADAM>
__global__ __launch_bounds__(256) void k_entity_sl(EntArgs a) {
  static_assert(OPT == OPT_ADAM || OPT == OPT_ADAGRAD, "the sliced pass has no row-wise kind");
  constexpr bool CPLX = Traits<M>::cplx;
  using EL = Elem<M, MODE>;
  constexpr int VEC = 4;
  constexpr int PF = 4;  // q rows in flight per wave
  const int lane = threadIdx.x & 63;
  const int w = wave_id();
  const int nsl = a.nsl;
  // leading blocks (dispatched first, so they do not trail the entity blocks):
  // block 0 the loss finalisation when fused (it reads only the row pass's
  // outputs: one launch less, no gap before the next step), then the relation
  // pass (same launch, no stream join); padded to a multiple of 8 so entity
  // block b still runs on XCD b % 8 with its column slice in that XCD's L2
  const unsigned lead = ent_lead_blocks(a);
  if (blockIdx.x < lead) {
    if (a.fin_fused && blockIdx.x == 0) {
      __shared__ float fred[6 * 256];
      finalize_block<256, OPT>(a.fin, fred);
      return;
    }
    const int64_t rb = (int64_t)blockIdx.x - (a.fin_fused ? 1 : 0);
    const int64_t rr = rb * 4 + w;
    if (rb < a.rel_blocks && rr < a.rel.R) rel_row_chunks<4, false, OPT>(a.rel, rr, lane);
    return;
  }
  const unsigned bx = blockIdx.x - lead;
  const int slice = (int)(bx % (unsigned)nsl);
  int64_t e = a.e_begin + (int64_t)(bx / (unsigned)nsl) * 4 + w;
  if constexpr (LAZY) {
    const int64_t place = (int64_t)(bx / (unsigned)nsl) * 4 + w;
    if (place >= (int64_t)a.nrows[0]) return;
    e = a.rows[place];
  } else {
    if (e >= a.e_end) return;
  }
  // this slice's slots [s0, s1) of the (half-)row.  align_sl: the inner
  // boundaries sit on 128-B lines of the row's first half (64-slot slices
  // shifted by the row's 16-B phase sh), so no line of that half is shared by
  // the two XCDs of neighbouring slices; same per-element work either way
  int s0, s1;
  if (a.align_sl) {
    const int sh = (int)((reinterpret_cast<uintptr_t>(a.ent + e * a.Le) >> 4) & 7);
    s0 = slice == 0 ? 0 : slice * 64 - sh;
    s1 = slice == nsl - 1 ? a.eg.S : (slice + 1) * 64 - sh;
  } else {
    s0 = slice * a.slice_w;
    s1 = s0 + a.slice_w < a.eg.S ? s0 + a.slice_w : a.eg.S;
  }
  const int slot = s0 + lane;
  const bool act = slot < s1;
  const int so = act ? slot * VEC : 0;  // float offset inside the (half-)row
  Consts c = a.c;
  if constexpr (M == PROTATE) c.modulus = a.modulus[0];

  float ea[VEC], eb[VEC], acca[VEC], accb[VEC];
  zv<VEC>(ea);
  zv<VEC>(eb);
  zv<VEC>(acca);
  zv<VEC>(accb);
  const float* erow = a.ent + e * a.Le;
  if (act) {
    ldv_nt(erow + so, ea);
    if constexpr (CPLX) ldv_nt(erow + a.eg.half + so, eb);
  }
  // the Adam moments do not depend on the occurrence loop: issue their loads
  // now so they are in flight behind it
  constexpr int H2 = CPLX ? 2 : 1;
  float mv[H2][VEC], vv[H2][VEC];
  if (a.adam.p && act) {
#pragma unroll
    for (int h2 = 0; h2 < H2; ++h2) {
      const int64_t off = e * a.Le + (h2 ? a.eg.half : 0) + so;
      ldv_nt(a.adam.m + off, mv[h2]);
      if constexpr (OPT == OPT_ADAM) ldv_nt(a.adam.v + off, vv[h2]);
    }
  }
  auto ld_slot = [&](const float* row, float (&x)[VEC], float (&y)[VEC]) {
    if (act) {
      ldv<VEC>(row + so, x);
      if constexpr (CPLX) ldv<VEC>(row + a.eg.half + so, y);
    }
  };
  auto accumulate = [&](const float (&qa)[VEC], const float (&qb)[VEC], float g) {
    if constexpr (M == ROTATE) {
      // Elem<ROTATE>::grads on adjacent dims (v, v+1) as register pairs:
      // v_pk_{add,mul}_f32 for the same per-element operations, so the sums
      // are bit-identical to the scalar form below
#pragma unroll
      for (int v = 0; v < VEC; v += 2) {
        const tf2 dr = tf2{qa[v], qa[v + 1]} - tf2{ea[v], ea[v + 1]};
        const tf2 di = tf2{qb[v], qb[v + 1]} - tf2{eb[v], eb[v + 1]};
        const tf2 s2 = dr * dr + di * di;
        const tf2 inv = tf2{(s2.x > 0.f) ? frsq(s2.x) : 0.f, (s2.y > 0.f) ? frsq(s2.y) : 0.f};
        const tf2 gg = tf2{g, g};
        const tf2 ar = tf2{acca[v], acca[v + 1]} + gg * (dr * inv);
        const tf2 ai = tf2{accb[v], accb[v + 1]} + gg * (di * inv);
        acca[v] = ar.x; acca[v + 1] = ar.y;
        accb[v] = ai.x; accb[v + 1] = ai.y;
      }
      return;
    }
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
      float gqa, gqb, gea, geb;
      if constexpr (CPLX) {
        EL::grads(qa[v], qb[v], ea[v], eb[v], c, gqa, gqb, gea, geb);
        accb[v] += g * geb;
      } else {
        EL::grads(qa[v], 0.f, ea[v], 0.f, c, gqa, gqb, gea, geb);
      }
      acca[v] += g * gea;
    }
  };

  const uint32_t n32 = (uint32_t)a.n;
  // the entity's occurrences from its CSR bucket in chunks of ≤ 64, ascending
  // ids in lanes 0 .. cnt-1 (so a chunk's negatives come first)
  int32_t c0 = a.off[e];
  const int32_t b1 = a.off[e + 1];
  while (c0 < b1) {
    const int cnt = (b1 - c0 < 64) ? (b1 - c0) : 64;
    const int32_t o_l = (lane < cnt) ? a.occ[c0 + lane] : 0x7fffffff;
    c0 += 64;
    const bool neg_l = o_l < a.Bn;
    const uint32_t i_l = neg_l ? ((uint32_t)o_l / n32) : 0u;
    const float g_l = neg_l ? a.g[o_l] : 0.f;
    const int nneg = __popcll(__ballot(neg_l && lane < cnt));  // negatives first (ids ascend)
    // QSL: q from k_row's slice-major copy, 2 KB contiguous per (slice, row)
    auto ld_q = [&](int p, float (&x)[VEC], float (&y)[VEC]) {
      const uint32_t ip = (uint32_t)__builtin_amdgcn_readlane((int)i_l, p);
      if constexpr (QSL) {
        const float* base = a.q_sl + (((int64_t)slice * a.B + ip) * 2) * 256 + lane * 4;
        if (act) {
          ldv<VEC>(base, x);
          if constexpr (CPLX) ldv<VEC>(base + 256, y);
        }
      } else {
        ld_slot(a.q + (int64_t)ip * a.Le, x, y);
      }
    };
    float qa[PF][VEC], qb[PF][VEC];
#pragma unroll
    for (int u = 0; u < PF; ++u) {
      zv<VEC>(qa[u]);
      zv<VEC>(qb[u]);
      if (u < nneg) ld_q(u, qa[u], qb[u]);
    }
    for (int p = 0; p < nneg; p += PF) {
#pragma unroll
      for (int u = 0; u < PF; ++u) {
        if (p + u < nneg) {
          accumulate(qa[u], qb[u], readlanef(g_l, p + u));
          if (p + u + PF < nneg) ld_q(p + u + PF, qa[u], qb[u]);
        }
      }
    }
    for (int p = nneg; p < cnt; ++p) {
      const int32_t o = __builtin_amdgcn_readlane(o_l, p);
      float ca[VEC], cb[VEC];
      zv<VEC>(ca);
      zv<VEC>(cb);
      ld_slot(a.ent_contrib + (int64_t)(o - a.Bn) * a.Le, ca, cb);
#pragma unroll
      for (int v = 0; v < VEC; ++v) {
        acca[v] += ca[v];
        if constexpr (CPLX) accb[v] += cb[v];
      }
    }
  }

  if (a.reg3 != 0.f) {
    float part = 0.f;
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
      acca[v] += a.reg3 * (ea[v] * fabsf(ea[v]));
      part += fabsf(ea[v]) * ea[v] * ea[v];
      if constexpr (CPLX) {
        accb[v] += a.reg3 * (eb[v] * fabsf(eb[v]));
        part += fabsf(eb[v]) * eb[v] * eb[v];
      }
    }
    part = wave_sum(part);
    if (lane == 0) a.reg_partial[e * nsl + slice] = part;
  }
  // the gradient write and the Adam update of this wave's slice
  if (!act) return;
  if (a.write_grad) {
    stv_nt(a.grad_ent + e * a.Le + so, acca);
    if constexpr (CPLX) stv_nt(a.grad_ent + e * a.Le + a.eg.half + so, accb);
  }
  if (a.adam.p) {
#pragma unroll
    for (int h2 = 0; h2 < H2; ++h2) {
      const int64_t off = e * a.Le + (h2 ? a.eg.half : 0) + so;
      float pv[VEC];
#pragma unroll
      for (int v = 0; v < VEC; ++v) {
        pv[v] = h2 ? eb[v] : ea[v];
        if constexpr (OPT == OPT_ADAM)
          adam_elem(pv[v], h2 ? accb[v] : acca[v], mv[h2][v], vv[h2][v], a.adamk, a.adam.step_size, a.adam.bc2s);
        else
          adagrad_elem(pv[v], h2 ? accb[v] : acca[v], mv[h2][v], a.adam.step_size, a.adamk.eps);
      }
      stv_nt(a.adam.p + off, pv);
      stv_nt(a.adam.m + off, mv[h2]);
      if constexpr (OPT == OPT_ADAM) stv_nt(a.adam.v + off, vv[h2]);
    }
  }
}

// One launch for one direction (MODE) or both (BOTH_DIRS): the grid is then
// two halves of gridDim.x / 2 blocks, head-batch's then tail-batch's, each
// block wholly in one direction; query j of direction d is qi = d·nq + j in
// the per-query arrays (RefArgs' pointers are direction 0's) and row j of
// the shared queries[nq, 3].
template <int MODE>
__device__ __forceinline__ int ref_dir(int64_t& bx) {
  if constexpr (MODE != BOTH_DIRS) {
    bx = blockIdx.x;
    return MODE;
  } else {
    const int64_t gd = gridDim.x / 2;
    const bool tail = (int64_t)blockIdx.x >= gd;
    bx = (int64_t)blockIdx.x - (tail ? gd : 0);
    return tail ? TAIL_BATCH : HEAD_BATCH;
  }
}

// ------------------------------------------------------------- ranking
// q vector and the true candidate's score for each query (one wave each).
// (qi: the query's index in the per-query arrays, qrow: its row of queries)
template <int M, int MODE, int VEC, int NS>
__device__ __forceinline__ void rank_prep_body(const RankArgs& a, int64_t qi, int64_t qrow) {
  constexpr bool CPLX = Traits<M>::cplx;
  using R_ = Row<NS, VEC, CPLX>;
  const int lane = threadIdx.x & 63;
  if (a.zero_counts && lane < 6) a.gt[lane * a.cstride + qi] = 0;  // gt, eq, gtx, eqx, ucnt, done of this query
  Consts c = a.c;
  if constexpr (M == PROTATE) c.modulus = a.modulus[0];
  const int64_t h = a.queries[qrow * 3], r = a.queries[qrow * 3 + 1], t = a.queries[qrow * 3 + 2];
  const int64_t x = (MODE == HEAD_BATCH) ? t : h;
  const int64_t ev = (MODE == HEAD_BATCH) ? h : t;
  if (h < 0 || h >= a.E || t < 0 || t >= a.E || r < 0 || r >= a.R) {
    if (lane == 0) {
      atomicOr(a.err, KGE_DEVERR_INDEX);
      a.s_true[qi] = NAN;
      a.true_id[qi] = -1;
    }
    return;
  }
  R_ q, er;
  {
    R_ xr, rr;
    load_row<NS, VEC, CPLX>(a.ent + x * a.Le, a.eg, lane, xr);
    if constexpr (M == ROTATE) {
      if (a.trig) {  // the caller's reference cos | sin row: q equals k_rank_window's reference q bit for bit
        const float* tr = a.trig + r * 2 * a.Lr;
        load_phase<NS, VEC>(tr, a.eg.S, lane, rr.a);
        load_phase<NS, VEC>(tr + a.Lr, a.eg.S, lane, rr.b);
#pragma unroll
        for (int s = 0; s < NS; ++s)
#pragma unroll
          for (int v = 0; v < VEC; ++v)
            Elem<M, MODE>::rotate(xr.a[s][v], xr.b[s][v], rr.a[s][v], rr.b[s][v], q.a[s][v], q.b[s][v]);
      } else {
        load_rel<M, NS, VEC, CPLX>(a.rel + r * a.Lr, a.eg, lane, rr);
        build_q<M, MODE, NS, VEC, CPLX>(xr, rr, c, q);
      }
    } else {
      load_rel<M, NS, VEC, CPLX>(a.rel + r * a.Lr, a.eg, lane, rr);
      build_q<M, MODE, NS, VEC, CPLX>(xr, rr, c, q);
    }
  }
  store_row<NS, VEC, CPLX>(a.q + qi * a.Le, a.eg, lane, q);
  load_row<NS, VEC, CPLX>(a.ent + ev * a.Le, a.eg, lane, er);
  const float tot = wave_sum(lane_total<M, MODE, NS, VEC, CPLX>(q, er, c));
  if (lane == 0) {
    a.s_true[qi] = Elem<M, MODE>::finish(tot, c);
    a.true_id[qi] = ev;
  }
}

// one direction (MODE), or both (BOTH_DIRS: the grid's second half is
// tail-batch's, query j at qi = nq + j, as the refinement launches)
template <int M, int MODE, int VEC, int NS>
__global__ __launch_bounds__(256) void k_rank_prep(RankArgs a) {
  int64_t bx;
  const int md = ref_dir<MODE>(bx);
  const int64_t j = bx * 4 + wave_id();
  if (j >= a.nq) return;
  const int64_t qi = (md == TAIL_BATCH && MODE == BOTH_DIRS) ? a.nq + j : j;
  if constexpr (MODE == BOTH_DIRS) {
    if (md == HEAD_BATCH) rank_prep_body<M, HEAD_BATCH, VEC, NS>(a, qi, j);
    else rank_prep_body<M, TAIL_BATCH, VEC, NS>(a, qi, j);
  } else {
    rank_prep_body<M, MODE, VEC, NS>(a, qi, j);
  }
}

// Wave-scan counting pass (any model; the fallback when rows are not float4
// staged): candidates scoring above the true one by more than the query's
// window are counted, those within it listed for the refinement
// (k_rank_refine); excluded candidates (filtered ids, the true id) come from
// the bitmap.  Work unit = (query, candidate chunk), one wave each; counts are
// integers, so the atomics keep the result exact and order-independent.
template <int M, int MODE, int VEC, int NS>
__global__ __launch_bounds__(256) void k_rank_scan(RankArgs a) {
  constexpr bool CPLX = Traits<M>::cplx;
  using R_ = Row<NS, VEC, CPLX>;
  const int lane = threadIdx.x & 63;
  const int64_t unit = (int64_t)blockIdx.x * 4 + wave_id();
  const int64_t chunks = (a.E + a.cpw - 1) / a.cpw;
  if (unit >= a.nq * chunks) return;
  const int64_t qi = unit / chunks;
  const int64_t c0 = (unit - qi * chunks) * a.cpw;
  const int64_t c1 = (c0 + a.cpw < a.E) ? (c0 + a.cpw) : a.E;
  if (a.true_id[qi] < 0) return;
  Consts c = a.c;
  if constexpr (M == PROTATE) c.modulus = a.modulus[0];
  const float st = a.s_true[qi], dlt = a.win.delta[qi];
  const uint32_t* bits = a.fbits + qi * a.W;
  R_ q;
  load_row<NS, VEC, CPLX>(a.q + qi * a.Le, a.eg, lane, q);
  int gt = 0;
  for (int64_t e = c0; e < c1; ++e) {
    if (filter_bit(bits, e)) continue;  // wave-uniform
    R_ r0;
    load_row<NS, VEC, CPLX>(a.ent + e * a.Le, a.eg, lane, r0);
    const float s0 = Elem<M, MODE>::finish(wave_sum(lane_total<M, MODE, NS, VEC, CPLX>(q, r0, c)), c);
    if (lane == 0) win_count(a.win, qi, e, s0, st, dlt, gt);
  }
  if (lane == 0 && gt) atomicAdd(&a.gt[qi], gt);
}

// ------------------------------------------------------- tiled ranking
// Filtered ranking as a register-tiled VALU "GEMM" with the model's phi in
// place of the multiply (the distance models have no matrix-core form):
// 64 queries × 64 candidates per workgroup, each thread a 4 × 4 block of
// pairs, reduction slabs of 16 elements staged through LDS as [k][row] and
// prefetched one slab ahead in registers.  Every pair sums its terms in
// ascending k with no cross-lane step, so the gather pass (B rows = the
// queries' true entities, diagonal kept) and the scan pass produce identical
// bits for the true candidate.  Counting: strictly greater / equal versus
// s_true beyond the query's window (win_count), skipping the filtered ids and
// the true id (bitmap); near-ties are listed for k_rank_refine.
constexpr int TILE_RQ = 64, TILE_BK = 16;

// One reduction element k of the 4 × 4 pair block, written in packed form so
// the compiler issues v_pk_{add,mul}_f32 on register pairs with no operand
// shuffles.  acc[i][h] holds the sums of pairs (i, 2h) and (i, 2h+1).
// Complex rows are staged as interleaved (re, im) pairs; real rows as plain
// floats.  The per-pair arithmetic is Elem::phi's, in the same order.
template <int M, int MODE>
struct TileMath {
  static constexpr bool HEAD = (MODE == HEAD_BATCH);
  // complex: q, e = 4 (re, im) pairs each
  __device__ static __forceinline__ void cplx(const tf2 (&q)[4], const tf2 (&e)[4], tf2 (&acc)[4][2]) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        float r[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          const tf2 ej = e[2 * h + u];
          if constexpr (M == ROTATE) {           // model.py:217-226
            const tf2 d = q[i] - ej;
            const tf2 d2 = d * d;
            r[u] = fsqrt(d2.x + d2.y);
          } else {                               // COMPLEX, model.py:192,196
            const tf2 p = HEAD ? (ej * q[i]) : (q[i] * ej);
            r[u] = p.x + p.y;
          }
        }
        acc[i][h] += tf2{r[0], r[1]};
      }
  }
  // RotatE with the candidates staged as four re then four im values (so
  // (re_j, re_j+1) and (im_j, im_j+1) are register pairs) and q broadcast by
  // op_sel: per two candidates v_pk_add ×2 (q − e, re and im), v_pk_mul (im²),
  // v_pk_fma (re² + im²), two v_sqrt and a v_pk_add — 18 issue cycles per
  // pair-element where the (re, im)-pair form takes 22 (a v_pk_mul and a
  // v_add per candidate).  The fma rounds re² + im² once instead of twice;
  // the window's per-element term (k_rank_window: ≤ 3u of each modulus for
  // the fast elements) covers either.
  __device__ static __forceinline__ void rot(const tf2 (&q)[4], const float4& er, const float4& ei,
                                             tf2 (&acc)[4][2]) {
    const tf2 R[2] = {tf2{er.x, er.y}, tf2{er.z, er.w}};
    const tf2 I[2] = {tf2{ei.x, ei.y}, tf2{ei.z, ei.w}};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const tf2 qr = tf2{q[i].x, q[i].x}, qi = tf2{q[i].y, q[i].y};
      // both candidate pairs stage by stage, so no packed result feeds the
      // next instruction directly (each such pair costs an s_nop)
      const tf2 dx0 = qr - R[0], dx1 = qr - R[1];
      const tf2 dy0 = qi - I[0], dy1 = qi - I[1];
      const tf2 y0 = dy0 * dy0, y1 = dy1 * dy1;
      const tf2 s0 = __builtin_elementwise_fma(dx0, dx0, y0), s1 = __builtin_elementwise_fma(dx1, dx1, y1);
      acc[i][0] += tf2{fsqrt(s0.x), fsqrt(s0.y)};
      acc[i][1] += tf2{fsqrt(s1.x), fsqrt(s1.y)};
    }
  }
  // real: q, e = 4 floats each
  __device__ static __forceinline__ void real(const float4& q4, const float4& e4, tf2 (&acc)[4][2], const Consts& c) {
    const float q[4] = {q4.x, q4.y, q4.z, q4.w};
    const tf2 e[2] = {tf2{e4.x, e4.y}, tf2{e4.z, e4.w}};
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const tf2 qq = tf2{q[i], q[i]};
        if constexpr (M == TRANSE) {             // model.py:168-172
          const tf2 d = HEAD ? (e[h] + qq) : (qq - e[h]);
          // acc += |d| as v_add_f32 with the |·| source modifier (same
          // rounding; the compiler's form is two v_and_b32 + v_pk_add_f32)
          float ax = acc[i][h].x, ay = acc[i][h].y;
          asm("v_add_f32_e64 %0, %1, |%2|" : "=v"(ax) : "v"(ax), "v"(d.x));
          asm("v_add_f32_e64 %0, %1, |%2|" : "=v"(ay) : "v"(ay), "v"(d.y));
          acc[i][h] = tf2{ax, ay};
        } else if constexpr (M == DISTMULT) {    // model.py:177-181
          acc[i][h] += HEAD ? (e[h] * qq) : (qq * e[h]);
        }
      }
  }
  // pRotatE (model.py:238-248) by the angle-difference identity: q staged as
  // (sin q, cos q) pairs, a thread's four candidates as their cos then their
  // sin values (c0 c1 c2 c3 | s0 s1 s2 s3: (c_j, c_j+1) and (s_j, s_j+1) are
  // register pairs), from launch_prot_phase's tables:
  //   tail  sin(q − e) = sin q·cos e − cos q·sin e
  //   head  sin(e + q) = sin q·cos e + cos q·sin e
  // per two candidates one v_pk_mul_f32 (sin q splat) and one v_pk_fma_f32
  // (cos q splat, negated for tail), then two adds with |·| as a source
  // modifier — 4 VALU instructions per 2 pair-elements where the interleaved
  // (cos, sin) pairs took 9 (operand shuffles, v_and for |·|, v_pk_add).  The fma rounds
  // once where the multiply-subtract rounded twice; the window's per-element
  // term (k_rank_window, 32·K·u·mod) covers either.
  // TransE with the queries staged as (q, q) pairs: qv[0] = (q0, q0, q1, q1),
  // qv[1] = (q2, q2, q3, q3); the differences first, then the |·| adds
  __device__ static __forceinline__ void transe_spl(const float4 (&qv)[2], const float4& e4, tf2 (&acc)[4][2]) {
    const tf2 e[2] = {tf2{e4.x, e4.y}, tf2{e4.z, e4.w}};
    const tf2 qq[4] = {tf2{qv[0].x, qv[0].y}, tf2{qv[0].z, qv[0].w}, tf2{qv[1].x, qv[1].y}, tf2{qv[1].z, qv[1].w}};
    tf2 d[4][2];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int h = 0; h < 2; ++h) d[i][h] = HEAD ? (e[h] + qq[i]) : (qq[i] - e[h]);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        float ax = acc[i][h].x, ay = acc[i][h].y;
        asm("v_add_f32_e64 %0, %1, |%2|" : "=v"(ax) : "v"(ax), "v"(d[i][h].x));
        asm("v_add_f32_e64 %0, %1, |%2|" : "=v"(ay) : "v"(ay), "v"(d[i][h].y));
        acc[i][h] = tf2{ax, ay};
      }
  }
  // (round 6) the query's sin and cos are splatted by the packed ops' own
  // operand selects — v_pk_mul_f32 (sin q)·C with op_sel_hi:[0,1] reads the
  // pair's low half in both lanes, v_pk_fma_f32 ±(cos q)·S + m with
  // op_sel:[1,0,0] its high half (neg_lo / neg_hi: tail-batch's −cos) — where
  // hipcc materialised the splat with a v_mov for half the queries; all
  // products, then all fmas, then the adds, so no instruction reads the one
  // just before it (the compiler put an s_nop in front of each such read).
  // The same products, fmas and adds in the same order: the same bits.
  __device__ static __forceinline__ void prot(const tf2 (&q)[4], const float4& ec, const float4& es,
                                              tf2 (&acc)[4][2]) {
    const tf2 C[2] = {tf2{ec.x, ec.y}, tf2{ec.z, ec.w}};
    const tf2 S[2] = {tf2{es.x, es.y}, tf2{es.z, es.w}};
    tf2 m[4][2], r[4][2];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int h = 0; h < 2; ++h) asm("v_pk_mul_f32 %0, %1, %2 op_sel_hi:[0,1]" : "=v"(m[i][h]) : "v"(q[i]), "v"(C[h]));
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        if constexpr (HEAD)
          asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[1,0,0]" : "=v"(r[i][h]) : "v"(q[i]), "v"(S[h]), "v"(m[i][h]));
        else
          asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[1,0,0] neg_lo:[1,0,0] neg_hi:[1,0,0]"
              : "=v"(r[i][h]) : "v"(q[i]), "v"(S[h]), "v"(m[i][h]));
      }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        // acc += |r| as v_add_f32 with the |·| source modifier (the compiler
        // packs fabsf + add into two v_and_b32 and a v_pk_add_f32)
        float ax = acc[i][h].x, ay = acc[i][h].y;
        asm("v_add_f32_e64 %0, %1, |%2|" : "=v"(ax) : "v"(ax), "v"(r[i][h].x));
        asm("v_add_f32_e64 %0, %1, |%2|" : "=v"(ay) : "v"(ay), "v"(r[i][h].y));
        acc[i][h] = tf2{ax, ay};
      }
  }
};

// The staging geometry of one 64 × 64 tile (k_rank_tile, k_topk_tile).  The
// reduction loop itself is one text, kge_tile_reduce.inc, included in
// k_rank_tile's body and in tile_reduce, which k_topk_tile calls: a textual
// fragment, so both kernels keep the instructions they were measured with.
// k_rank_tile calling tile_reduce instead costs VGPRs (as it stands RotatE
// 70 → 74, one wave per SIMD less); with the arguments by value and the staging
// buffers the function's own it stayed within the allocation step (72 / 72 /
// 78 / 50 / 72 VGPRs for 70 / 70 / 76 / 49 / 72) and ranked as fast, but that
// form changed k_topk_tile, which then measured slower at k = 10 (DESIGN.md
// §5b).
template <int M, bool SPLT>
struct TileCfg {
  static constexpr bool CPLX = Traits<M>::cplx;
  static constexpr bool PROT = (M == PROTATE);
  static constexpr int P = CPLX ? 2 : 1;             // float4 loads per staged slot
  static constexpr int PS = (CPLX || PROT) ? 2 : 1;  // floats staged per element
  static constexpr int T = TILE_RQ, BK = TILE_BK;
  // SPL (TransE): the queries are staged pre-splatted, [k][row][q, q], so
  // each packed operand of the inner loop is a plain register pair (no op_sel
  // splat, which hipcc materialised with a v_mov for half the pairs).
  // pRotatE staged the same way, [k][row][sin, sin, cos, cos],
  // measured slower (whole evaluation 12.89-13.14 vs 12.61-12.68 ms, same box:
  // twice the query LDS, fewer waves) and keeps the (sin, cos) pairs.
  static constexpr bool SPL = SPLT && (M == TRANSE);
  static constexpr int QW = SPL ? 2 : PS;  // floats per query per k-row of Qs
  // TransE (SPL) and pRotatE: k-rows padded by 4 floats, so a 16-lane
  // group's staging stores (4 rows × 4 k-offsets) fall on 16 different banks;
  // unpadded, the k-offsets' rows are 128 or 64 floats apart, a multiple of
  // the bank count (4-way conflicts).  pRotatE's tile: SQ_LDS_BANK_CONFLICT
  // 4.0e8 → 1.4e8 cycles per wn18rr direction, evaluation 12.8-13.1 →
  // 11.8 ms (`profiles/r06/rank/`).  RotatE measured slower padded (FB15k
  // 24.4-24.5 → 25.9-26.5 ms) and stays unpadded, as do ComplEx and DistMult.
  static constexpr int PAD = (SPL || PROT) ? 4 : 0;
  static constexpr int QSTR = T * QW + PAD, ESTR = T * PS + PAD;
};

// One 64 × 64 tile's reduction as a function (k_topk_tile): kge_tile_reduce.inc.
template <int M, int MODE, bool GATHER, bool SPLT>
__device__ __forceinline__ void tile_reduce(const TileArgs& a, const Consts& c, int64_t q0, int64_t e0,
                                            const int64_t* arow, const int64_t* brow,
                                            float (&Qs)[TILE_BK][TileCfg<M, SPLT>::QSTR],
                                            float (&Es)[TILE_BK][TileCfg<M, SPLT>::ESTR], tf2 (&acc)[4][2]) {
  using C_ = TileCfg<M, SPLT>;
  constexpr int T = C_::T, BK = C_::BK;
  const int t = threadIdx.x;
  const int ty = t >> 4, tx = t & 15;
#include "kge_tile_reduce.inc"
}

template <int M, int MODE, bool GATHER, bool SPLT = true>
__global__ __launch_bounds__(256) void k_rank_tile(TileArgs a) {
  using C_ = TileCfg<M, SPLT>;
  constexpr int T = C_::T, BK = C_::BK;
  // Qs: [k][row] (real), [k][row][re, im] (complex), or TileCfg's SPL form.
  // Es: [k][row] (real); complex and pRotatE rows in two halves
  // of a k-row, [k][half][row / 4][4] — RotatE: re | im, pRotatE: cos | sin,
  // ComplEx: candidates 4c, 4c+1 | 4c+2, 4c+3 as (re, im) pairs — so the 16
  // candidate columns of a ds_read_b128 lane group are 16 consecutive 16-B
  // slots (every bank once) where [row][8] put columns c and c + 8 on one bank
  __shared__ __attribute__((aligned(16))) float Qs[BK][C_::QSTR];
  __shared__ __attribute__((aligned(16))) float Es[BK][C_::ESTR];
  __shared__ int64_t arow[T], brow[T], tids[T];
  __shared__ float sts[T], sdl[T];
  __shared__ int32_t cnt[T];  // strictly greater beyond the window (≤ 64 per block)
  const int t = threadIdx.x;
  const int ty = t >> 4, tx = t & 15;
  const int64_t q0 = (int64_t)blockIdx.y * T;
  const int64_t e0 = (int64_t)blockIdx.x * T;
  Consts c = a.c;
  if constexpr (M == PROTATE) c.modulus = a.modulus[0];
  if (t < T) {
    const int64_t q = q0 + t;
    arow[t] = (q < a.nq) ? q : -1;
    const int64_t tid_ = (q < a.nq) ? a.true_id[q] : -1;
    tids[t] = tid_;
    if (GATHER) {
      brow[t] = (tid_ >= 0 && tid_ < a.E) ? tid_ : -1;
    } else {
      const int64_t e = e0 + t;
      brow[t] = (e < a.E) ? e : -1;
      sts[t] = (q < a.nq) ? a.s_true[q] : 0.f;
      sdl[t] = (q < a.nq) ? a.win.delta[q] : 0.f;
    }
    cnt[t] = 0;
  }
  __syncthreads();

  tf2 acc[4][2];
#include "kge_tile_reduce.inc"
  auto pair_total = [&](int i, int j) -> float { return (j & 1) ? acc[i][j >> 1].y : acc[i][j >> 1].x; };

  if (GATHER) {
    if (ty != tx) return;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int m = ty * 4 + i;
      if (arow[m] >= 0 && brow[m] >= 0) a.s_true[q0 + m] = Elem<M, MODE>::finish(pair_total(i, i), c);
    }
    return;
  }
  const int64_t eb0 = e0 + tx * 4;  // four candidates in one bitmap word
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int m = ty * 4 + i;
    const int64_t q = arow[m];
    if (q < 0 || eb0 >= a.E) continue;
    const uint32_t word = a.fbits[q * a.W + (eb0 >> 5)];
    const float st = sts[m], dlt = sdl[m];
    const int64_t tid_ = tids[m];
    int g = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int64_t e = eb0 + j;
      const bool ok = (e < a.E) && (e != tid_) && (((word >> (e & 31)) & 1u) == 0u);
      const float s = Elem<M, MODE>::finish(pair_total(i, j), c);
      if (ok) win_count(a.win, q, e, s, st, dlt, g);
    }
    if (g) atomicAdd(&cnt[m], g);
  }
  __syncthreads();
  if (t < T && arow[t] >= 0 && cnt[t]) atomicAdd(&a.gt[q0 + t], cnt[t]);
}

template <int M>
int launch_rank_tile(int mode, int gather, const TileArgs& a, hipStream_t s) {
  const unsigned gy = (unsigned)((a.nq + TILE_RQ - 1) / TILE_RQ);
  const unsigned gx = gather ? 1u : (unsigned)((a.E + TILE_RQ - 1) / TILE_RQ);
  // KGE_TILE_SPL=0 (diagnostic, same bits): TransE with round 5's staging
  // (op_sel splats, unpadded k-rows, unroll-4 k loop)
  const bool spl = !(M == TRANSE && env_flag_off("KGE_TILE_SPL"));
  auto go = [&](auto kh, auto kt) {
    hipLaunchKernelGGL(pick_dir(mode, kh, kt), dim3(gx, gy), dim3(256), 0, s, a);
    return (int)hipGetLastError();
  };
  if (gather)
    return spl ? go(k_rank_tile<M, HEAD_BATCH, true>, k_rank_tile<M, TAIL_BATCH, true>)
               : go(k_rank_tile<M, HEAD_BATCH, true, false>, k_rank_tile<M, TAIL_BATCH, true, false>);
  return spl ? go(k_rank_tile<M, HEAD_BATCH, false>, k_rank_tile<M, TAIL_BATCH, false>)
             : go(k_rank_tile<M, HEAD_BATCH, false, false>, k_rank_tile<M, TAIL_BATCH, false, false>);
}

// ------------------------------------------------------- top-k prediction
// kge_topk: each (query, candidate part) keeps the k best unexcluded
// candidates of its part as a list sorted by (score descending, id ascending)
// in LDS, owned by one wave; k_topk_merge (kge_common.hip) reduces a query's
// parts.  Unused places hold (−∞, TOPK_NO_ID), so a list is always "full" and
// its last place is the threshold a new candidate has to beat.

// One wave inserts (s, e) into its sorted k-list (k ≤ 128: places lane and
// lane + 64) and returns the new threshold.  Wave-uniform arguments; LDS
// operations of one wave execute in order, so the moved entries are read
// before any place is overwritten.
__device__ __forceinline__ float topk_insert(volatile float* ls, volatile int32_t* li, int k, float s, int32_t e,
                                             int lane) {
  const int p0 = lane, p1 = lane + 64;
  const bool in0 = p0 < k, in1 = p1 < k;
  const float s0 = in0 ? ls[p0] : 0.f, s1 = in1 ? ls[p1] : 0.f;
  const int32_t i0 = in0 ? li[p0] : 0, i1 = in1 ? li[p1] : 0;
  // the places that stay ahead of the new entry (a prefix: the list is sorted)
  const bool a0 = in0 && (s0 > s || (s0 == s && i0 < e));
  const bool a1 = in1 && (s1 > s || (s1 == s && i1 < e));
  const int pos = __popcll(__ballot(a0)) + __popcll(__ballot(a1));
  if (pos < k) {
    const bool w0 = in0 && p0 > pos, w1 = in1 && p1 > pos;
    const float m0 = w0 ? ls[p0 - 1] : 0.f, m1 = w1 ? ls[p1 - 1] : 0.f;
    const int32_t j0 = w0 ? li[p0 - 1] : 0, j1 = w1 ? li[p1 - 1] : 0;
    __builtin_amdgcn_wave_barrier();
    if (w0) { ls[p0] = m0; li[p0] = j0; }
    if (w1) { ls[p1] = m1; li[p1] = j1; }
    if (p0 == pos) { ls[p0] = s; li[p0] = e; }
    if (p1 == pos) { ls[p1] = s; li[p1] = e; }
    __builtin_amdgcn_wave_barrier();
  }
  return ls[k - 1];
}

// a wave writes one list to its place of the partial lists
__device__ __forceinline__ void topk_store(const TopkArgs& a, int64_t q, int part, const volatile float* ls,
                                           const volatile int32_t* li, int lane) {
  const int64_t dst = (q * a.parts + part) * a.k;
  for (int p = lane; p < a.k; p += 64) {
    a.pscore[dst + p] = ls[p];
    a.pid[dst + p] = li[p];
  }
}

// q of every query (one wave each), as k_rank_prep builds it with device
// cos / sin, without the true entity: the predicted column is neither read for
// a row nor range-checked.  A query whose other two ids are out of range sets
// KGE_DEVERR_INDEX and is marked TOPK_BAD.
template <int M, int MODE, int VEC, int NS>
__global__ __launch_bounds__(256) void k_topk_prep(TopkArgs a) {
  constexpr bool CPLX = Traits<M>::cplx;
  using R_ = Row<NS, VEC, CPLX>;
  const int lane = threadIdx.x & 63;
  const int64_t qi = (int64_t)blockIdx.x * 4 + wave_id();
  if (qi >= a.nq) return;
  Consts c = a.c;
  if constexpr (M == PROTATE) c.modulus = a.modulus[0];
  const int64_t h = a.queries[qi * 3], r = a.queries[qi * 3 + 1], t = a.queries[qi * 3 + 2];
  const int64_t x = (MODE == HEAD_BATCH) ? t : h;
  const bool bad = x < 0 || x >= a.E || r < 0 || r >= a.R;
  if (lane == 0) {
    a.qsan[qi * 3] = (MODE == HEAD_BATCH) ? 0 : h;
    a.qsan[qi * 3 + 1] = r;
    a.qsan[qi * 3 + 2] = (MODE == HEAD_BATCH) ? t : 0;
    a.state[qi] = bad ? TOPK_BAD : TOPK_VALID;
    if (bad) atomicOr(a.err, KGE_DEVERR_INDEX);
  }
  if (bad) return;
  R_ q, xr, rr;
  load_row<NS, VEC, CPLX>(a.ent + x * a.Le, a.eg, lane, xr);
  load_rel<M, NS, VEC, CPLX>(a.rel + r * a.Lr, a.eg, lane, rr);
  build_q<M, MODE, NS, VEC, CPLX>(xr, rr, c, q);
  store_row<NS, VEC, CPLX>(a.q + qi * a.Le, a.eg, lane, q);
}

// kge_topk_shard's prep: k_topk_prep with the fixed side's row taken from
// fixed_rows[qi] (KGE_RSHARD_ROWS, reduced) and not from a table — the same
// load_row / build_q on the same bits, so the same q.  a.E is the global
// entity count; qsan is not written (the ranged bitmap reads the queries).
template <int M, int MODE, int VEC, int NS>
__global__ __launch_bounds__(256) void k_topk_prep_rows(TopkArgs a) {
  constexpr bool CPLX = Traits<M>::cplx;
  using R_ = Row<NS, VEC, CPLX>;
  const int lane = threadIdx.x & 63;
  const int64_t qi = (int64_t)blockIdx.x * 4 + wave_id();
  if (qi >= a.nq) return;
  Consts c = a.c;
  if constexpr (M == PROTATE) c.modulus = a.modulus[0];
  const int64_t x = a.queries[qi * 3 + (MODE == HEAD_BATCH ? 2 : 0)], r = a.queries[qi * 3 + 1];
  const bool bad = x < 0 || x >= a.E || r < 0 || r >= a.R;
  if (lane == 0) {
    a.state[qi] = bad ? TOPK_BAD : TOPK_VALID;
    if (bad) atomicOr(a.err, KGE_DEVERR_INDEX);
  }
  if (bad) return;
  R_ q, xr, rr;
  load_row<NS, VEC, CPLX>(a.fixed_rows + qi * a.Le, a.eg, lane, xr);
  load_rel<M, NS, VEC, CPLX>(a.rel + r * a.Lr, a.eg, lane, rr);
  build_q<M, MODE, NS, VEC, CPLX>(xr, rr, c, q);
  store_row<NS, VEC, CPLX>(a.q + qi * a.Le, a.eg, lane, q);
}

// Wave-scan top-k (any row the register kernels hold): one wave per (query,
// part) scores its candidates in ascending id as k_rank_scan does and offers
// those that beat the list's threshold.
template <int M, int MODE, int VEC, int NS>
__global__ __launch_bounds__(256) void k_topk_scan(TopkArgs a) {
  constexpr bool CPLX = Traits<M>::cplx;
  using R_ = Row<NS, VEC, CPLX>;
  __shared__ float lss[4][KGE_TOPK_MAX_K];
  __shared__ int32_t lis[4][KGE_TOPK_MAX_K];
  const int lane = threadIdx.x & 63, w = wave_id();
  const int64_t unit = (int64_t)blockIdx.x * 4 + w;
  if (unit >= a.nq * a.parts) return;
  const int64_t qi = unit / a.parts;
  const int part = (int)(unit - qi * a.parts);
  const int64_t c0 = part * a.span;
  const int64_t c1 = (c0 + a.span < a.E) ? (c0 + a.span) : a.E;
  volatile float* ls = lss[w];
  volatile int32_t* li = lis[w];
  for (int p = lane; p < a.k; p += 64) {
    ls[p] = -__builtin_inff();
    li[p] = TOPK_NO_ID;
  }
  __builtin_amdgcn_wave_barrier();
  if (a.state[qi] == TOPK_VALID) {
    Consts c = a.c;
    if constexpr (M == PROTATE) c.modulus = a.modulus[0];
    const uint32_t* bits = a.fbits + qi * a.W;
    R_ q;
    load_row<NS, VEC, CPLX>(a.q + qi * a.Le, a.eg, lane, q);
    float thr = -__builtin_inff();
    for (int64_t e = c0; e < c1; ++e) {
      if (filter_bit(bits, e)) continue;  // wave-uniform
      R_ r0;
      load_row<NS, VEC, CPLX>(a.ent + e * a.Le, a.eg, lane, r0);
      const float s0 = Elem<M, MODE>::finish(wave_sum(lane_total<M, MODE, NS, VEC, CPLX>(q, r0, c)), c);
      if (s0 > thr) thr = topk_insert(ls, li, a.k, s0, (int32_t)e, lane);  // (false for NaN)
    }
  }
  topk_store(a, qi, part, ls, li, lane);
}

// Register-tile top-k: a workgroup takes 64 queries and one candidate part and
// walks the part's 64-candidate tiles in ascending id with k_rank_tile's
// reduction (tile_reduce).  A query's 64 scores of a tile sit in the 16 lanes
// of one wave (its row of the 4 × 4 thread blocks), so its list is that wave's
// alone: no block-wide step in the epilogue.  Each lane keeps its four
// queries' thresholds in registers; a pair costs the filter bit and one
// compare, and only pairs that beat the threshold are offered — one at a time
// per wave, lowest lane and candidate first, which is ascending id within a
// query.  After an offer the row's threshold moves and its waiting pairs are
// re-screened.  A score equal to the threshold comes from a higher id than
// every listed one (ids ascend within the part), so it loses: the tie rule.
template <int M, int MODE>
__global__ __launch_bounds__(256) void k_topk_tile(TopkTileArgs b) {
  const TileArgs& a = b.t;
  using C_ = TileCfg<M, true>;
  constexpr int T = C_::T, BK = C_::BK;
  __shared__ __attribute__((aligned(16))) float Qs[BK][C_::QSTR];
  __shared__ __attribute__((aligned(16))) float Es[BK][C_::ESTR];
  extern __shared__ __attribute__((aligned(16))) float tk_lists[];  // [T][k] scores, then [T][k] ids
  const int k = b.k;
  volatile float* lsb = tk_lists;
  volatile int32_t* lib = reinterpret_cast<int32_t*>(tk_lists + T * k);
  const int t = threadIdx.x, lane = t & 63, w = wave_id();
  const int ty = t >> 4, tx = t & 15;
  const int64_t q0 = (int64_t)blockIdx.y * T;
  const int part = blockIdx.x;
  const int64_t c0 = part * b.span;
  const int64_t c1 = (c0 + b.span < a.E) ? (c0 + b.span) : a.E;
  Consts c = a.c;
  if constexpr (M == PROTATE) c.modulus = a.modulus[0];
  for (int i = t; i < T * k; i += 256) {
    lsb[i] = -__builtin_inff();
    lib[i] = TOPK_NO_ID;
  }
  bool rowok[4];
  float thr[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int64_t q = q0 + ty * 4 + i;
    rowok[i] = q < a.nq && a.true_id[q] == TOPK_VALID;
    thr[i] = -__builtin_inff();
  }
  __syncthreads();

  for (int64_t e0 = c0; e0 < c1; e0 += T) {
    tf2 acc[4][2];
    tile_reduce<M, MODE, false, true>(a, c, q0, e0, nullptr, nullptr, Qs, Es, acc);
    auto pair_total = [&](int i, int j) -> float { return (j & 1) ? acc[i][j >> 1].y : acc[i][j >> 1].x; };
    const int64_t eb0 = e0 + tx * 4;  // four candidates in one bitmap word
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float s[4];
      uint32_t pm = 0u;  // this lane's pairs of row i that wait to be offered
#pragma unroll
      for (int j = 0; j < 4; ++j) s[j] = Elem<M, MODE>::finish(pair_total(i, j), c);
      if (rowok[i] && eb0 < a.E) {
        const uint32_t word = a.fbits[(q0 + ty * 4 + i) * a.W + (eb0 >> 5)];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int64_t e = eb0 + j;
          const bool ok = (e < a.E) && (((word >> (e & 31)) & 1u) == 0u);
          if (ok && s[j] > thr[i]) pm |= 1u << j;  // (false for NaN)
        }
      }
      uint64_t waiting = __ballot(pm != 0u);
      while (waiting) {  // the rare path
        const int L = __builtin_ctzll(waiting);
        const int jn = pm ? __builtin_ctz(pm) : 0;
        const float sn = (jn == 0) ? s[0] : (jn == 1) ? s[1] : (jn == 2) ? s[2] : s[3];
        const int jL = __builtin_amdgcn_readlane(jn, L);
        const float sL = readlanef(sn, L);
        const int row = (w * 4 + (L >> 4)) * 4 + i;
        const int32_t eL = (int32_t)(e0 + (L & 15) * 4 + jL);
        const float nt = topk_insert(lsb + row * k, lib + row * k, k, sL, eL, lane);
        if (lane == L) pm &= pm - 1u;
        if ((lane >> 4) == (L >> 4)) {
          thr[i] = nt;
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (!(s[j] > nt)) pm &= ~(1u << j);
        }
        waiting = __ballot(pm != 0u);
      }
    }
  }
  // each wave writes its 16 rows' lists
  for (int r = 0; r < 16; ++r) {
    const int row = w * 16 + r;
    const int64_t q = q0 + row;
    if (q >= a.nq) break;
    const int64_t dst = (q * b.parts + part) * k;
    for (int p = lane; p < k; p += 64) {
      b.pscore[dst + p] = lsb[row * k + p];
      b.pid[dst + p] = lib[row * k + p];
    }
  }
}

template <int M>
int launch_topk_tile(int mode, const TopkTileArgs& b, hipStream_t s) {
  const dim3 grid((unsigned)b.parts, (unsigned)((b.t.nq + TILE_RQ - 1) / TILE_RQ));
  const size_t lds = (size_t)TILE_RQ * b.k * (sizeof(float) + sizeof(int32_t));
  auto go = [&](auto kern) {
    // the lists of k > 64 pass the 64 KB a launch may use without asking
    if (lds > 32768) {
      const hipError_t he = hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      if (he != hipSuccess) return (int)he;
    }
    hipLaunchKernelGGL(kern, grid, dim3(256), lds, s, b);
    return (int)hipGetLastError();
  };
  return go(pick_dir(mode, k_topk_tile<M, HEAD_BATCH>, k_topk_tile<M, TAIL_BATCH>));
}

// ---------------------------------------------- near-tie refinement
// Window of query q (one wave per query), and its reference-order q vector.
// δ_q bounds |fast score − reference-order score| of the true entity plus that
// of any candidate the window has to catch (standard fp32 summation bounds,
// γ_n ≤ 1.01·n·u with u = 2^-24; a sum of n rounded terms in ANY order has
// error ≤ γ_(depth+1)·Σ|terms|, depth ≤ n − 1):
//   DistMult   2.5·1.01·(K + D)·u·‖q‖₂·max‖e‖₂    (fast: K products in any
//              order (MFMA fma chain, VALU sequential, DPP tree) ≤ γ_K; the
//              reference: a rounded product then ATen's sum(dim=2) cascade,
//              whose depth is ≤ 16 per accumulator level × 3 levels + the
//              column / vector-lane / tail folds < 80 for K ≤ 2^20 —
//              D = min(K, 96) + 1 —; |Σ q_k e_k| terms ≤ ‖q‖‖e‖ (Cauchy-
//              Schwarz); × 2 scores (candidate and true entity) × 1.25 margin;
//              × 1 score when s_true is the reference-order score itself,
//              k_rank_true_ref, a.true_exact: then only the candidate's
//              |fast − reference| has to stay inside δ)
//   ComplEx    2.5·1.01·(2K + D + 2)·u·‖q‖₂·max‖e‖₂  (2K products fast; the
//              reference's K two-product elements, then the same cascade)
//   (split-bf16 tile, both: fast_u instead of K / 2K, plus the split's own
//              error from the pieces' norms, below)
//   TransE /   2.5·((1.01·(K + D_ref) + 5.02)·u·(S + 1) + 2u·(|γ| + |s_true| + 1))
//   RotatE     (terms ≥ 0 sum to S = γ − s; D_ref = D for RotatE's cascade, K for
//              TransE's sequential norm; 5.02u per element for RotatE's modulus,
//              0 for TransE) + 32·u·Σ|x| for RotatE's fp32 sincos in the fast q
//              (x = the anchor row); none with the caller's trig table (fast and
//              reference q identical); 1.25 instead of 2.5 when s_true is the
//              reference-order score (a.true_exact: RotatE on the register tile)
//   pRotatE    modulus·(2.5·(1.01·(K + D) + 3)·u·(S_true + 1) + 32·K·u
//              + 4·u·(Σ|q| + K·max|θ_e|)) + 8·u·(|γ| + |s_true|)
//              (the terms |sin| ≥ 0 sum to S = (γ − s)/modulus: the fast sum in
//              any order γ_K, the reference's cascade γ_D, the product with the
//              modulus and the reference's rounded sin 3u, × 2 scores × 1.25;
//              per-element fast-table and phase-rounding errors in the other
//              terms.  Rounds 1-4 used 8·K·u·(S + 1): 2.6× wider at K = 500);
//              on the register tile s_true is a point of the reference score's
//              interval (k_rank_true_ref): the sum term × 1.25 instead of 2.5,
//              plus the interval's width, added there
// TransE on the register tile is already the reference's sequence (same q,
// same sequential sum from 0): δ = 0, only exact ties are listed.
// (xrow: the anchor row where it is not the table's — kge_rank_shard_fast's
// fixed_rows[q], whose owner may be another rank)
template <int M, int MODE>
__device__ __forceinline__ void rank_window_body(const RefArgs& a, int64_t qi, int64_t qrow,
                                                 const float* xrow = nullptr) {
  constexpr bool CPLX = Traits<M>::cplx;
  const int lane = threadIdx.x & 63;
  if (a.true_id[qi] < 0) {
    if (lane == 0) a.delta[qi] = -1.f;
    return;
  }
  Consts c = a.c;
  if constexpr (M == PROTATE) c.modulus = a.modulus[0];
  const int64_t h = a.queries[qrow * 3], r = a.queries[qrow * 3 + 1], t = a.queries[qrow * 3 + 2];
  const int64_t x = (MODE == HEAD_BATCH) ? t : h;
  const float* xr = xrow ? xrow : a.ent + x * a.Le;
  const float* rr = a.rel + r * a.Lr;
  const float* qf = a.q + qi * a.Le;
  float* qo = a.qref + qi * a.Le;
  const float* tr = (M == ROTATE && a.trig) ? a.trig + r * 2 * a.Lr : nullptr;
  float n2 = 0.f, a1 = 0.f;  // ‖q_fast‖², Σ|x| (RotatE) or Σ|q| (pRotatE)
  float ql2 = 0.f, qr2 = 0.f;  // split tile: Σ (lo·2^8)², Σ (r·2^16)² of q_fast's bf16 split (bf16_split_scaled)
  const bool split = (M == DISTMULT || M == COMPLEX) && a.fast_u > 0.f;
  for (int k = lane; k < a.K; k += 64) {
    const float xa = xr[k], xb = CPLX ? xr[a.K + k] : 0.f;
    const float ra = rr[k], rb = (M == COMPLEX) ? rr[a.K + k] : 0.f;
    float qa, qb;
    ref_make_q<M, MODE>(xa, xb, ra, rb, c, qa, qb, tr, k, a.K);
    qo[k] = qa;
    if constexpr (CPLX) qo[a.K + k] = qb;
    const float fa = qf[k], fb = CPLX ? qf[a.K + k] : 0.f;
    n2 += fa * fa + fb * fb;
    if (split) {
      float l8, r16;
      bf16_split_scaled(fa, l8, r16);
      ql2 += l8 * l8;
      qr2 += r16 * r16;
      if constexpr (CPLX) {
        bf16_split_scaled(fb, l8, r16);
        ql2 += l8 * l8;
        qr2 += r16 * r16;
      }
    }
    a1 += (M == ROTATE) ? (fabsf(xa) + fabsf(xb)) : fabsf(qa);
  }
  n2 = wave_sum(n2);
  a1 = wave_sum(a1);
  if (split) {  // (wave-uniform)
    ql2 = wave_sum(ql2);
    qr2 = wave_sum(qr2);
  }
  if (lane != 0) return;
  const float u = 5.9604645e-8f;  // 2^-24
  const float K = (float)a.K, st = a.s_true[qi];
  float d;
  const float D = fminf(K, 96.f) + 1.f;  // ATen cascade depth bound (kge_rank_ref.h)
  const float qn = sqrtf(n2) * 1.0001f;   // ‖q‖ from an fp32 sum (γ_K relative)
  if constexpr (M == DISTMULT || M == COMPLEX) {
    // fast-pass bound: K (fp32 tile / VALU, ComplEx 2K products) or the split
    // tile's own (a.fast_u), plus the reference's D (+2 for ComplEx's pairs)
    const float Kd = (M == COMPLEX) ? 2.f * K : K;
    const float fast = (a.fast_u > 0.f) ? a.fast_u : Kd;
    const float c1 = a.true_exact ? 1.2625f : 2.525f, Ne = a.stats[0];
    d = c1 * (fast + D + (M == COMPLEX ? 2.f : 0.f)) * u * qn * Ne;
    if (split) {
      // the split's own error, from the pieces' actual sizes (q = q_hi + q_lo + r_q
      // exactly, e likewise; e_lo·q_lo not computed):
      //   |Σq e − Σ(q_hi e_hi + q_hi e_lo + q_lo e_hi)| = |Σ(q r_e + r_q e − r_q r_e + q_lo e_lo)|
      //   ≤ ‖q‖‖r_e‖ + ‖r_q‖‖e‖ + ‖r_q‖‖r_e‖ + ‖q_lo‖‖e_lo‖      (Cauchy-Schwarz per sum)
      // with the table's maxima of ‖e‖, ‖r_e‖, ‖e_lo‖ (stats[0], [2], [3]).  The
      // worst case, |r| ≤ 2^-16 |x| and |lo| ≤ 2^-8 (1 + 2^-8) |x|, gave 770·u·‖q‖‖e‖;
      // uniform tables measure ≈ 42·u per residual and 0.41·2^-8 per lo piece (≈ 126·u)
      const float mg = 1.0001f + (float)a.Le * 3.1e-8f;
      const float rqn = sqrtf(qr2) * mg * 0x1p-16f, lqn = sqrtf(ql2) * mg * 0x1p-8f;
      const float Re = a.stats[2], Lo = a.stats[3];
      d += c1 * 1.0001f * ((qn * Re + rqn * Ne) + (rqn * Re + lqn * Lo));
      // bf16 pieces or fp32 products below the normal range may flush to zero:
      // ≤ 2^-126 per operand piece and per product, 4 per element; elements
      // whose squares underflow in the fp32 norms (|v| < 2^-63 after the
      // pieces' power-of-two scaling) add ≤ 2^-63 × the other factor to each of
      // the four sums and to P: Le·2^-60·(‖q‖ + ‖e‖ + 1) covers them
      d += 4.f * Kd * (qn + Ne + 1.f) * 1.1754944e-38f + (float)a.Le * 0x1p-60f * (qn + Ne + 1.f);
    }
  } else if constexpr (M == TRANSE || M == ROTATE) {
    // per fast score: its own sum of K terms in any order (γ_K), the
    // reference's (RotatE: ATen's sum(dim=2) cascade, depth ≤ D; TransE:
    // norm(p=1), sequential, K), RotatE's elements (the same rounded
    // differences; fast mul, mul, add and the native ≤ 1-ulp sqrt ≤ 3u,
    // reference mul, fma and correctly rounded sqrt ≤ 2u: ≤ 5.02u of each
    // modulus), and the γ − · rounding of both scores; terms ≥ 0 sum to S =
    // γ − s.  × 2 fast scores (the candidate and the gather pass's s_true) ×
    // 1.25 margin — × 1 when s_true is the reference-order score
    // (k_rank_true_ref, a.true_exact; S then comes from the gather pass's
    // fast s_true, within 1e-4·S of the exact one, inside the margin); + an
    // absolute 8·2^-126 per element for underflowing squares.  (Rounds 1-4
    // used 8·K·u·(S + 1): ≈ 2.9× wider at K = 1000.)
    const float Dr = (M == ROTATE) ? D : K;
    const float el = (M == ROTATE) ? 5.02f : 0.f;
    const float S = fabsf(c.gamma - st) + 1.f;
    d = a.exact_fast ? 0.f
                     : (a.true_exact ? 1.25f : 2.5f) * ((1.01f * (K + Dr) + el) * u * S + 2.f * u * (fabsf(c.gamma) + fabsf(st) + 1.f)) +
                           8.f * K * 1.1754944e-38f;
    if constexpr (M == ROTATE)
      if (!tr) d += 32.f * u * a1;  // with the caller's trig table both q are the same bits
  } else {
    const float mod = fabsf(c.modulus);
    const float S = (mod > 0.f) ? fabsf(c.gamma - st) / mod : K;
    d = mod * ((a.true_exact ? 1.25f : 2.5f) * (1.01f * (K + D) + 3.f) * u * (S + 1.f) + 32.f * K * u +
               4.f * u * (a1 + K * a.stats[1] / fabsf(c.kappa_p))) +
        8.f * u * (fabsf(c.gamma) + fabsf(st));
    // the reference's sin from the caller's library (≤ 1 ulp ≤ 2u per element
    // instead of the correctly rounded ≤ u), for the candidate and the true score
    if (a.lib_sin) d += mod * 4.f * K * u;
  }
  a.delta[qi] = (d == d && d < INFINITY) ? d : INFINITY;  // a NaN bound lists everything
}

template <int M, int MODE>
__global__ __launch_bounds__(256) void k_rank_window(RefArgs a) {
  int64_t bx;
  const int md = ref_dir<MODE>(bx);
  const int64_t j = bx * 4 + wave_id();
  if (j >= a.nq) return;
  const int64_t qi = (md == TAIL_BATCH && MODE == BOTH_DIRS) ? a.nq + j : j;
  if (md == HEAD_BATCH) rank_window_body<M, HEAD_BATCH>(a, qi, j);
  else rank_window_body<M, TAIL_BATCH>(a, qi, j);
}

#include "kge_row_walk.inc"

// Refinement of the listed near-ties, one 256-thread block per query.  Work
// item 0 is the true entity, items 1..n the listed candidates; the
// half-waves with a staging slot take items j = half, half + nslot, ...  The
// reference-order sum walks its elements in a data-dependent cascade, so it
// reads them from LDS: the query's reference q is staged once per block and
// each item's row is copied into the half's slot with all its loads in flight
// at once (reading the row from global memory inside the cascade exposed one
// memory latency per 32-element step: 0.16 ms per wn18rr DistMult direction).
// Scores land in LDS; the block then counts strictly-greater and equal.
// Dynamic LDS (no static __shared__: it would shift the 16-B alignment of the
// dynamic base): [q: Lp][scores: cap + 1][upper ends: cap + 1][2 counters,
// rounded to 4][slots: nslot × Lp] floats, Lp = Le rounded to 4 (refine_slots).
// pRotatE, three-call form: the list stage (screen) scores each item as an
// interval under any library sin within one ulp (ref_score_half_prot_bounds)
// and decides every candidate whose interval clears the true one's; the
// finish stage (sinv) scores the remaining items from the caller's sin
// values.
__host__ __device__ inline int refine_capp(int cap) { return (2 * (cap + 1) + 2 + 3) & ~3; }
inline int refine_slots(int Le, int cap) {
  const int free_ = 65536 / 4 - refine_lp(Le) - refine_capp(cap);
  const int k = free_ / refine_lp(Le);
  return k > 8 ? 8 : (k < 1 ? 1 : k);
}
// the list tag (pRotatE's three-call form): the list stage's mode, nq and
// table, which sin_args / finish must match
__device__ __forceinline__ bool list_tag_ok(const RefArgs& a) {
  return a.ltag && a.ltag[0] == a.ltag_v[0] && a.ltag[1] == a.ltag_v[1] && a.ltag[2] == a.ltag_v[2];
}
// PQ: float4 per lane of the prefetched next row (rows of ≤ 128·PQ floats;
// 0: no prefetch) — a template parameter, so a short row's kernel does not
// carry a long row's registers (DistMult's 500-float rows lost occupancy to them)
template <int M, int MODE, int PQ>
__device__ __forceinline__ void rank_refine_body(const RefArgs& a, int64_t qi) {
  extern __shared__ __attribute__((aligned(16))) float rsm[];
  const int tid = threadIdx.x, hl = tid & 31, half = tid >> 5;
  const int64_t tid_ = a.true_id[qi];
  if (tid_ < 0) return;
  Consts c = a.c;
  if constexpr (M == PROTATE) c.modulus = a.modulus[0];
  const int Le = a.Le, Lp = refine_lp(Le);
  // ref_global (rows too wide for LDS): q and the rows are read in place
  float* qs_l = rsm;
  float* scr = rsm + (a.ref_global ? 0 : Lp);
  float* scr_hi = scr + a.cap + 1;
  int* cnt_s = reinterpret_cast<int*>(scr + 2 * (a.cap + 1));
  float* slots = scr + refine_capp(a.cap);
  const int n = a.ucnt[qi];
  int items = (n > a.cap) ? 1 : n + 1;  // overflow: the true score only (k_rank_exact reads it)
  // pRotatE with the caller's sin: item j's row is its K sin values (Le == K)
  const bool sinv = (M == PROTATE) && a.sins;
  const bool iv = (M == PROTATE) && a.screen && !sinv;
  // nothing listed: the fast pass's counts are final, and the true score's
  // reference value is read only for overflowed lists (k_rank_exact[_iv]) —
  // the whole block is skipped (TransE's exact fast pass lists ≈0.02 per query)
  if (n == 0 && !sinv) return;
  if (sinv) {
    // items delivered for this query: none (decided on the device, or in
    // another call's chunk), or exactly the true entity and its n listed
    const int64_t have = a.item_off[qi + 1] - a.item_off[qi];
    if (have == 0) return;
    const bool bad = !list_tag_ok(a) || n == 0 || n > a.cap || have != 1 + (int64_t)n || a.done[qi] != 0;
    __syncthreads();  // every thread has read done[qi] before thread 0 sets it
    if (bad) {
      if (tid == 0) atomicOr(a.err, KGE_DEVERR_ARG);
      return;
    }
    if (tid == 0) a.done[qi] = 1;
    items = n + 1;
  }
  const int32_t* lst = a.ulist + qi * (int64_t)a.cap;
  const float* qr = a.qref + qi * Le;
  if (!a.ref_global)
    for (int k = tid; k < Le; k += 256) qs_l[k] = qr[k];
  const float* qs = a.ref_global ? qr : qs_l;
  __syncthreads();
  const float* srow0 = sinv ? a.sins + a.item_off[qi] * (int64_t)Le : nullptr;
  const bool vec4 = ((Le & 3) == 0) && ((((uintptr_t)(sinv ? a.sins : a.ent)) & 15) == 0);
  if (half < a.ref_slots) {
    float* const row_l = slots + half * Lp;
    auto row_src = [&](int j) -> const float* {
      int64_t e = (j == 0) ? tid_ : (int64_t)lst[j - 1];
      if (e < 0 || e >= a.E) e = tid_;
      return sinv ? srow0 + (int64_t)j * Le : a.ent + e * Le;
    };
    // item j's score in the reference's order from its row (LDS or in place)
    auto score_item = [&](int j, const float* row) {
      if constexpr (M == PROTATE) {
        if (iv) {
          const tf2 b = ref_score_half_prot_bounds<MODE>(qs, row, a.K, c, hl);
          if (hl == 0) {
            scr[j] = b.x;
            scr_hi[j] = b.y;
          }
        } else {
          const float sc = sinv ? ref_score_half<M, MODE, true>(qs, row, a.K, c, hl)
                                : ref_score_half<M, MODE>(qs, row, a.K, c, hl);
          if (hl == 0) scr[j] = sc;
        }
      } else {
        const float sc = ref_score_half<M, MODE>(qs, row, a.K, c, hl);
        if (hl == 0) scr[j] = sc;
      }
      // (the score depends on every element of the row through the shuffles,
      // so the row's reads are done before the next item overwrites it)
    };
    const int n4 = Le >> 2;
    if (PQ > 0 && !a.ref_global && vec4 && n4 <= 32 * PQ) {
      // the half's next item's row is loaded into registers while this item
      // is scored (the row loads used to wait in front of every score)
      float4 nx[PQ > 0 ? PQ : 1];
      auto fetch = [&](int j) {
        const float4* s4 = reinterpret_cast<const float4*>(row_src(j));
#pragma unroll
        for (int u = 0; u < PQ; ++u) {
          const int k = hl + 32 * u;
          nx[u] = (k < n4) ? s4[k] : make_float4(0.f, 0.f, 0.f, 0.f);
        }
      };
      float4* r4 = reinterpret_cast<float4*>(row_l);
      if (half < items) fetch(half);
      for (int j = half; j < items; j += a.ref_slots) {
#pragma unroll
        for (int u = 0; u < PQ; ++u) {
          const int k = hl + 32 * u;
          if (k < n4) r4[k] = nx[u];
        }
        if (j + a.ref_slots < items) fetch(j + a.ref_slots);
        // the half's 32 lanes read each other's writes: LDS operations of one
        // wave complete in order, so waiting for this wave's writes suffices
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        score_item(j, row_l);
      }
    } else {
      for (int j = half; j < items; j += a.ref_slots) {
        float* row = row_l;
        const float* src = row_src(j);
        if (a.ref_global) {
          row = const_cast<float*>(src);  // read in place (never written)
        } else if (vec4) {
          stage_row<4>(src, row, n4, hl);
        } else {
          stage_row<1>(src, row, Le, hl);
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        score_item(j, row);
      }
    }
  }
  __syncthreads();
  const float st = scr[0];
  if (tid == 0) {
    a.sref_true[qi] = st;
    if (iv) a.sref_hi[qi] = scr_hi[0];
  }
  if (n > a.cap) return;  // overflow: k_rank_exact (k_rank_exact_iv in the list stage) rescans this query
  if constexpr (M == PROTATE) {
    if (iv) {
      // a listed candidate whose interval lies wholly above the true score's
      // is counted, one wholly below is dropped; the others stay listed for
      // the caller's library sin (NaN bounds: kept).  a.decide = 0 keeps all.
      const float tl = scr[0], th = scr_hi[0];
      if (tid < 2) cnt_s[tid] = 0;
      int kid[4];
      bool keep[4];
      int g = 0;
#pragma unroll
      for (int u4 = 0; u4 < 4; ++u4) {  // n ≤ cap = 4 · 256
        const int j = 1 + tid + 256 * u4;
        keep[u4] = false;
        kid[u4] = 0;
        if (j <= n) {
          const float lo = scr[j], hi = scr_hi[j];
          if (a.decide && lo > th) ++g;
          else if (!a.decide || !(hi < tl)) {
            keep[u4] = true;
            kid[u4] = lst[j - 1];
          }
        }
      }
      __syncthreads();  // every listed id read before the list is rewritten
      g = (int)wave_sum((float)g);
      if ((tid & 63) == 0 && g) atomicAdd(&cnt_s[0], g);
#pragma unroll
      for (int u4 = 0; u4 < 4; ++u4)
        if (keep[u4]) a.ulist_w[qi * (int64_t)a.cap + atomicAdd(&cnt_s[1], 1)] = kid[u4];
      __syncthreads();
      if (tid == 0) {
        a.gt[qi] += cnt_s[0];
        a.ucnt_w[qi] = cnt_s[1];
      }
      return;
    }
  }
  if (tid < 2) cnt_s[tid] = 0;
  __syncthreads();
  count_scores(scr + 1, n, st, cnt_s, [](int) { return false; });
  __syncthreads();
  if (tid == 0) {
    a.gt[qi] += cnt_s[0];
    a.eq[qi] += cnt_s[1];
  }
}

template <int M, int MODE, int PQ>
__global__ __launch_bounds__(256) void k_rank_refine(RefArgs a) {
  int64_t bx;
  const int md = ref_dir<MODE>(bx);
  if (bx >= a.nq) return;
  const int64_t qi = (md == TAIL_BATCH && MODE == BOTH_DIRS) ? a.nq + bx : bx;
  if (md == HEAD_BATCH) rank_refine_body<M, HEAD_BATCH, PQ>(a, qi);
  else rank_refine_body<M, TAIL_BATCH, PQ>(a, qi);
}

// Queries whose window overflowed the list (degenerate tables: many exact or
// near ties): every unfiltered candidate in reference order, one wave per query.
template <int M, int MODE>
__device__ __forceinline__ void rank_exact_body(const RefArgs& a, int64_t qi) {
  const int lane = threadIdx.x & 63, hl = lane & 31, half = lane >> 5;
  const int64_t tid_ = a.true_id[qi];
  if (tid_ < 0 || a.ucnt[qi] <= a.cap) return;
  Consts c = a.c;
  if constexpr (M == PROTATE) c.modulus = a.modulus[0];
  const float* qr = a.qref + qi * a.Le;
  const float st = a.sref_true[qi];
  const uint32_t* bits = a.fbits + qi * a.W;
  int g = 0, e_ = 0;
  for (int64_t e0 = 0; e0 < a.E; e0 += 2) {
    const int64_t e = e0 + half;
    const bool valid = e < a.E && !((bits[(e < a.E ? e : 0) >> 5] >> (e & 31)) & 1u);
    const float sc = ref_score_half<M, MODE>(qr, a.ent + (valid ? e : tid_) * a.Le, a.K, c, hl);
    if (valid && hl == 0) {
      g += (sc > st);
      e_ += (sc == st);
    }
  }
  g += __shfl_xor(g, 32);
  e_ += __shfl_xor(e_, 32);
  if (lane == 0) {
    a.gtx[qi] = g;
    a.eqx[qi] = e_;
  }
}

template <int M, int MODE>
__global__ __launch_bounds__(256) void k_rank_exact(RefArgs a) {
  int64_t bx;
  const int md = ref_dir<MODE>(bx);
  const int64_t j = bx * 4 + wave_id();
  if (j >= a.nq) return;
  const int64_t qi = (md == TAIL_BATCH && MODE == BOTH_DIRS) ? a.nq + j : j;
  if (md == HEAD_BATCH) rank_exact_body<M, HEAD_BATCH>(a, qi);
  else rank_exact_body<M, TAIL_BATCH>(a, qi);
}

// pRotatE's list stage, queries whose window overflowed the list: every
// unfiltered candidate's score interval under any library sin within one ulp
// (as the screen in k_rank_refine), one wave per query.  Candidates above the
// true interval are counted; the undecided ones are listed.  If they fit the
// list, the query continues as a listed one (its count replaced by this
// scan's, its list by the undecided candidates) and only they go to the
// caller's sin; otherwise (a degenerate table: more than a list of
// candidates inside the true score's last-bit interval) the query is ranked
// here with correctly rounded sin — exact to the reference up to the
// library's last bits — and keeps its overflow mark, so the caller's buffer
// never holds more than a list per query.
template <int M, int MODE>
__global__ __launch_bounds__(256) void k_rank_exact_iv(RefArgs a) {
  if constexpr (M == PROTATE) {
    const int lane = threadIdx.x & 63, hl = lane & 31, half = lane >> 5;
    const int64_t qi = (int64_t)blockIdx.x * 4 + wave_id();
    if (qi >= a.nq) return;
    const int64_t tid_ = a.true_id[qi];
    if (tid_ < 0 || a.ucnt[qi] <= a.cap) return;
    Consts c = a.c;
    c.modulus = a.modulus[0];
    const float* qr = a.qref + qi * a.Le;
    const float tl = a.sref_true[qi], th = a.sref_hi[qi];
    const uint32_t* bits = a.fbits + qi * a.W;
    int32_t* lst = a.ulist_w + qi * (int64_t)a.cap;
    int g = 0, namb = 0;  // namb: wave-uniform (ballot)
    for (int64_t e0 = 0; e0 < a.E; e0 += 2) {
      const int64_t e = e0 + half;
      const bool valid = e < a.E && !((bits[(e < a.E ? e : 0) >> 5] >> (e & 31)) & 1u);
      const tf2 b = ref_score_half_prot_bounds<MODE>(qr, a.ent + (valid ? e : tid_) * a.Le, a.K, c, hl);
      const bool above = valid && b.x > th;
      const bool amb = valid && !above && !(b.y < tl);
      if (above && hl == 0) ++g;
      const uint64_t am = __ballot(amb && hl == 0);  // bit 0: half 0's candidate, bit 32: half 1's
      if (am & 1ull) {
        if (lane == 0 && namb < a.cap) lst[namb] = (int32_t)e;
        ++namb;
      }
      if ((am >> 32) & 1ull) {
        if (lane == 32 && namb < a.cap) lst[namb] = (int32_t)e;
        ++namb;
      }
    }
    g += __shfl_xor(g, 32);
    if (namb <= a.cap) {
      if (lane == 0) {
        a.gt[qi] = g;
        a.ucnt_w[qi] = namb;
      }
      return;
    }
    // too many undecided candidates: correctly rounded sin for this query
    const float st = ref_score_half<M, MODE>(qr, a.ent + tid_ * a.Le, a.K, c, hl);
    int gx = 0, ex = 0;
    for (int64_t e0 = 0; e0 < a.E; e0 += 2) {
      const int64_t e = e0 + half;
      const bool valid = e < a.E && !((bits[(e < a.E ? e : 0) >> 5] >> (e & 31)) & 1u);
      const float sc = ref_score_half<M, MODE>(qr, a.ent + (valid ? e : tid_) * a.Le, a.K, c, hl);
      if (valid && hl == 0) {
        gx += (sc > st);
        ex += (sc == st);
      }
    }
    gx += __shfl_xor(gx, 32);
    ex += __shfl_xor(ex, 32);
    if (lane == 0) {
      a.gtx[qi] = gx;
      a.eqx[qi] = ex;
    }
  }
}

// pRotatE: the K phase sums of every item of a query (the arguments of the
// reference's sin, model.py:236-245 — IEEE divisions and adds in the
// reference's association, so host-independent), one block per query, a wave
// per item.  Item 0 is the true entity, then the listed candidates.  A query
// whose [item_off] range is empty is skipped (decided on the device, or
// delivered in another chunk); one whose range is not empty and does not hold
// exactly 1 + its listed count, or a call whose list tag does not match the
// list stage's, flags KGE_DEVERR_ARG.
template <int M, int MODE>
__global__ __launch_bounds__(256) void k_rank_sin_args(RefArgs a) {
  if constexpr (M == PROTATE) {
    const int64_t qi = blockIdx.x;
    if (qi >= a.nq) return;
    const int64_t tid_ = a.true_id[qi];
    const int64_t off = a.item_off[qi];
    const int64_t items = a.item_off[qi + 1] - off;
    if (items == 0) return;
    const int n = a.ucnt[qi];
    if (!list_tag_ok(a) || tid_ < 0 || n == 0 || n > a.cap || items != 1 + (int64_t)n) {
      if (threadIdx.x == 0) atomicOr(a.err, KGE_DEVERR_ARG);
      return;
    }
    const int lane = threadIdx.x & 63, w = wave_id();
    const int K = a.K;
    const float kp = a.c.kappa_p;
    const float* qr = a.qref + qi * a.Le;
    const int32_t* lst = a.ulist + qi * (int64_t)a.cap;
    for (int64_t j = w; j < items; j += 4) {
      int64_t e = (j == 0) ? tid_ : (int64_t)lst[j - 1];
      if (e < 0 || e >= a.E) e = tid_;
      const float* er = a.ent + e * a.Le;
      float* o = a.args + (off + j) * (int64_t)K;
      for (int k = lane; k < K; k += 64) {
        const float pe = er[k] / kp;  // model.py:236 / :238
        o[k] = (MODE == HEAD_BATCH) ? (pe + qr[k]) : (qr[k] - pe);  // model.py:240-243
      }
    }
  }
}

// The true entity's score in the reference's own order, as the counting
// pass's s_true (split-bf16 path; replaces the gather-mode tile, which ran
// one workgroup per 128 queries: 25 on wn18rr, ≈55 µs).  Sound for the
// window: a candidate is counted when fast − s_true > δ, and with s_true
// exact only the candidate's own fast-pass error has to stay inside δ, which
// k_rank_window's pair bound covers with room.  One half-wave per query, q
// (k_rank_window's reference-order q) and the true row staged in LDS, the
// refinement's own scoring (ref_score_half).  Le ≤ 1024 (64 KB of LDS);
// wider rows (a.ref_global) are read in place — RotatE on the register tile
// (its rows are 2K floats) uses that form, one row pair per query.  pRotatE
// (register tile): a point of the reference score's interval under any 1-ulp
// sin, the window widened by the interval's width.
template <int M, int MODE>
__device__ __forceinline__ void rank_true_ref_body(const RefArgs& a, int64_t qi) {
  extern __shared__ __attribute__((aligned(16))) float tsm[];
  const int tid = threadIdx.x, hl = tid & 31, hw = tid >> 5;
  const int64_t t = a.true_id[qi];
  if (t < 0 || t >= a.E) {
    if (hl == 0) a.s_true_w[qi] = 0.f;
    return;
  }
  Consts c = a.c;
  if constexpr (M == PROTATE) c.modulus = a.modulus[0];
  const int Le = a.Le, Lp = refine_lp(Le);
  const float* qp = a.qref + qi * Le;
  const float* ep = a.ent + t * Le;
  if (!a.ref_global) {
    float* qs = tsm + hw * 2 * Lp;
    float* row = qs + Lp;
    for (int k = hl; k < Le; k += 32) {
      qs[k] = qp[k];
      row[k] = ep[k];
    }
    // the half-wave's lanes read each other's writes: this wave's LDS
    // operations complete in order
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    qp = qs;
    ep = row;
  }
  if constexpr (M == PROTATE) {
    // the reference's score under any sin within one ulp (the caller's
    // library, or the correctly rounded one) lies in [lo, hi]
    // (ref_score_half_prot_bounds): s_true = a float of it and the window
    // grows by the width, so |s_true − reference| ≤ the added term; a
    // non-finite interval keeps the fast s_true and lists every candidate
    const tf2 b = ref_score_half_prot_bounds<MODE>(qp, ep, a.K, c, hl);
    if (hl == 0) {
      const float w = b.y - b.x;
      if (w == w && w < INFINITY) {
        a.s_true_w[qi] = fminf(fmaxf(0.5f * b.x + 0.5f * b.y, b.x), b.y);
        const float d = a.delta[qi];
        if (d >= 0.f) a.delta[qi] = d + w * 1.0000003f;
      } else {
        a.delta[qi] = INFINITY;
      }
    }
  } else {
    const float sc = ref_score_half<M, MODE>(qp, ep, a.K, c, hl);
    if (hl == 0) a.s_true_w[qi] = sc;
  }
}

template <int M, int MODE>
__global__ __launch_bounds__(256) void k_rank_true_ref(RefArgs a) {
  int64_t bx;
  const int md = ref_dir<MODE>(bx);
  const int64_t j = bx * 8 + (threadIdx.x >> 5);
  if (j >= a.nq) return;  // (a whole half-wave)
  const int64_t qi = (md == TAIL_BATCH && MODE == BOTH_DIRS) ? a.nq + j : j;
  if (md == HEAD_BATCH) rank_true_ref_body<M, HEAD_BATCH>(a, qi);
  else rank_true_ref_body<M, TAIL_BATCH>(a, qi);
}

template <int M>
int launch_rank_ref(int mode, RefStage stage, const RefArgs& a, hipStream_t s) {
  RefArgs b = a;
  size_t lds = 0;
  unsigned g = (unsigned)((a.nq + 3) / 4);
  auto launch = [&](auto k, unsigned grid) {
    hipLaunchKernelGGL(k, dim3(grid), dim3(256), lds, s, b);
    return (int)hipGetLastError();
  };
  // (BOTH_DIRS: both directions' queries in one launch, twice the grid)
  auto go = [&](auto kh, auto kt, auto kb) {
    return mode == BOTH_DIRS ? launch(kb, 2 * g) : launch(pick_dir(mode, kh, kt), g);
  };
  switch (stage) {
    case RefStage::TrueRef: {
      if (!a.s_true_w) return (int)hipErrorInvalidValue;
      b.ref_global = refine_lp(a.Le) > 1024 ? 1 : 0;
      lds = b.ref_global ? 0 : sizeof(float) * 16 * (size_t)refine_lp(a.Le);
      g = (unsigned)((a.nq + 7) / 8);  // a half-wave per query
      return go(k_rank_true_ref<M, HEAD_BATCH>, k_rank_true_ref<M, TAIL_BATCH>, k_rank_true_ref<M, BOTH_DIRS>);
    }
    case RefStage::SinArgs:  // (a block per query; no both-directions form, as Interval)
      if (M != PROTATE) return (int)hipErrorInvalidValue;
      return launch(pick_dir(mode, k_rank_sin_args<M, HEAD_BATCH>, k_rank_sin_args<M, TAIL_BATCH>), (unsigned)a.nq);
    case RefStage::Interval:
      if (M != PROTATE) return (int)hipErrorInvalidValue;
      return launch(pick_dir(mode, k_rank_exact_iv<M, HEAD_BATCH>, k_rank_exact_iv<M, TAIL_BATCH>), g);
    case RefStage::Window:
      return go(k_rank_window<M, HEAD_BATCH>, k_rank_window<M, TAIL_BATCH>, k_rank_window<M, BOTH_DIRS>);
    case RefStage::Refine: {
      g = (unsigned)a.nq;  // a block per query
      // q and one row slot must fit the 64 KB of LDS; wider rows are read in place
      b.ref_global = (refine_lp(a.Le) * 2 + refine_capp(a.cap) > 65536 / 4) ? 1 : 0;
      b.ref_slots = b.ref_global ? 8 : refine_slots(a.Le, a.cap);
      lds = sizeof(float) * (size_t)(b.ref_global ? refine_capp(a.cap)
                                                  : refine_lp(a.Le) * (1 + b.ref_slots) + refine_capp(a.cap));
      const int n4 = a.Le >> 2;  // float4 per row (the prefetch path's condition is rechecked in the kernel)
      if (n4 <= 128)
        return go(k_rank_refine<M, HEAD_BATCH, 4>, k_rank_refine<M, TAIL_BATCH, 4>, k_rank_refine<M, BOTH_DIRS, 4>);
      if (n4 <= 256)
        return go(k_rank_refine<M, HEAD_BATCH, 8>, k_rank_refine<M, TAIL_BATCH, 8>, k_rank_refine<M, BOTH_DIRS, 8>);
      if (n4 <= 512)
        return go(k_rank_refine<M, HEAD_BATCH, 16>, k_rank_refine<M, TAIL_BATCH, 16>,
                  k_rank_refine<M, BOTH_DIRS, 16>);
      return go(k_rank_refine<M, HEAD_BATCH, 0>, k_rank_refine<M, TAIL_BATCH, 0>, k_rank_refine<M, BOTH_DIRS, 0>);
    }
    case RefStage::Exact:
      return go(k_rank_exact<M, HEAD_BATCH>, k_rank_exact<M, TAIL_BATCH>, k_rank_exact<M, BOTH_DIRS>);
  }
  return -1;  // (not a RefStage)
}

// ------------------------------------- ranking against candidate lists
// kge_rank_candidates: every query brings its own list cand[q, 0..C) (negative
// ids: padding) and is ranked among exactly those, in the reference's fp32
// operation order — k_rank_refine's scoring with the caller's list in place of
// the fast pass's near-ties, so there is no fast pass, no window and no filter.
// Work unit = (query, chunk of cpc candidates), one 256-thread block each,
// chunk-minor on grid.x.  The block builds the query's reference q in LDS
// (ref_make_q, as k_rank_window), then its half-waves with a row slot walk the
// items j = half, half + nslot, ...: item 0 is the true entity, items 1..n the
// chunk's candidates, each row through the half's LDS slot (walk_rows).
// The ids of a half's next 32 items sit one per lane, so a row's address never
// waits for an id load.  Padding and out-of-range ids score the true row and
// store NaN, which compares neither greater nor equal: a half-wave's shuffles
// never diverge.  Scores land in LDS; the block counts them against item 0's
// and adds its two integers to the query's counters.
// Dynamic LDS, floats: [q: Lp][scores: 1 + cpc | 2 counters, walk_scrp][slots:
// nslot × Lp], Lp = refine_lp(Le).  Rows too wide for q and one slot (in_place)
// are read where they lie and q comes from k_rank_cand_q's global copy
// (walk_scrp, cand_slots: kge_internal.h).

// a query's reference-order q from its fixed-side row xr, its relation row rr
// and (RotatE, or null) the relation's [cos | sin] row tr, element k by thread
// k mod 256 (k_rank_window's q)
template <int M, int MODE>
__device__ __forceinline__ void ref_build_q(const float* xr, const float* rr, const float* tr, int K, const Consts& c,
                                            float* __restrict__ qo) {
  constexpr bool CPLX = Traits<M>::cplx;
  for (int k = threadIdx.x; k < K; k += 256) {
    const float xa = xr[k], xb = CPLX ? xr[K + k] : 0.f;
    const float ra = rr[k], rb = (M == COMPLEX) ? rr[K + k] : 0.f;
    float qa, qb;
    ref_make_q<M, MODE>(xa, xb, ra, rb, c, qa, qb, tr, k, K);
    qo[k] = qa;
    if constexpr (CPLX) qo[K + k] = qb;
  }
}
// ... with the fixed side's row read from the table
template <int M, int MODE>
__device__ __forceinline__ void cand_build_q(const CandArgs& a, int64_t h, int64_t r, int64_t t, const Consts& c,
                                             float* __restrict__ qo) {
  ref_build_q<M, MODE>(a.ent + ((MODE == HEAD_BATCH) ? t : h) * a.Le, a.rel + r * a.Lr,
                       (M == ROTATE && a.trig) ? a.trig + r * 2 * a.Lr : nullptr, a.K, c, qo);
}

// a query whose three ids lie in the tables
__device__ __forceinline__ bool query_ok(int64_t E, int64_t R, int64_t h, int64_t r, int64_t t) {
  return h >= 0 && h < E && t >= 0 && t < E && r >= 0 && r < R;
}

// TransE over a row staged in the half's own LDS slot: torch.norm(p=1) is one
// fp32 accumulator over ascending k, which no lane can share — ref_score_half
// has every lane add the 32 elements of a step from 32 shuffles, one LDS-pipe
// operation per element, and that pipe, not the gather, bounded the call (85 ms
// at the 2.5 M-entity shape against a 12 ms gather).  Here the elements
// |q ∓ e| are written over the row, 32 at a time, and every lane then adds them
// from 16-byte broadcast reads: the same values in the same order from the
// same 0, a quarter of the LDS operations.  (Rows read in place keep
// ref_score_half: global memory is not written.)
template <int MODE>
__device__ __forceinline__ float cand_score_transe_lds(const float* __restrict__ q, float* row, int K, const Consts& c,
                                                       int hl) {
  for (int k = hl; k < K; k += 32) row[k] = ref_elem<TRANSE, MODE>(q[k], 0.f, row[k], 0.f, c);
  // the half's lanes read each other's writes: this wave's LDS operations complete in order
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  float acc = 0.f;
  int k = 0;
  for (; k + 4 <= K; k += 4) {
    const tf4 v = *reinterpret_cast<const tf4*>(row + k);  // (slots are 16-byte aligned)
    acc += v.x;
    acc += v.y;
    acc += v.z;
    acc += v.w;
  }
  for (; k < K; ++k) acc += row[k];
  return ref_finish<TRANSE>(acc, c);
}

// in_place only: q of every query into the workspace, one block per query
template <int M, int MODE>
__global__ __launch_bounds__(256) void k_rank_cand_q(CandArgs a) {
  const int64_t qi = blockIdx.x;
  const int64_t h = a.queries[qi * 3], r = a.queries[qi * 3 + 1], t = a.queries[qi * 3 + 2];
  if (!query_ok(a.E, a.R, h, r, t)) return;  // (k_rank_cand flags it)
  cand_build_q<M, MODE>(a, h, r, t, a.c, a.qref + qi * a.Le);
}

// PQ, VW: the shape of the row walk (walk_rows, kge_row_walk.inc; walk_variant picks them)
template <int M, int MODE, int PQ, int VW>
__global__ __launch_bounds__(256) void k_rank_cand(CandArgs a) {
  extern __shared__ __attribute__((aligned(16))) float csm[];
  constexpr bool IN_PLACE = PQ < 0;
  const int tid = threadIdx.x, hl = tid & 31, half = tid >> 5;
  const int64_t qi = (int64_t)blockIdx.x / a.chunks;
  const int64_t ch = (int64_t)blockIdx.x - qi * a.chunks;
  const int64_t h = a.queries[qi * 3], r = a.queries[qi * 3 + 1], t = a.queries[qi * 3 + 2];
  if (!query_ok(a.E, a.R, h, r, t)) {  // (block-uniform) rank 0, ties 0: k_rank_cand_emit
    if (ch == 0 && tid == 0) atomicOr(a.err, KGE_DEVERR_INDEX);
    return;
  }
  const int32_t true_e = (int32_t)((MODE == HEAD_BATCH) ? h : t);
  Consts c = a.c;
  if constexpr (M == PROTATE) c.modulus = a.modulus[0];
  const int Le = a.Le, Lp = refine_lp(Le);
  const int64_t j0 = ch * a.cpc;
  const int n = (int)((a.C - j0 < a.cpc) ? (a.C - j0) : a.cpc);  // ≥ 1
  const int items = n + 1;
  float* scr = csm + (IN_PLACE ? 0 : Lp);
  int* cnt_s = reinterpret_cast<int*>(scr + a.cpc + 1);
  float* slots = scr + walk_scrp(a.cpc);
  if constexpr (!IN_PLACE) cand_build_q<M, MODE>(a, h, r, t, c, csm);
  const float* qs = IN_PLACE ? a.qref + qi * Le : csm;
  if (tid < 2) cnt_s[tid] = 0;
  __syncthreads();
  const int64_t* lst = a.cand + qi * a.C + j0;
  const int ns = IN_PLACE ? 8 : a.nslot;
  if (half < ns) {
    // the half's i-th item is j = half + ns·i; lane hl holds the row id of item
    // i with i mod 32 = hl of the current group of 32: the true id for item 0
    // and for a candidate that is not scored (my_ok = 0 then says "discard");
    // walk_rows asks for i ascending, every i once
    int my_e = true_e, my_ok = 1;
    auto item_src = [&](int i, bool& ok) __attribute__((always_inline)) -> const float* {
      if ((i & 31) == 0) {
        const int j = half + ns * (i + hl);
        my_e = true_e;
        my_ok = 1;
        if (j > 0 && j < items) {
          const int64_t e = lst[j - 1];
          my_ok = (e >= 0 && e < a.E);
          if (my_ok) my_e = (int32_t)e;
          else if (e >= a.E) atomicOr(a.err, KGE_DEVERR_INDEX);
        }
      }
      const int src = ((tid & 32) + (i & 31)) << 2;
      ok = __builtin_amdgcn_ds_bpermute(src, my_ok) != 0;
      return a.ent + (int64_t)__builtin_amdgcn_ds_bpermute(src, my_e) * Le;
    };
    auto score = [&](int j, float* row, bool ok) __attribute__((always_inline)) {
      float sc;
      if constexpr (M == TRANSE && !IN_PLACE) sc = cand_score_transe_lds<MODE>(qs, row, a.K, c, hl);
      else sc = ref_score_half<M, MODE>(qs, row, a.K, c, hl);
      if (hl == 0) scr[j] = ok ? sc : NAN;
    };
    walk_rows<PQ, VW>(items, half, ns, hl, slots + half * Lp, Le, item_src, score);
  }
  __syncthreads();
  count_scores(scr + 1, n, scr[0], cnt_s, [](int) { return false; });
  __syncthreads();
  if (tid == 0) {  // integer sums: any order of the chunks gives the same counts
    if (cnt_s[0]) atomicAdd(&a.gt[qi], cnt_s[0]);
    if (cnt_s[1]) atomicAdd(&a.eq[qi], cnt_s[1]);
  }
}

template <int M>
int launch_rank_cand(int mode, const CandArgs& a, hipStream_t s) {
  const int Lp = refine_lp(a.Le);
  if (a.in_place) {
    hipLaunchKernelGGL(pick_dir(mode, k_rank_cand_q<M, HEAD_BATCH>, k_rank_cand_q<M, TAIL_BATCH>),
                       dim3((unsigned)a.nq), dim3(256), 0, s, a);
    const int st = (int)hipGetLastError();
    if (st) return st;
  }
  const size_t lds = sizeof(float) * (size_t)((a.in_place ? 0 : Lp * (1 + a.nslot)) + walk_scrp(a.cpc));
  const dim3 grid((unsigned)(a.nq * a.chunks));
  return walk_variant(a.in_place, a.vec4, a.Le, [&](auto pq, auto vw) {
    constexpr int PQ = decltype(pq)::value, VW = decltype(vw)::value;
    hipLaunchKernelGGL(pick_dir(mode, k_rank_cand<M, HEAD_BATCH, PQ, VW>, k_rank_cand<M, TAIL_BATCH, PQ, VW>), grid,
                       dim3(256), lds, s, a);
    return (int)hipGetLastError();
  });
}

// ------------------------------------------------- relation prediction
// kge_rank_relations: query (h, r, t) is scored with every relation r' in
// [0, R) — k_rank_cand with the roles turned round: the two entity rows are
// fixed per query, the relation rows are the ones walked.  Work unit = (query,
// chunk of cpc consecutive relations), one 256-thread block each, chunk-minor
// on grid.x.  The block stages the query's h row and t row in LDS once; its
// half-waves with a row slot walk the items j = half, half + nslot, ...: item 0
// is the true relation (relation 0 when r = −1: its score is never compared),
// items 1..n the relations j0 .. j0 + n − 1.  A relation row — RotatE: its
// [cos | sin] row of the trig table, the caller's or the one k_rel_trig_table
// built in the workspace — is staged into the half's LDS slot from registers
// loaded while the previous item was scored.  Element k is ref_elem<M, TAIL>(
// ref_make_q<M, TAIL>(h_k, r'_k), t_k): 'single' mode is the tail-batch
// association (model.py:166-249), reduced by ref_cascade_half, or for TransE
// by the sequential sum over the elements written back over the slot
// (cand_score_transe_lds's trick).  Scores land in LDS; the ids of the query's
// filter list that fall into the chunk are marked in a bitmap of cpc bits; the
// block counts the unmarked relations other than r against item 0, adds its two
// integers to the query's counters and writes its slice of scores_out.
// Dynamic LDS, floats: [h: Lp][t: Lp][scores: 1 + cpc | 2 counters, walk_scrp]
// [bitmap: walk_bmw words][slots: nslot × Lp], Lp = refine_lp(Le) — a relation
// row, or RotatE's [cos | sin] row, is Le floats wide.  Rows too wide for h, t
// and one slot (in_place) are all read where they lie (rel_slots:
// kge_internal.h).

// element k of the (h, r', t) triple's reduction; row: the relation row, RotatE: [cos | sin]
template <int M>
__device__ __forceinline__ float rel_elem(const float* hs, const float* ts, const float* row, int k, int K,
                                          const Consts& c) {
  constexpr bool CPLX = Traits<M>::cplx;
  const float xa = hs[k], xb = CPLX ? hs[K + k] : 0.f;
  const float ra = (M == ROTATE) ? 0.f : row[k], rb = (M == COMPLEX) ? row[K + k] : 0.f;
  float qa, qb;
  ref_make_q<M, TAIL_BATCH>(xa, xb, ra, rb, c, qa, qb, (M == ROTATE) ? row : nullptr, k, K);
  return ref_elem<M, TAIL_BATCH>(qa, qb, ts[k], CPLX ? ts[K + k] : 0.f, c);
}

// reference-order score by one half-wave, rows wherever they lie (ref_score_half's reductions)
template <int M>
__device__ __forceinline__ float rel_score_half(const float* hs, const float* ts, const float* row, int K,
                                                const Consts& c, int hl) {
  auto elem = [&](int k) -> float { return rel_elem<M>(hs, ts, row, k, K, c); };
  if constexpr (M == TRANSE) {
    float acc = 0.f;
    for (int k0 = 0; k0 < K; k0 += 32) {
      const int k = k0 + hl;
      const float v = (k < K) ? elem(k) : 0.f;
      const int m = (K - k0 < 32) ? (K - k0) : 32;
      for (int j = 0; j < m; ++j) acc += half_shfl(v, j);
    }
    return ref_finish<M>(acc, c);
  } else {
    // eight rows of 32 elements evaluated before they are added: an element
    // reads h, r' and t from LDS (RotatE six values), and one row at a time
    // left every read's latency exposed (FB15k's shape: DistMult d = 2000 29.1 ms
    // per call, 18.6 ms with eight; RotatE d = 1000 43.4 → 31.3 ms)
    return ref_finish<M>(ref_cascade_half<float, decltype(elem), 8>(elem, K, hl), c);
  }
}

// TransE over a relation row staged in the half's own slot: the elements
// |(h + r') − t| over the row, then added from 16-byte broadcast reads in
// ascending k (cand_score_transe_lds), 32 floats read ahead of their adds
__device__ __forceinline__ float rel_score_transe_lds(const float* hs, const float* ts, float* row, int K,
                                                      const Consts& c, int hl) {
  for (int k0 = hl; k0 < K; k0 += 128) {  // four elements' reads before their writes
    float e[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int k = k0 + 32 * u;
      e[u] = (k < K) ? rel_elem<TRANSE>(hs, ts, row, k, K, c) : 0.f;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (k0 + 32 * u < K) row[k0 + 32 * u] = e[u];
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  float acc = 0.f;
  int k = 0;
  for (; k + 32 <= K; k += 32) {
    tf4 v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = *reinterpret_cast<const tf4*>(row + k + 4 * u);
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      acc += v[u].x;
      acc += v[u].y;
      acc += v[u].z;
      acc += v[u].w;
    }
  }
  for (; k + 4 <= K; k += 4) {
    const tf4 v = *reinterpret_cast<const tf4*>(row + k);
    acc += v.x;
    acc += v.y;
    acc += v.z;
    acc += v.w;
  }
  for (; k < K; ++k) acc += row[k];
  return ref_finish<TRANSE>(acc, c);
}

// PQ, VW: the shape of the row walk (walk_rows, kge_row_walk.inc)
template <int M, int PQ, int VW>
__global__ __launch_bounds__(256) void k_rank_rel(RelRankArgs a) {
  extern __shared__ __attribute__((aligned(16))) float rsm[];
  constexpr bool IN_PLACE = PQ < 0;
  const int tid = threadIdx.x, hl = tid & 31, half = tid >> 5;
  const int64_t qi = (int64_t)blockIdx.x / a.chunks;
  const int64_t ch = (int64_t)blockIdx.x - qi * a.chunks;
  const int64_t h = a.queries[qi * 3], r = a.queries[qi * 3 + 1], t = a.queries[qi * 3 + 2];
  const int64_t j0 = ch * a.cpc;
  const int n = (int)((a.R - j0 < a.cpc) ? (a.R - j0) : a.cpc);  // ≥ 1
  // (query_ok with r = −1, "no true relation", let through)
  if (!(h >= 0 && h < a.E && t >= 0 && t < a.E && r >= -1 && r < a.R)) {  // (block-uniform)
    if (ch == 0 && tid == 0) atomicOr(a.err, KGE_DEVERR_INDEX);
    if (a.scores)
      for (int j = tid; j < n; j += 256) a.scores[qi * a.R + j0 + j] = NAN;
    return;  // rank 0, ties 0: k_rank_cand_emit
  }
  Consts c = a.c;
  if constexpr (M == PROTATE) c.modulus = a.modulus[0];
  const int Le = a.Le, Lp = refine_lp(Le);
  const int items = n + 1;
  float* scr = rsm + (IN_PLACE ? 0 : 2 * Lp);
  int* cnt_s = reinterpret_cast<int*>(scr + a.cpc + 1);
  uint32_t* bm = reinterpret_cast<uint32_t*>(scr + walk_scrp(a.cpc));
  float* slots = scr + walk_scrp(a.cpc) + walk_bmw(a.cpc);
  const float* hs = a.ent + h * Le;
  const float* ts = a.ent + t * Le;
  if constexpr (!IN_PLACE) {
    for (int k = tid; k < Le; k += 256) {
      rsm[k] = hs[k];
      rsm[Lp + k] = ts[k];
    }
    hs = rsm;
    ts = rsm + Lp;
  }
  if (tid < 2) cnt_s[tid] = 0;
  for (int w = tid; w < walk_bmw(a.cpc); w += 256) bm[w] = 0u;
  __syncthreads();
  if (a.filt_off && r >= 0) {  // the excluded ids of this chunk (any order, repeats, ids outside [0, R): harmless)
    const int64_t f1 = a.filt_off[qi + 1];
    for (int64_t i = a.filt_off[qi] + tid; i < f1; i += 256) {
      const int64_t x = a.filt_ids[i] - j0;
      if (x >= 0 && x < n) atomicOr(&bm[x >> 5], 1u << (x & 31));
    }
  }
  // relation rows: RotatE walks the trig table's [cos | sin] rows (2·Lr = Le floats)
  const float* tab = (M == ROTATE) ? a.trig : a.rel;
  const int64_t r0 = r >= 0 ? r : 0;
  const int ns = IN_PLACE ? 8 : a.nslot;
  if (half < ns) {
    auto item_row = [&](int i, bool&) __attribute__((always_inline)) -> const float* {  // the half's i-th item
      const int j = half + ns * i;
      return tab + (j == 0 ? r0 : j0 + j - 1) * Le;
    };
    auto score = [&](int j, float* row, bool) __attribute__((always_inline)) {
      float sc;
      if constexpr (M == TRANSE && !IN_PLACE) sc = rel_score_transe_lds(hs, ts, row, a.K, c, hl);
      else sc = rel_score_half<M>(hs, ts, row, a.K, c, hl);
      if (hl == 0) scr[j] = sc;
    };
    walk_rows<PQ, VW>(items, half, ns, hl, slots + half * Lp, Le, item_row, score);
  }
  __syncthreads();
  if (a.scores)
    for (int j = 1 + tid; j <= n; j += 256) a.scores[qi * a.R + j0 + j - 1] = scr[j];
  if (r < 0) return;  // (block-uniform) prediction: no true relation, nothing to count
  count_scores(scr + 1, n, scr[0], cnt_s, [&](int x) {  // the true relation itself; excluded
    return j0 + x == r || ((bm[x >> 5] >> (x & 31)) & 1u) != 0u;
  });
  __syncthreads();
  if (tid == 0) {  // integer sums: any order of the chunks gives the same counts
    if (cnt_s[0]) atomicAdd(&a.gt[qi], cnt_s[0]);
    if (cnt_s[1]) atomicAdd(&a.eq[qi], cnt_s[1]);
  }
}

template <int M>
int launch_rank_rel(const RelRankArgs& a, hipStream_t s) {
  const int Lp = refine_lp(a.Le);
  const size_t lds =
      sizeof(float) * (size_t)((a.in_place ? 0 : Lp * (2 + a.nslot)) + walk_scrp(a.cpc) + walk_bmw(a.cpc));
  const dim3 grid((unsigned)(a.nq * a.chunks));
  return walk_variant(a.in_place, a.vec4, a.Le, [&](auto pq, auto vw) {
    hipLaunchKernelGGL((k_rank_rel<M, decltype(pq)::value, decltype(vw)::value>), grid, dim3(256), lds, s, a);
    return (int)hipGetLastError();
  });
}

// ------------------------------------------- sharded filtered ranking
// kge_rank_shard: the filtered ranks over a row shard [own_lo, own_hi) of the
// entity table, in three stages with the host's all-reduces between them
// (kge_hip.h).  a.ent points own_lo rows before the shard, so rows are
// addressed by global id and only owned ones are touched; the fixed side's row
// and the true score come from the caller's reduced buffers, never from the
// scanned table.
//   k_rshard_rows   a half-wave per query copies the fixed side's row (its
//                   bits) where owned, zero bits elsewhere.
//   k_rshard_true   a workgroup per query builds the reference q in LDS from
//                   fixed_rows[q]; its first half-wave scores the true row where
//                   it lies (ref_score_half, TransE included: the sequential
//                   sum cand_score_transe_lds reproduces).
//   k_rshard_count  k_rank_cand with a contiguous range in place of a list.
//                   Work unit = (chunk of cpc consecutive owned rows, query),
//                   one 256-thread workgroup each, QUERY-minor on grid.x: the
//                   workgroups resident together scan the same chunk, whose
//                   rows then come from L2.  The workgroup builds q, then the
//                   exclusion bitmap of its chunk (≤ 32 words) from the query's
//                   filter list and the true id with LDS atomics; its half-
//                   waves walk the rows j = half, half + nslot, ... staged
//                   through their LDS slots one row ahead.  Every row is
//                   scored (no divergence inside a half-wave); the excluded
//                   ones are left out when the scores are counted against
//                   s_true[q].  The two integers go to counts by atomics.
// Dynamic LDS of k_rshard_count, floats: [q: Lp][scores: cpc | 2 counters,
// walk_scrp][bitmap: walk_bmw][slots: nslot × Lp] (the first three QW times over
// with QW queries per workgroup).  Rows too wide for q and one
// slot (in_place) are read where they lie and q comes from k_rshard_q's copy in
// the workspace.

__device__ __forceinline__ bool rshard_owned(const ShardArgs& a, int64_t e) { return e >= a.own_lo && e < a.own_hi; }

// the query's reference-order q from the reduced fixed-side row (ref_build_q;
// A: ShardArgs or CandShardArgs)
template <int M, int MODE, class A>
__device__ __forceinline__ void rshard_build_q(const A& a, int64_t qi, int64_t r, const Consts& c,
                                               float* __restrict__ qo) {
  ref_build_q<M, MODE>(a.fixed_rows + qi * a.Le, a.rel + r * a.Lr,
                       (M == ROTATE && a.trig) ? a.trig + r * 2 * a.Lr : nullptr, a.K, c, qo);
}

template <int M, int MODE>
__global__ __launch_bounds__(256) void k_rshard_rows(ShardArgs a) {
  const int hl = threadIdx.x & 31;
  const int64_t qi = (int64_t)blockIdx.x * 8 + (threadIdx.x >> 5);
  if (qi >= a.nq) return;  // (a whole half-wave)
  const int64_t x = a.queries[qi * 3 + (MODE == HEAD_BATCH ? 2 : 0)];
  if ((x < 0 || x >= a.E) && hl == 0) atomicOr(a.err, KGE_DEVERR_INDEX);
  uint32_t* out = reinterpret_cast<uint32_t*>(a.fixed_rows + qi * a.Le);  // (bits, not values)
  if (rshard_owned(a, x)) {
    const uint32_t* src = reinterpret_cast<const uint32_t*>(a.ent + x * a.Le);
    for (int k = hl; k < a.Le; k += 32) out[k] = src[k];
  } else {
    for (int k = hl; k < a.Le; k += 32) out[k] = 0u;
  }
}

// in_place only: q of every query into the workspace, one block per query
template <int M, int MODE>
__global__ __launch_bounds__(256) void k_rshard_q(ShardArgs a) {
  const int64_t qi = blockIdx.x;
  const int64_t h = a.queries[qi * 3], r = a.queries[qi * 3 + 1], t = a.queries[qi * 3 + 2];
  if (!query_ok(a.E, a.R, h, r, t)) return;  // (k_rshard_count flags it)
  rshard_build_q<M, MODE>(a, qi, r, a.c, a.qref + qi * a.Le);
}

template <int M, int MODE>
__global__ __launch_bounds__(256) void k_rshard_true(ShardArgs a) {
  extern __shared__ __attribute__((aligned(16))) float tqs[];
  const int tid = threadIdx.x;
  const int64_t qi = blockIdx.x;
  const int64_t h = a.queries[qi * 3], r = a.queries[qi * 3 + 1], t = a.queries[qi * 3 + 2];
  const int64_t te = (MODE == HEAD_BATCH) ? h : t;
  if (!query_ok(a.E, a.R, h, r, t) || !rshard_owned(a, te)) {  // (block-uniform)
    if (tid == 0) reinterpret_cast<uint32_t*>(a.s_true)[qi] = 0u;
    return;
  }
  Consts c = a.c;
  if constexpr (M == PROTATE) c.modulus = a.modulus[0];
  const float* qs = a.qref + qi * a.Le;
  if (!a.in_place) {
    rshard_build_q<M, MODE>(a, qi, r, c, tqs);
    qs = tqs;
  }
  __syncthreads();
  if (tid < 32) {
    const float sc = ref_score_half<M, MODE>(qs, a.ent + te * a.Le, a.K, c, tid);
    if (tid == 0) a.s_true[qi] = sc;
  }
}

// PQ, VW: the shape of the row walk (walk_rows).  QW: queries per workgroup —
// every staged row is scored against QW consecutive queries, whose q vectors, score arrays and
// bitmaps sit side by side in LDS (the same arithmetic per (query, row), 1 / QW
// of the row reads; staged 16-byte rows of DistMult / ComplEx / RotatE /
// pRotatE only: TransE's LDS sum overwrites the staged row).
template <int M, int MODE, int PQ, int VW, int QW = 1>
__global__ __launch_bounds__(256) void k_rshard_count(ShardArgs a) {
  extern __shared__ __attribute__((aligned(16))) float ssm[];
  constexpr bool IN_PLACE = PQ < 0;
  static_assert(QW == 1 || (!IN_PLACE && M != TRANSE), "several queries per workgroup: staged rows, not TransE");
  const int tid = threadIdx.x, hl = tid & 31, half = tid >> 5;
  const int64_t groups = (a.nq + QW - 1) / QW;
  const int64_t ch = (int64_t)blockIdx.x / groups;  // chunk-major: neighbours on grid.x scan the same rows
  const int64_t qi0 = ((int64_t)blockIdx.x - ch * groups) * QW;
  int64_t te[QW];
  bool ok[QW];  // (block-uniform) a bad query's counts stay 0 / 0
  bool any = false;
  Consts c = a.c;
  if constexpr (M == PROTATE) c.modulus = a.modulus[0];
  const int Le = a.Le, Lp = refine_lp(Le);
  const int64_t e0 = a.own_lo + ch * a.cpc;  // the chunk's first row
  const int n = (int)((a.own_hi - e0 < a.cpc) ? (a.own_hi - e0) : a.cpc);  // (0: an empty shard's one chunk)
  const int scrp = walk_scrp(a.cpc), bmw = walk_bmw(a.cpc);
  float* const scr0 = ssm + (IN_PLACE ? 0 : QW * Lp);   // query w: scores scr0 + w·scrp (2 counters behind them),
  uint32_t* const bm0 = reinterpret_cast<uint32_t*>(scr0 + QW * scrp);  // bitmap bm0 + w·bmw, q at ssm + w·Lp
  float* slots = scr0 + QW * (scrp + bmw);
  for (int w = tid; w < QW * bmw; w += 256) bm0[w] = 0u;
  if (tid < 2 * QW) reinterpret_cast<int*>(scr0 + (tid >> 1) * scrp + a.cpc)[tid & 1] = 0;
  __syncthreads();
#pragma unroll
  for (int w = 0; w < QW; ++w) {
    const int64_t qi = qi0 + w;
    ok[w] = false;
    te[w] = 0;
    if (qi >= a.nq) continue;  // (the last group may be short)
    const int64_t h = a.queries[qi * 3], r = a.queries[qi * 3 + 1], t = a.queries[qi * 3 + 2];
    if (!query_ok(a.E, a.R, h, r, t)) {
      if (ch == 0 && tid == 0) atomicOr(a.err, KGE_DEVERR_INDEX);
      continue;
    }
    ok[w] = any = true;
    te[w] = (MODE == HEAD_BATCH) ? h : t;
    if constexpr (!IN_PLACE) rshard_build_q<M, MODE>(a, qi, r, c, ssm + w * Lp);
    // the chunk's excluded rows: the true id, and the filter list's ids that fall into it
    uint32_t* bm = bm0 + w * bmw;
    int64_t f0, f1;
    if (a.ftab) {  // the whole index: the query's key (k_filter_bits_tab's lookup)
      const int64_t key = (MODE == HEAD_BATCH) ? r * a.E + t : h * a.R + r;
      f0 = a.filt_off[key];
      f1 = a.filt_off[key + 1];
    } else {
      f0 = a.filt_off[qi];
      f1 = a.filt_off[qi + 1];
    }
    for (int64_t i = f0 + tid; i < f1; i += 256) {
      const int64_t x = a.filt_ids[i] - e0;
      if (x >= 0 && x < n) atomicOr(&bm[x >> 5], 1u << (x & 31));
    }
    const int64_t x = te[w] - e0;
    if (tid == 0 && x >= 0 && x < n) atomicOr(&bm[x >> 5], 1u << (x & 31));
  }
  if (!any) return;
  __syncthreads();  // q is read by every half-wave
  const int ns = IN_PLACE ? 8 : a.nslot;
  if (half < ns) {
    // the half's i-th item is row j = half + ns·i of the chunk
    auto item_row = [&](int i, bool&) __attribute__((always_inline)) -> const float* {
      return a.ent + (e0 + half + ns * i) * Le;
    };
    auto score = [&](int j, float* row, bool) __attribute__((always_inline)) {
#pragma unroll
      for (int w = 0; w < QW; ++w) {
        if (QW > 1 && !ok[w]) continue;  // (its q was not built)
        const float* qs = IN_PLACE ? a.qref + qi0 * Le : ssm + w * Lp;
        float sc;
        if constexpr (M == TRANSE && !IN_PLACE) sc = cand_score_transe_lds<MODE>(qs, row, a.K, c, hl);
        else sc = ref_score_half<M, MODE>(qs, row, a.K, c, hl);
        if (hl == 0) scr0[w * scrp + j] = sc;
      }
    };
    walk_rows<PQ, VW>(n, half, ns, hl, slots + half * Lp, Le, item_row, score);
  }
  __syncthreads();
#pragma unroll
  for (int w = 0; w < QW; ++w) {
    if (!ok[w]) continue;
    const float* scr = scr0 + w * scrp;
    const uint32_t* bm = bm0 + w * bmw;
    count_scores(scr, n, a.s_true[qi0 + w], reinterpret_cast<int*>(scr0 + w * scrp + a.cpc), [&](int j) {
      return ((bm[j >> 5] >> (j & 31)) & 1u) != 0u;  // the true entity itself; filtered
    });
  }
  __syncthreads();
#pragma unroll
  for (int w = 0; w < QW; ++w) {
    if (tid != w || !ok[w]) continue;  // integer sums: any order of the chunks gives the same counts
    const int* cnt_s = reinterpret_cast<const int*>(scr0 + w * scrp + a.cpc);
    unsigned long long* cn = reinterpret_cast<unsigned long long*>(a.counts);
    if (cnt_s[0]) atomicAdd(&cn[qi0 + w], (unsigned long long)cnt_s[0]);
    if (cnt_s[1]) atomicAdd(&cn[a.nq + qi0 + w], (unsigned long long)cnt_s[1]);
  }
}

template <int M>
int launch_rank_shard(int mode, int stage, const ShardArgs& a, hipStream_t s) {
  const int Lp = refine_lp(a.Le);
  auto launch = [&](auto kh, auto kt, unsigned grid, size_t lds) {
    hipLaunchKernelGGL(pick_dir(mode, kh, kt), dim3(grid), dim3(256), lds, s, a);
    return (int)hipGetLastError();
  };
  if (stage == KGE_RSHARD_ROWS)
    return launch(k_rshard_rows<M, HEAD_BATCH>, k_rshard_rows<M, TAIL_BATCH>, (unsigned)((a.nq + 7) / 8), 0);
  if (a.in_place) {
    const int st = launch(k_rshard_q<M, HEAD_BATCH>, k_rshard_q<M, TAIL_BATCH>, (unsigned)a.nq, 0);
    if (st) return st;
  }
  if (stage == KGE_RSHARD_TRUE)
    return launch(k_rshard_true<M, HEAD_BATCH>, k_rshard_true<M, TAIL_BATCH>, (unsigned)a.nq,
                  a.in_place ? 0 : sizeof(float) * (size_t)Lp);
  if (stage != KGE_RSHARD_COUNT) return -1;
  const int nT = a.vec4 ? a.Le >> 2 : a.Le;  // slots per row
  // several queries per workgroup (a.qw = 2 or 4): 16-byte slots of at most 1024 floats, not TransE
  const int qw = ((a.qw == 2 || a.qw == 4) && !a.in_place && a.vec4 && nT <= 256 && M != TRANSE) ? a.qw : 1;
  ShardArgs b = a;
  b.nslot = shard_slots(a.Le, qw);
  const size_t lds = sizeof(float) * (size_t)((a.in_place ? 0 : Lp * (qw + b.nslot)) +
                                              qw * (walk_scrp(a.cpc) + walk_bmw(a.cpc)));
  const unsigned grid = (unsigned)(((a.nq + qw - 1) / qw) * a.chunks);
  auto launch_b = [&](auto kh, auto kt) {
    hipLaunchKernelGGL(pick_dir(mode, kh, kt), dim3(grid), dim3(256), lds, s, b);
    return (int)hipGetLastError();
  };
#define KGE_RSHARD_GOQ(PQ_, QW_) \
  launch_b(k_rshard_count<M, HEAD_BATCH, PQ_, 4, QW_>, k_rshard_count<M, TAIL_BATCH, PQ_, 4, QW_>)
  if constexpr (M != TRANSE) {
    if (qw == 2) return nT <= 128 ? KGE_RSHARD_GOQ(4, 2) : KGE_RSHARD_GOQ(8, 2);
    if (qw == 4) return nT <= 128 ? KGE_RSHARD_GOQ(4, 4) : KGE_RSHARD_GOQ(8, 4);
  }
#undef KGE_RSHARD_GOQ
  return walk_variant(a.in_place, a.vec4, a.Le, [&](auto pq, auto vw) {
    constexpr int PQ = decltype(pq)::value, VW = decltype(vw)::value;
    return launch_b(k_rshard_count<M, HEAD_BATCH, PQ, VW>, k_rshard_count<M, TAIL_BATCH, PQ, VW>);
  });
}

// ------------------------- sharded ranking against candidate lists
// kge_rank_candidates_shard: k_rank_cand's counts over the candidates of every
// list that fall into the row shard [own_lo, own_hi), against the caller's
// reduced s_true[q] and with q built from the reduced fixed_rows[q] — the third
// call of kge_rank_shard's protocol (ROWS, TRUE, then this).  Work unit =
// (query, chunk of cpc list places), one 256-thread workgroup each, chunk-minor
// on grid.x.  A rank owns about 1 / world of every list, so the workgroup first
// COMPACTS its chunk: the 256 threads read the ids coalesced, 256 places a
// round, and sort each into padding (negative), out of table (≥ E: flagged) or
// owned; a wave64 ballot and a popcount prefix place the owned ids of a wave,
// the four waves' counts go through LDS, and the owned ids land in list order
// in an int32 array in LDS.  A workgroup with no owned candidate leaves before
// it builds q.  There is no filler row: k_rank_cand's is the true row, which
// here may be another rank's — the half-waves walk the compacted list alone,
// each row through the half's LDS slot (walk_rows), every one scored.  Scores
// land in LDS; the block counts them against s_true[q], nothing skipped (a
// copy of the true id is a tie), and adds its two integers to counts.
// Dynamic LDS, floats: [q: Lp][scores: cpc | 2 counters, walk_scrp][owned ids:
// cpc int32 | 4 wave counts, walk_idw][slots: nslot × Lp].  Rows too wide for q
// and one slot (in_place) are read where they lie and q comes from
// k_rshard_cand_q's copy in the workspace (cand_shard_slots: kge_internal.h).

// in_place only: q of every query into the workspace, one block per query
template <int M, int MODE>
__global__ __launch_bounds__(256) void k_rshard_cand_q(CandShardArgs a) {
  const int64_t qi = blockIdx.x;
  const int64_t h = a.queries[qi * 3], r = a.queries[qi * 3 + 1], t = a.queries[qi * 3 + 2];
  if (!query_ok(a.E, a.R, h, r, t)) return;  // (k_rshard_cand flags it)
  rshard_build_q<M, MODE>(a, qi, r, a.c, a.qref + qi * a.Le);
}

// PQ, VW: the shape of the row walk (walk_rows, kge_row_walk.inc; walk_variant picks them)
template <int M, int MODE, int PQ, int VW>
__global__ __launch_bounds__(256) void k_rshard_cand(CandShardArgs a) {
  extern __shared__ __attribute__((aligned(16))) float xsm[];
  constexpr bool IN_PLACE = PQ < 0;
  const int tid = threadIdx.x, hl = tid & 31, half = tid >> 5, lane = tid & 63, wv = tid >> 6;
  const int64_t qi = (int64_t)blockIdx.x / a.chunks;
  const int64_t ch = (int64_t)blockIdx.x - qi * a.chunks;
  const int64_t h = a.queries[qi * 3], r = a.queries[qi * 3 + 1], t = a.queries[qi * 3 + 2];
  if (!query_ok(a.E, a.R, h, r, t)) {  // (block-uniform) its counts stay 0 / 0
    if (ch == 0 && tid == 0) atomicOr(a.err, KGE_DEVERR_INDEX);
    return;
  }
  // (the one copy of the constants, made here as k_rank_cand makes it: made behind the compaction,
  // pRotatE's went to a second scratch slot beside the kernel argument's)
  Consts c = a.c;
  if constexpr (M == PROTATE) c.modulus = a.modulus[0];
  const int Le = a.Le, Lp = refine_lp(Le);
  const int64_t j0 = ch * a.cpc;
  const int n = (int)((a.C - j0 < a.cpc) ? (a.C - j0) : a.cpc);  // the chunk's list places, ≥ 1
  float* scr = xsm + (IN_PLACE ? 0 : Lp);
  int* cnt_s = reinterpret_cast<int*>(scr + a.cpc);
  int32_t* ids_l = reinterpret_cast<int32_t*>(scr + walk_scrp(a.cpc));
  int* wcnt = ids_l + ((a.cpc + 3) & ~3);  // the four waves' owned counts of one round
  float* slots = scr + walk_scrp(a.cpc) + walk_idw(a.cpc);
  if (tid < 2) cnt_s[tid] = 0;
  // the chunk's owned ids, compacted in list order
  const int64_t* lst = a.cand + qi * a.C + j0;
  int nown = 0;  // (block-uniform)
  for (int x0 = 0; x0 < n; x0 += 256) {
    const int x = x0 + tid;
    const int64_t e = (x < n) ? lst[x] : (int64_t)-1;
    const bool mine = e >= a.own_lo && e < a.own_hi;  // (own_hi ≤ E, own_lo ≥ 0)
    const unsigned long long oob = __ballot(e >= a.E);
    if (oob && lane == 0) atomicOr(a.err, KGE_DEVERR_INDEX);
    const unsigned long long bal = __ballot(mine);
    if (lane == 0) wcnt[wv] = __popcll(bal);
    __syncthreads();
    const int c0 = wcnt[0], c1 = wcnt[1], c2 = wcnt[2], c3 = wcnt[3];
    if (mine) {
      const int base = nown + (wv > 0 ? c0 : 0) + (wv > 1 ? c1 : 0) + (wv > 2 ? c2 : 0);
      ids_l[base + __popcll(bal & ((1ull << lane) - 1ull))] = (int32_t)e;
    }
    nown += c0 + c1 + c2 + c3;
    __syncthreads();  // (wcnt is rewritten by the next round; ids_l and cnt_s are read below)
  }
  if (nown == 0) return;  // no candidate of this chunk is this shard's
  if constexpr (!IN_PLACE) {
    rshard_build_q<M, MODE>(a, qi, r, c, xsm);
    __syncthreads();  // q is read by every half-wave
  }
  const float* qs = IN_PLACE ? a.qref + qi * Le : xsm;
  const int ns = IN_PLACE ? 8 : a.nslot;
  if (half < ns) {
    // the half's i-th item is place j = half + ns·i of the compacted list
    auto item_src = [&](int i, bool&) __attribute__((always_inline)) -> const float* {
      return a.ent + (int64_t)ids_l[half + ns * i] * Le;
    };
    auto score = [&](int j, float* row, bool) __attribute__((always_inline)) {
      float sc;
      if constexpr (M == TRANSE && !IN_PLACE) sc = cand_score_transe_lds<MODE>(qs, row, a.K, c, hl);
      else sc = ref_score_half<M, MODE>(qs, row, a.K, c, hl);
      if (hl == 0) scr[j] = sc;
    };
    walk_rows<PQ, VW>(nown, half, ns, hl, slots + half * Lp, Le, item_src, score);
  }
  __syncthreads();
  count_scores(scr, nown, a.s_true[qi], cnt_s, [](int) { return false; });
  __syncthreads();
  if (tid == 0) {  // integer sums: any order of the chunks gives the same counts
    unsigned long long* cn = reinterpret_cast<unsigned long long*>(a.counts);
    if (cnt_s[0]) atomicAdd(&cn[qi], (unsigned long long)cnt_s[0]);
    if (cnt_s[1]) atomicAdd(&cn[a.nq + qi], (unsigned long long)cnt_s[1]);
  }
}

template <int M>
int launch_rank_cand_shard(int mode, const CandShardArgs& a, hipStream_t s) {
  const int Lp = refine_lp(a.Le);
  if (a.in_place) {
    hipLaunchKernelGGL(pick_dir(mode, k_rshard_cand_q<M, HEAD_BATCH>, k_rshard_cand_q<M, TAIL_BATCH>),
                       dim3((unsigned)a.nq), dim3(256), 0, s, a);
    const int st = (int)hipGetLastError();
    if (st) return st;
  }
  const size_t lds =
      sizeof(float) * (size_t)((a.in_place ? 0 : Lp * (1 + a.nslot)) + walk_scrp(a.cpc) + walk_idw(a.cpc));
  const dim3 grid((unsigned)(a.nq * a.chunks));
  return walk_variant(a.in_place, a.vec4, a.Le, [&](auto pq, auto vw) {
    constexpr int PQ = decltype(pq)::value, VW = decltype(vw)::value;
    hipLaunchKernelGGL(pick_dir(mode, k_rshard_cand<M, HEAD_BATCH, PQ, VW>, k_rshard_cand<M, TAIL_BATCH, PQ, VW>),
                       grid, dim3(256), lds, s, a);
    return (int)hipGetLastError();
  });
}

// ------------------------- sharded filtered ranking, the fast counting pass
// kge_rank_shard_fast: KGE_RSHARD_COUNT's counts from the single-table
// pipeline's fast pass run on the shard's view (ShardFastArgs): the counting
// tiles decide every owned candidate whose fast score clears the query's
// window around the GIVEN reference-order s_true, and list the rest.
//   k_rsf_prep     a wave per query: its state, the workspace's s_true, zeroed
//                  counters, and the fast q from fixed_rows[q] with k_rank_prep's
//                  load_row / build_q (RotatE with the caller's trig table: its
//                  rotation, the reference q's bits).  No table row is read.
//   k_rsf_window   a wave per query: the owned true row's bit into the shard's
//                  bitmap, then rank_window_body with fixed_rows[q] as the
//                  anchor row — the reference-order q and δ for true_exact.
//   k_rsf_finish   a workgroup per query: the listed candidates (or, past the
//                  list's cap, every owned row the bitmap leaves) scored in the
//                  reference's order by its half-waves from their LDS row slots
//                  and compared with s_true[q]; then the query's two counts.
//                  The true row is no item here and is never read.
template <int M, int MODE, int VEC, int NS>
__global__ __launch_bounds__(256) void k_rsf_prep(ShardFastArgs a) {
  constexpr bool CPLX = Traits<M>::cplx;
  using R_ = Row<NS, VEC, CPLX>;
  const RefArgs& f = a.r;
  const int lane = threadIdx.x & 63;
  const int64_t qi = (int64_t)blockIdx.x * 4 + wave_id();
  if (qi >= f.nq) return;
  Consts c = f.c;
  if constexpr (M == PROTATE) c.modulus = f.modulus[0];
  const int64_t h = f.queries[qi * 3], r = f.queries[qi * 3 + 1], t = f.queries[qi * 3 + 2];
  const int64_t te = (MODE == HEAD_BATCH) ? h : t;
  const bool bad = h < 0 || h >= a.E_glob || t < 0 || t >= a.E_glob || r < 0 || r >= f.R;
  if (lane == 0) {
    const int64_t tl = te - a.own_lo;
    a.state_w[qi] = bad ? -1 : ((tl >= 0 && tl < f.E) ? tl : f.E);
    a.s_true_w[qi] = bad ? NAN : a.s_true_in[qi];
    a.gt_w[qi] = 0;
    a.ucnt_w[qi] = 0;
    if (bad) atomicOr(f.err, KGE_DEVERR_INDEX);
  }
  if (bad) return;
  R_ q, xr, rr;
  load_row<NS, VEC, CPLX>(a.fixed_rows + qi * f.Le, a.eg, lane, xr);
  bool built = false;
  if constexpr (M == ROTATE) {
    if (f.trig) {  // (as k_rank_prep) q equals the window's reference q bit for bit
      const float* tr = f.trig + r * 2 * f.Lr;
      load_phase<NS, VEC>(tr, a.eg.S, lane, rr.a);
      load_phase<NS, VEC>(tr + f.Lr, a.eg.S, lane, rr.b);
#pragma unroll
      for (int s = 0; s < NS; ++s)
#pragma unroll
        for (int v = 0; v < VEC; ++v)
          Elem<M, MODE>::rotate(xr.a[s][v], xr.b[s][v], rr.a[s][v], rr.b[s][v], q.a[s][v], q.b[s][v]);
      built = true;
    }
  }
  if (!built) {
    load_rel<M, NS, VEC, CPLX>(f.rel + r * f.Lr, a.eg, lane, rr);
    build_q<M, MODE, NS, VEC, CPLX>(xr, rr, c, q);
  }
  store_row<NS, VEC, CPLX>(a.q_w + qi * f.Le, a.eg, lane, q);
}

template <int M, int MODE>
__global__ __launch_bounds__(256) void k_rsf_window(ShardFastArgs a) {
  const int64_t qi = (int64_t)blockIdx.x * 4 + wave_id();
  if (qi >= a.r.nq) return;
  const int64_t tl = a.r.true_id[qi];
  if ((threadIdx.x & 63) == 0 && tl >= 0 && tl < a.r.E) atomicOr(&a.bits_w[qi * a.r.W + (tl >> 5)], 1u << (tl & 31));
  rank_window_body<M, MODE>(a.r, qi, qi, a.fixed_rows + qi * a.r.Le);
  // an infinite s_true: score − s_true is NaN for a score of the same infinity, which no window catches and the
  // exact stage counts as a tie — mark the list as overflowed, so k_rsf_finish rescans the own rows
  if ((threadIdx.x & 63) == 0 && tl >= 0 && __builtin_isinf(a.r.s_true[qi])) a.ucnt_w[qi] = a.r.cap + 1;
}

template <int M, int MODE>
__global__ __launch_bounds__(256) void k_rsf_finish(ShardFastArgs a) {
  extern __shared__ __attribute__((aligned(16))) float fsm[];
  const RefArgs& f = a.r;
  const int tid = threadIdx.x, hl = tid & 31, half = tid >> 5;
  const int64_t qi = blockIdx.x;
  const bool ok = f.true_id[qi] >= 0;  // (block-uniform)
  const int n = ok ? f.ucnt[qi] : 0;
  const int64_t gt0 = ok ? f.gt[qi] : 0;
  if (n == 0) {  // nothing listed: the counting pass's count is final (a bad query: 0 / 0)
    if (tid == 0) {
      a.counts[qi] = gt0;
      a.counts[f.nq + qi] = 0;
      if (a.listed) a.listed[qi] = 0;
    }
    return;
  }
  Consts c = f.c;
  if constexpr (M == PROTATE) c.modulus = f.modulus[0];
  const int Le = f.Le, Lp = refine_lp(Le);
  const int ns = a.in_place ? 8 : a.nslot;
  float* slots = fsm + Lp;
  int* cnt_s = reinterpret_cast<int*>(fsm + (a.in_place ? 0 : Lp * (1 + ns)));
  const float* qr = f.qref + qi * Le;
  if (!a.in_place)
    for (int k = tid; k < Le; k += 256) fsm[k] = qr[k];
  if (tid < 2) cnt_s[tid] = 0;
  __syncthreads();
  const float* qs = a.in_place ? qr : fsm;
  const float st = f.s_true[qi];
  const bool ovf = n > f.cap;  // the list overflowed: every owned row the bitmap leaves
  const int64_t items = ovf ? f.E : (int64_t)n;
  const int32_t* lst = f.ulist + qi * (int64_t)f.cap;
  const uint32_t* bits = f.fbits + qi * f.W;
  const bool vec4 = ((Le & 3) == 0) && ((((uintptr_t)f.ent) & 15) == 0);
  int g = 0, e_ = 0;
  if (half < ns) {
    float* const row_l = slots + half * Lp;
    for (int64_t j = half; j < items; j += ns) {
      const int64_t e = ovf ? j : (int64_t)lst[j];
      bool valid = e >= 0 && e < f.E;
      if (ovf && valid) valid = ((bits[e >> 5] >> (e & 31)) & 1u) == 0u;
      if (!valid) continue;  // (uniform in the half-wave, whose shuffles stay inside it)
      const float* row = f.ent + e * Le;
      if (!a.in_place) {
        if (vec4) stage_row<4>(row, row_l, Le >> 2, hl);
        else stage_row<1>(row, row_l, Le, hl);
        // the half's lanes read each other's writes: one wave's LDS operations complete in order
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        row = row_l;
      }
      // (the score depends on every element of the row through the shuffles,
      // so the row's reads are done before the next item overwrites it)
      const float sc = ref_score_half<M, MODE>(qs, row, f.K, c, hl);
      g += (sc > st);
      e_ += (sc == st);
    }
    if (hl == 0 && (g | e_)) {  // integer sums: any order gives the same counts
      atomicAdd(&cnt_s[0], g);
      atomicAdd(&cnt_s[1], e_);
    }
  }
  __syncthreads();
  if (tid == 0) {
    a.counts[qi] = (ovf ? 0 : gt0) + cnt_s[0];
    a.counts[f.nq + qi] = cnt_s[1];
    if (a.listed) a.listed[qi] = n;
  }
}

// stage 1 (k_rsf_window) and 2 (k_rsf_finish); stage 0 goes through the row dispatch (RunShardFast)
template <int M>
int launch_rank_shard_fast(int mode, int stage, const ShardFastArgs& a, hipStream_t s) {
  if (stage == 1) {
    hipLaunchKernelGGL(pick_dir(mode, k_rsf_window<M, HEAD_BATCH>, k_rsf_window<M, TAIL_BATCH>),
                       dim3((unsigned)((a.r.nq + 3) / 4)), dim3(256), 0, s, a);
    return (int)hipGetLastError();
  }
  if (stage != 2) return -1;
  ShardFastArgs b = a;
  const int Lp = refine_lp(a.r.Le);
  b.nslot = rsf_slots(a.r.Le);
  b.in_place = b.nslot == 0;
  const size_t lds = sizeof(float) * (size_t)((b.in_place ? 0 : Lp * (1 + b.nslot)) + 4);
  hipLaunchKernelGGL(pick_dir(mode, k_rsf_finish<M, HEAD_BATCH>, k_rsf_finish<M, TAIL_BATCH>), dim3((unsigned)a.r.nq),
                     dim3(256), lds, s, b);
  return (int)hipGetLastError();
}

// ------------------------------------------------------------ dispatch
template <int M, int MODE, int VEC, int NS>
struct Launch {
  static int score(const ScoreArgs& a, int64_t units, hipStream_t s) {
    const unsigned grid = (unsigned)((units + 3) / 4);
    hipLaunchKernelGGL((k_score<M, MODE, VEC, NS>), dim3(grid), dim3(256), 0, s, a);
    return (int)hipGetLastError();
  }
  // (RowStage::Pass is launched first: the GPU starts on the big kernel while
  // the host issues the rest)
  static int row(RowStage stage, const RowArgs& a, size_t lds, hipStream_t s) {
    const dim3 rows((unsigned)a.B), quads((unsigned)((a.B + 3) / 4));
    switch (stage) {
      case RowStage::ShipQ:
        hipLaunchKernelGGL((k_ship_q<M, MODE, VEC, NS>), quads, dim3(256), 0, s, a);
        break;
      case RowStage::ShipRows:
        hipLaunchKernelGGL((k_row<M, MODE, VEC, NS, false, true>), rows, dim3(256), lds, s, a);
        break;
      case RowStage::ShipMerge:
        hipLaunchKernelGGL((k_ship_merge<M, MODE, VEC, NS>), rows, dim3(256), 0, s, a);
        break;
      case RowStage::ShipChain:
        hipLaunchKernelGGL((k_ship_chain<M, MODE, VEC, NS>), rows, dim3(256), 0, s, a);
        break;
      case RowStage::QOnly:
        hipLaunchKernelGGL((k_build_q<M, MODE, VEC, NS>), quads, dim3(256), 0, s, a);
        break;
      case RowStage::Epilogue:
        if (a.fuse_epi) return 0;  // done in k_row's tail
        hipLaunchKernelGGL((k_row_epi<M, MODE, VEC, NS>), rows, dim3(256), 0, s, a);
        break;
      case RowStage::Pass:
        if (a.timer_mid) a.timer_mid(s);
        if (a.fuse_epi)
          hipLaunchKernelGGL((k_row<M, MODE, VEC, NS, true>), rows, dim3(256), lds, s, a);
        else
          hipLaunchKernelGGL((k_row<M, MODE, VEC, NS, false>), rows, dim3(256), lds, s, a);
        break;
    }
    return (int)hipGetLastError();
  }
  // column-sliced pass for float4 rows; the row-per-wave pass otherwise
  // opt (OptKind): the fused optimizer's rule; Adagrad only with the lazy rows
  static int entity(const EntArgs& a, int opt, hipStream_t s) {
    if (opt != OPT_ADAM && !a.rows) return -1;
    if constexpr (VEC == 4) {
      if (a.nsl > 0) {
        const int64_t ne = a.e_end - a.e_begin;  // (lazy: the row places, kge_capi.hip run_grad)
        const unsigned gs = (unsigned)(a.nsl * ((ne + 3) / 4)) + ent_lead_blocks(a);
        if (opt == OPT_ADAGRAD) {
          if (a.q_sl)
            hipLaunchKernelGGL((k_entity_sl<M, MODE, true, true, OPT_ADAGRAD>), dim3(gs), dim3(256), 0, s, a);
          else
            hipLaunchKernelGGL((k_entity_sl<M, MODE, false, true, OPT_ADAGRAD>), dim3(gs), dim3(256), 0, s, a);
          return (int)hipGetLastError();
        }
        if (opt != OPT_ADAM) return -1;  // (the row-wise kind is planned unsliced)
        if (a.rows) {
          if (a.q_sl)
            hipLaunchKernelGGL((k_entity_sl<M, MODE, true, true>), dim3(gs), dim3(256), 0, s, a);
          else
            hipLaunchKernelGGL((k_entity_sl<M, MODE, false, true>), dim3(gs), dim3(256), 0, s, a);
          return (int)hipGetLastError();
        }
        if (a.q_sl)
          hipLaunchKernelGGL((k_entity_sl<M, MODE, true>), dim3(gs), dim3(256), 0, s, a);
        else
          hipLaunchKernelGGL((k_entity_sl<M, MODE, false>), dim3(gs), dim3(256), 0, s, a);
        return (int)hipGetLastError();
      }
    }
    const unsigned grid = (unsigned)((a.e_end - a.e_begin + 3) / 4);
    if (opt == OPT_ADAGRAD) {
      hipLaunchKernelGGL((k_entity<M, MODE, VEC, NS, true, OPT_ADAGRAD>), dim3(grid), dim3(256), 0, s, a);
      return (int)hipGetLastError();
    }
    if (opt == OPT_ADAGRAD_ROW) {
      hipLaunchKernelGGL((k_entity<M, MODE, VEC, NS, true, OPT_ADAGRAD_ROW>), dim3(grid), dim3(256), 0, s, a);
      return (int)hipGetLastError();
    }
    if (a.rows) {
      hipLaunchKernelGGL((k_entity<M, MODE, VEC, NS, true>), dim3(grid), dim3(256), 0, s, a);
      return (int)hipGetLastError();
    }
    hipLaunchKernelGGL((k_entity<M, MODE, VEC, NS>), dim3(grid), dim3(256), 0, s, a);
    return (int)hipGetLastError();
  }
  static int rank(const RankArgs& a, hipStream_t s) {
    const unsigned gq = (unsigned)((a.nq + 3) / 4);
    if (a.both_dirs) {  // (prep only) both directions' q in one launch
      if (!a.prep_only) return -1;
      hipLaunchKernelGGL((k_rank_prep<M, BOTH_DIRS, VEC, NS>), dim3(2 * gq), dim3(256), 0, s, a);
      return (int)hipGetLastError();
    }
    hipLaunchKernelGGL((k_rank_prep<M, MODE, VEC, NS>), dim3(gq), dim3(256), 0, s, a);
    int st = (int)hipGetLastError();
    if (st || a.prep_only) return st;
    const int64_t chunks = (a.E + a.cpw - 1) / a.cpw;
    const unsigned gs = (unsigned)((a.nq * chunks + 3) / 4);
    hipLaunchKernelGGL((k_rank_scan<M, MODE, VEC, NS>), dim3(gs), dim3(256), 0, s, a);
    return (int)hipGetLastError();
  }
};

#include "kge_wide.inc"

// Pick (MODE, VEC, NS) at run time.  VEC=4 needs 16-byte aligned slots
// (row lengths divisible by 4, and by 8 for the complex halves); NS is the
// smallest supported count with 64*NS*VEC >= the slot span.  Both cover
// spans up to 2048 floats per (half-)row: VEC=4 with NS ≤ 8, VEC=1 (any
// hidden_dim, e.g. an odd one) with NS ≤ 32 — the wide single-float rows
// hold more registers per lane and run at lower occupancy, but every kernel
// keeps its structure and its fixed summation order.
template <int M, template <int, int, int, int> class F, typename... Args>
int dispatch(int mode, int vec, int ns, Args&&... args) {
#define KGE_NS_CASES(MODE_, VEC_)                                                         \
  switch (ns) {                                                                            \
    case 1: return F<M, MODE_, VEC_, 1>::run(std::forward<Args>(args)...);                \
    case 2: return F<M, MODE_, VEC_, 2>::run(std::forward<Args>(args)...);                \
    case 4: return F<M, MODE_, VEC_, 4>::run(std::forward<Args>(args)...);                \
    case 8: return F<M, MODE_, VEC_, 8>::run(std::forward<Args>(args)...);                \
    default: break;                                                                        \
  }
#define KGE_NS_WIDE(MODE_)                                                                 \
  switch (ns) {                                                                            \
    case 16: return F<M, MODE_, 1, 16>::run(std::forward<Args>(args)...);                 \
    case 32: return F<M, MODE_, 1, 32>::run(std::forward<Args>(args)...);                 \
    default: return -1;                                                                    \
  }
  if (ns == 0)  // rows wider than any register tile (kge_wide.inc)
    return (mode == HEAD_BATCH) ? F<M, HEAD_BATCH, 1, 0>::run(std::forward<Args>(args)...)
                                : F<M, TAIL_BATCH, 1, 0>::run(std::forward<Args>(args)...);
  if (mode == HEAD_BATCH) {
    if (vec == 4) { KGE_NS_CASES(HEAD_BATCH, 4) return -1; } else { KGE_NS_CASES(HEAD_BATCH, 1) KGE_NS_WIDE(HEAD_BATCH) }
  } else {
    if (vec == 4) { KGE_NS_CASES(TAIL_BATCH, 4) return -1; } else { KGE_NS_CASES(TAIL_BATCH, 1) KGE_NS_WIDE(TAIL_BATCH) }
  }
#undef KGE_NS_CASES
#undef KGE_NS_WIDE
}

template <int M, int MODE, int VEC, int NS>
struct RunScore { static int run(const ScoreArgs& a, int64_t u, hipStream_t s) { return Launch<M, MODE, VEC, NS>::score(a, u, s); } };
template <int M, int MODE, int VEC, int NS>
struct RunRow { static int run(RowStage stage, const RowArgs& a, size_t l, hipStream_t s) { return Launch<M, MODE, VEC, NS>::row(stage, a, l, s); } };
template <int M, int MODE, int VEC, int NS>
struct RunEntity { static int run(const EntArgs& a, int opt, hipStream_t s) { return Launch<M, MODE, VEC, NS>::entity(a, opt, s); } };
template <int M, int MODE, int VEC, int NS>
struct RunRank { static int run(const RankArgs& a, hipStream_t s) { return Launch<M, MODE, VEC, NS>::rank(a, s); } };

template <int M, int MODE, int VEC, int NS>
struct RunTopk {
  static int run(const TopkArgs& a, hipStream_t s) {
    if constexpr (NS == 0) {
      return -1;  // rows wider than the register kernels hold: not served (KGE_ERR_DIM)
    } else {
      if (a.stage == 0) {
        hipLaunchKernelGGL((k_topk_prep<M, MODE, VEC, NS>), dim3((unsigned)((a.nq + 3) / 4)), dim3(256), 0, s, a);
      } else if (a.stage == 2) {
        hipLaunchKernelGGL((k_topk_prep_rows<M, MODE, VEC, NS>), dim3((unsigned)((a.nq + 3) / 4)), dim3(256), 0, s, a);
      } else {
        const int64_t units = a.nq * a.parts;
        hipLaunchKernelGGL((k_topk_scan<M, MODE, VEC, NS>), dim3((unsigned)((units + 3) / 4)), dim3(256), 0, s, a);
      }
      return (int)hipGetLastError();
    }
  }
};

template <int M, int MODE, int VEC, int NS>
struct RunShardFast {
  static int run(int stage, const ShardFastArgs& a, hipStream_t s) {
    if (stage != 0) return launch_rank_shard_fast<M>(MODE, stage, a, s);
    if constexpr (NS == 0) {
      return -1;  // rows wider than the register kernels hold: the entry resolves them to the exact stage
    } else {
      hipLaunchKernelGGL((k_rsf_prep<M, MODE, VEC, NS>), dim3((unsigned)((a.r.nq + 3) / 4)), dim3(256), 0, s, a);
      return (int)hipGetLastError();
    }
  }
};

template <int M>
struct ModelTable {
  static int rank_shard_fast(int mode, int vec, int ns, int stage, const ShardFastArgs& a, hipStream_t s) {
    return dispatch<M, RunShardFast>(mode, vec, ns, stage, a, s);
  }
  static int score(int mode, int vec, int ns, const ScoreArgs& a, int64_t u, hipStream_t s) {
    return dispatch<M, RunScore>(mode, vec, ns, a, u, s);
  }
  static int row(int mode, int vec, int ns, RowStage stage, const RowArgs& a, size_t l, hipStream_t s) {
    return dispatch<M, RunRow>(mode, vec, ns, stage, a, l, s);
  }
  static int entity(int mode, int vec, int ns, const EntArgs& a, int opt, hipStream_t s) {
    return dispatch<M, RunEntity>(mode, vec, ns, a, opt, s);
  }
  static int rank(int mode, int vec, int ns, const RankArgs& a, hipStream_t s) {
    return dispatch<M, RunRank>(mode, vec, ns, a, s);
  }
  static int topk(int mode, int vec, int ns, const TopkArgs& a, hipStream_t s) {
    return dispatch<M, RunTopk>(mode, vec, ns, a, s);
  }
};

}  // namespace kge

#define KGE_INSTANTIATE_MODEL(M, NAME)                                                            \
  namespace kge {                                                                                  \
  ModelOps model_ops_##NAME() {                                                                    \
    ModelOps o;                                                                                    \
    o.score = &ModelTable<M>::score;                                                               \
    o.row = &ModelTable<M>::row;                                                                   \
    o.entity = &ModelTable<M>::entity;                                                             \
    o.rank = &ModelTable<M>::rank;                                                                 \
    o.rank_tile = &launch_rank_tile<M>;                                                            \
    o.rank_ref = &launch_rank_ref<M>;                                                              \
    o.topk = &ModelTable<M>::topk;                                                                 \
    o.topk_tile = &launch_topk_tile<M>;                                                            \
    o.rank_cand = &launch_rank_cand<M>;                                                            \
    o.rank_rel = &launch_rank_rel<M>;                                                              \
    o.rank_shard = &launch_rank_shard<M>;                                                          \
    o.rank_shard_fast = &ModelTable<M>::rank_shard_fast;                                           \
    o.rank_cand_shard = &launch_rank_cand_shard<M>;                                                \
    return o;                                                                                      \
  }                                                                                                \
  }
