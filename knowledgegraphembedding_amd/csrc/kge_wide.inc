// kge_wide.inc — rows wider than the register-tiled kernels hold (more than
// 2048 floats per (half-)row; check_model's ns = 0).  The reference accepts any
// hidden_dim (model.py:42-45); these are the same passes as kge_kernels.inc's
// with the row walked in a run-time loop of single-float elements instead of
// NS register slots per lane: Launch<M, MODE, 1, 0> below.
//
//   k_score_w      forward scores (kge_score), one wave per (row, candidate chunk)
//   k_build_q_w    q rows alone (the factor exchange's global step)
//   k_row_w        the training / backward row pass, one workgroup per positive
//                  row: q, every negative's score (raw totals in LDS), the
//                  self-adversarial softmax and loss terms (model.py:268-288),
//                  dL/ds, dL/dq (a second walk over the gathered rows), then the
//                  positive score and the chain rule (row_epilogue, NS = 0)
//   k_entity_w     the entity-major gradient + fused Adam, one wave per (entity,
//                  one of WIDE_PARTS column parts)
//   k_rank_prep_w / k_rank_scan_w   ranking: q, the fast true score, and the
//                  wave-scan counting pass (the tile / MFMA passes take any K)
//
// Sums run in a fixed order — lane-strided partial sums, then the DPP wave sum
// or a fixed block tree — so every result is deterministic; the orders are not
// the register-tiled kernels' (no row fits both).  The ranking windows
// (k_rank_window) assume any order for the fast pass, so ranks stay exact.
// Performance is not the point here: every row is read twice in the row pass
// and the q build is evaluated per candidate in the forward scores.

// (included inside namespace kge, after the primary Launch template)

// element k of a (half-)row of S elements: (re, im) at k and half + k
template <int M>
__device__ __forceinline__ void wide_ent(const float* row, int64_t k, int half, float& a, float& b) {
  a = row[k];
  b = Traits<M>::cplx ? row[half + k] : 0.f;
}
template <int M>
__device__ __forceinline__ void wide_rel(const float* row, int64_t k, int half, float& a, float& b) {
  a = row[k];
  b = (Traits<M>::cplx && !Traits<M>::rel_phase) ? row[half + k] : 0.f;
}

// ------------------------------------------------------------------ forward
template <int M, int MODE>
__global__ __launch_bounds__(256) void k_score_w(ScoreArgs a) {
  using EL = Elem<M, MODE>;
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
  const float* xr = a.ent + x * a.Le;
  const float* rr = a.rel + r * a.Lr;
  const int S = a.eg.S, hf = a.eg.half;
  const int64_t* nb = a.neg + i * a.neg_stride;
  for (int64_t j = j0; j < j1; ++j) {
    int64_t e = nb[j];
    if (e < 0 || e >= a.E) {
      if (lane == 0) atomicOr(a.err, KGE_DEVERR_INDEX);
      e = 0;
    }
    const float* er = a.ent + e * a.Le;
    float part = 0.f;
    for (int k = lane; k < S; k += 64) {
      float xa, xb, ra, rb, ea, eb, qa, qb;
      wide_ent<M>(xr, k, hf, xa, xb);
      wide_rel<M>(rr, k, hf, ra, rb);
      wide_ent<M>(er, k, hf, ea, eb);
      EL::make_q(xa, xb, ra, rb, c, qa, qb);
      part += EL::phi(qa, qb, ea, eb, c);
    }
    const float tot = wave_sum(part);
    if (lane == 0) out[j] = EL::finish(tot, c);
  }
}

// ------------------------------------------------------------- row pass
template <int M, int MODE>
__device__ __forceinline__ void wide_q_row(const RowArgs& a, int64_t i, const Consts& c, int t0, int stride) {
  using EL = Elem<M, MODE>;
  const int64_t h = a.pos[i * 3], r = a.pos[i * 3 + 1], t = a.pos[i * 3 + 2];
  const int64_t x = (MODE == HEAD_BATCH) ? t : h;
  const bool bad = (h < 0 || h >= a.E || t < 0 || t >= a.E || r < 0 || r >= a.R);
  if (bad && t0 == 0) atomicOr(a.err, KGE_DEVERR_INDEX);
  const int S = a.eg.S, hf = a.eg.half;
  float* qo = a.q_out + i * a.Le;
  const float* xr = a.ent + (bad ? 0 : x) * a.Le;
  const float* rr = a.rel + (bad ? 0 : r) * a.Lr;
  for (int k = t0; k < S; k += stride) {
    float xa, xb, ra, rb, qa = 0.f, qb = 0.f;
    if (!bad) {
      wide_ent<M>(xr, k, hf, xa, xb);
      wide_rel<M>(rr, k, hf, ra, rb);
      EL::make_q(xa, xb, ra, rb, c, qa, qb);
    }
    qo[k] = qa;
    if constexpr (Traits<M>::cplx) qo[hf + k] = qb;
  }
}

template <int M, int MODE>
__global__ __launch_bounds__(256) void k_build_q_w(RowArgs a) {
  if (a.wsum_out && blockIdx.x == 0) {
    __shared__ float red[256];
    const float tot = block_weight_sum(a.sub_w, a.B, red);
    if (threadIdx.x == 0) a.wsum_out[0] = tot;
  }
  const int64_t i = (int64_t)blockIdx.x * 4 + wave_id();
  if (i >= a.B) return;
  Consts c = a.c;
  if constexpr (M == PROTATE) c.modulus = a.modulus[0];
  wide_q_row<M, MODE>(a, i, c, threadIdx.x & 63, 64);
}

// fixed-order block reductions over 256 threads (tree in LDS)
__device__ __forceinline__ float block_max256(float v, float* red) {
  red[threadIdx.x] = v;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] = fmaxf(red[threadIdx.x], red[threadIdx.x + o]);
    __syncthreads();
  }
  const float r = red[0];
  __syncthreads();
  return r;
}
__device__ __forceinline__ float block_sum256(float v, float* red) {
  red[threadIdx.x] = v;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  const float r = red[0];
  __syncthreads();
  return r;
}

// Dynamic LDS: [n] raw totals, later overwritten by each negative's dq weight.
template <int M, int MODE>
__global__ __launch_bounds__(256) void k_row_w(RowArgs a) {
  using EL = Elem<M, MODE>;
  extern __shared__ __attribute__((aligned(16))) float tl[];
  __shared__ float red[256];
  __shared__ float gp_s;
  const int tid = threadIdx.x, lane = tid & 63, w = wave_id();
  const int64_t i = blockIdx.x;
  const bool train = (a.op == ROW_TRAIN);
  const bool adv = train && a.adversarial;
  Consts c = a.c;
  if constexpr (M == PROTATE) c.modulus = a.modulus[0];
  float ci = 1.f;
  if (train && !a.uni_weight) {
    float wsum;
    if (a.wsum_out) {
      wsum = block_weight_sum(a.sub_w, a.B, red);
      if (blockIdx.x == 0 && tid == 0) a.wsum_out[0] = wsum;
    } else {
      wsum = a.w_sum[0];
    }
    ci = a.sub_w[i] / wsum;
  } else if (train) {
    ci = a.uni_inv;
  }
  __syncthreads();
  // q_i to global memory (read back below, and by the entity pass)
  wide_q_row<M, MODE>(a, i, c, tid, 256);
  __syncthreads();
  const int S = a.eg.S, hf = a.eg.half;
  const float* q = a.q_out + i * a.Le;
  const int64_t* nb = a.neg + i * a.neg_stride;
  auto row_of = [&](int64_t j) -> const float* {
    int64_t e = nb[j];
    if (e < 0 || e >= a.E) {
      if (lane == 0) atomicOr(a.err, KGE_DEVERR_INDEX);
      e = 0;
    }
    return a.ent + e * a.Le;
  };
  // raw totals Σ_k phi of every negative (wave w: j ≡ w mod 4)
  for (int64_t j = w; j < a.n; j += 4) {
    const float* er = row_of(j);
    float part = 0.f;
    for (int k = lane; k < S; k += 64) {
      float qa, qb, ea, eb;
      wide_ent<M>(q, k, hf, qa, qb);
      wide_ent<M>(er, k, hf, ea, eb);
      part += EL::phi(qa, qb, ea, eb, c);
    }
    const float tot = wave_sum(part);
    if (lane == 0) tl[j] = tot;
  }
  __syncthreads();
  // softmax statistics (model.py:272-288) in a fixed order: each thread its
  // strided negatives in ascending order, then the block tree
  const float T = a.adv_T;
  float Mx = 0.f;
  if (adv) {
    float mx = -INFINITY;
    for (int64_t j = tid; j < a.n; j += 256) mx = fmaxf(mx, T * EL::finish(tl[j], c));
    Mx = block_max256(mx, red);
  }
  float z = 0.f, nl = 0.f, mg = 0.f;
  for (int64_t j = tid; j < a.n; j += 256) {
    const float tot = tl[j], s = EL::finish(tot, c);
    if (train) {
      const float p = adv ? expf(T * s - Mx) : 1.f;
      z += p;
      nl += p * log_sigmoid(-s);
      mg += p * sigmoidf(s) * (-tot);
    } else {
      mg += a.g_in[i * a.n + j] * (-tot);
    }
  }
  const float Zt = block_sum256(z, red);
  const float NLt = block_sum256(nl, red);
  const float MGt = block_sum256(mg, red);
  const float nf = (float)a.n;
  // each negative's weight in dL/dq (cv_j, before the row's scale) and dL/ds_ij
  for (int64_t j = tid; j < a.n; j += 256) {
    const float s = EL::finish(tl[j], c);
    float cv;
    if (train) {
      const float p = adv ? expf(T * s - Mx) : 1.f;
      cv = p * sigmoidf(s);
      a.g_out[i * a.n + j] = 0.5f * ci * (adv ? (p / Zt) : (1.f / nf)) * sigmoidf(s);
    } else {
      cv = a.g_in[i * a.n + j];
    }
    tl[j] = cv;
  }
  if (tid == 0) {
    a.row_stats[i * 4 + 1] = train ? (adv ? (NLt / Zt) : (NLt / nf)) : 0.f;
    a.row_stats[i * 4 + 2] = train ? (0.5f * ci * MGt / (adv ? Zt : nf)) : MGt;
  }
  __syncthreads();
  // dL/dq = scale · Σ_j cv_j ∂s_ij/∂q, element by element (the gathered rows again)
  const float vscale = train ? (adv ? (0.5f * ci / Zt) : (0.5f * ci / nf)) : 1.f;
  float* dq = a.dq_out + i * a.Le;
  for (int k = tid; k < S; k += 256) {
    float qa, qb;
    wide_ent<M>(q, k, hf, qa, qb);
    float va = 0.f, vb = 0.f;
    for (int64_t j = 0; j < a.n; ++j) {
      int64_t e = nb[j];
      e = (e < 0 || e >= a.E) ? 0 : e;
      float ea, eb, da, db;
      wide_ent<M>(a.ent + e * a.Le, k, hf, ea, eb);
      EL::phi_dir(qa, qb, ea, eb, c);
      EL::dq_of(ea, eb, tl[j], c, da, db);
      va += da;
      vb += db;
    }
    dq[k] = va * vscale;
    if constexpr (Traits<M>::cplx) dq[hf + k] = vb * vscale;
  }
  if (a.fuse_epi) {
    __syncthreads();
    row_epilogue<M, MODE, 1, 0>(a, i, dq, &gp_s, train ? ci : -1.f);
  }
}

// ------------------------------------------------------- entity-major pass
// One wave per (entity e, column part p): elements [p·W, min(S, (p+1)·W)) of
// the (half-)row, W = a.slice_w, four per lane per sweep; each sweep walks
// the entity's occurrences (CSR, ascending) in chunks of 64, negatives first
// as in k_entity.  Gradient written densely; fused Adam when a.adam.p.
template <int M, int MODE>
__global__ __launch_bounds__(256) void k_entity_w(EntArgs a) {
  using EL = Elem<M, MODE>;
  constexpr bool CPLX = Traits<M>::cplx;
  const int lane = threadIdx.x & 63;
  const int64_t unit = (int64_t)blockIdx.x * 4 + wave_id();
  const int64_t e = a.e_begin + unit / a.nsl;
  const int p = (int)(unit % a.nsl);
  if (e >= a.e_end) return;
  Consts c = a.c;
  if constexpr (M == PROTATE) c.modulus = a.modulus[0];
  const int S = a.eg.S, hf = a.eg.half;
  const int k_lo = p * a.slice_w;
  const int k_hi = (k_lo + a.slice_w < S) ? (k_lo + a.slice_w) : S;
  const float* erow = a.ent + e * a.Le;
  const int32_t b0 = a.off[e], b1 = a.off[e + 1];
  const uint32_t n32 = (uint32_t)a.n;
  float regp = 0.f;
  for (int kb = k_lo; kb < k_hi; kb += 256) {
    float ea[4], eb[4], ga[4], gb[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int k = kb + lane + 64 * u;
      ea[u] = eb[u] = ga[u] = gb[u] = 0.f;
      if (k < k_hi) wide_ent<M>(erow, k, hf, ea[u], eb[u]);
    }
    for (int32_t c0 = b0; c0 < b1; c0 += 64) {
      const int cnt = (b1 - c0 < 64) ? (b1 - c0) : 64;
      const int32_t o_l = (lane < cnt) ? a.occ[c0 + lane] : 0x7fffffff;
      const bool neg_l = o_l < a.Bn;
      const uint32_t i_l = neg_l ? ((uint32_t)o_l / n32) : 0u;
      const float g_l = neg_l ? a.g[o_l] : 0.f;
      const int nneg = __popcll(__ballot(neg_l && lane < cnt));
      for (int pp = 0; pp < nneg; ++pp) {
        const uint32_t iq = (uint32_t)__builtin_amdgcn_readlane((int)i_l, pp);
        const float g = readlanef(g_l, pp);
        const float* qrow = a.q + (int64_t)iq * a.Le;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int k = kb + lane + 64 * u;
          if (k >= k_hi) continue;
          float qa, qb, gqa, gqb, gea, geb;
          wide_ent<M>(qrow, k, hf, qa, qb);
          EL::grads(qa, qb, ea[u], eb[u], c, gqa, gqb, gea, geb);
          ga[u] += g * gea;
          if constexpr (CPLX) gb[u] += g * geb;
        }
      }
      for (int pp = nneg; pp < cnt; ++pp) {
        const int32_t o = __builtin_amdgcn_readlane(o_l, pp);
        const float* cr = a.ent_contrib + (int64_t)(o - a.Bn) * a.Le;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int k = kb + lane + 64 * u;
          if (k >= k_hi) continue;
          float xa, xb;
          wide_ent<M>(cr, k, hf, xa, xb);
          ga[u] += xa;
          if constexpr (CPLX) gb[u] += xb;
        }
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int k = kb + lane + 64 * u;
      if (k >= k_hi) continue;
      if (a.reg3 != 0.f) {
        ga[u] += a.reg3 * (ea[u] * fabsf(ea[u]));
        regp += fabsf(ea[u]) * ea[u] * ea[u];
        if constexpr (CPLX) {
          gb[u] += a.reg3 * (eb[u] * fabsf(eb[u]));
          regp += fabsf(eb[u]) * eb[u] * eb[u];
        }
      }
      const int64_t o0 = e * a.Le + k, o1 = e * a.Le + hf + k;
      if (a.write_grad) {
        a.grad_ent[o0] = ga[u];
        if constexpr (CPLX) a.grad_ent[o1] = gb[u];
      }
      if (a.adam.p) {
        float pv = ea[u], mv = a.adam.m[o0], vv = a.adam.v[o0];
        adam_elem(pv, ga[u], mv, vv, a.adamk, a.adam.step_size, a.adam.bc2s);
        a.adam.p[o0] = pv; a.adam.m[o0] = mv; a.adam.v[o0] = vv;
        if constexpr (CPLX) {
          float pw = eb[u], mw = a.adam.m[o1], vw = a.adam.v[o1];
          adam_elem(pw, gb[u], mw, vw, a.adamk, a.adam.step_size, a.adam.bc2s);
          a.adam.p[o1] = pw; a.adam.m[o1] = mw; a.adam.v[o1] = vw;
        }
      }
    }
  }
  if (a.reg3 != 0.f) {
    regp = wave_sum(regp);
    if (lane == 0) a.reg_partial[e * a.nsl + p] = regp;
  }
}

// ------------------------------------------------------------- ranking
template <int M, int MODE>
__global__ __launch_bounds__(256) void k_rank_prep_w(RankArgs a) {
  using EL = Elem<M, MODE>;
  const int lane = threadIdx.x & 63;
  const int64_t qi = (int64_t)blockIdx.x * 4 + wave_id();
  if (qi >= a.nq) return;
  if (a.zero_counts && lane < 6) a.gt[lane * a.cstride + qi] = 0;
  Consts c = a.c;
  if constexpr (M == PROTATE) c.modulus = a.modulus[0];
  const int64_t h = a.queries[qi * 3], r = a.queries[qi * 3 + 1], t = a.queries[qi * 3 + 2];
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
  const int S = a.eg.S, hf = a.eg.half;
  const float* xr = a.ent + x * a.Le;
  const float* rr = a.rel + r * a.Lr;
  const float* er = a.ent + ev * a.Le;
  const float* tr = (M == ROTATE && a.trig) ? a.trig + r * 2 * a.Lr : nullptr;
  float* qo = a.q + qi * a.Le;
  float part = 0.f;
  for (int k = lane; k < S; k += 64) {
    float xa, xb, ra, rb, qa, qb, ea, eb;
    wide_ent<M>(xr, k, hf, xa, xb);
    if constexpr (M == ROTATE) {
      if (tr) {  // the caller's reference cos | sin (kge_model_desc.relation_trig)
        EL::rotate(xa, xb, tr[k], tr[a.Lr + k], qa, qb);
      } else {
        wide_rel<M>(rr, k, hf, ra, rb);
        EL::make_q(xa, xb, ra, rb, c, qa, qb);
      }
    } else {
      wide_rel<M>(rr, k, hf, ra, rb);
      EL::make_q(xa, xb, ra, rb, c, qa, qb);
    }
    qo[k] = qa;
    if constexpr (Traits<M>::cplx) qo[hf + k] = qb;
    wide_ent<M>(er, k, hf, ea, eb);
    part += EL::phi(qa, qb, ea, eb, c);
  }
  const float tot = wave_sum(part);
  if (lane == 0) {
    a.s_true[qi] = EL::finish(tot, c);
    a.true_id[qi] = ev;
  }
}

template <int M, int MODE>
__global__ __launch_bounds__(256) void k_rank_scan_w(RankArgs a) {
  using EL = Elem<M, MODE>;
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
  const int S = a.eg.S, hf = a.eg.half;
  const float* q = a.q + qi * a.Le;
  int gt = 0;
  for (int64_t e = c0; e < c1; ++e) {
    if (filter_bit(bits, e)) continue;  // wave-uniform
    const float* er = a.ent + e * a.Le;
    float part = 0.f;
    for (int k = lane; k < S; k += 64) {
      float qa, qb, ea, eb;
      wide_ent<M>(q, k, hf, qa, qb);
      wide_ent<M>(er, k, hf, ea, eb);
      part += EL::phi(qa, qb, ea, eb, c);
    }
    const float s0 = EL::finish(wave_sum(part), c);
    if (lane == 0) win_count(a.win, qi, e, s0, st, dlt, gt);
  }
  if (lane == 0 && gt) atomicAdd(&a.gt[qi], gt);
}

// The wide forms behind the same dispatch (check_model's ns = 0).
template <int M, int MODE>
struct Launch<M, MODE, 1, 0> {
  static int score(const ScoreArgs& a, int64_t units, hipStream_t s) {
    hipLaunchKernelGGL((k_score_w<M, MODE>), dim3((unsigned)((units + 3) / 4)), dim3(256), 0, s, a);
    return (int)hipGetLastError();
  }
  static int row(RowStage stage, const RowArgs& a, size_t lds, hipStream_t s) {
    switch (stage) {
      case RowStage::ShipQ:
      case RowStage::ShipRows:
      case RowStage::ShipMerge:
      case RowStage::ShipChain:
        return -1;  // query shipping: not for wide rows
      case RowStage::QOnly:
        hipLaunchKernelGGL((k_build_q_w<M, MODE>), dim3((unsigned)((a.B + 3) / 4)), dim3(256), 0, s, a);
        break;
      case RowStage::Epilogue:
        if (a.fuse_epi) return 0;
        hipLaunchKernelGGL((k_row_epi<M, MODE, 1, 0>), dim3((unsigned)a.B), dim3(256), 0, s, a);
        break;
      case RowStage::Pass:
        if (a.timer_mid) a.timer_mid(s);
        hipLaunchKernelGGL((k_row_w<M, MODE>), dim3((unsigned)a.B), dim3(256), lds, s, a);
        break;
    }
    return (int)hipGetLastError();
  }
  static int entity(const EntArgs& a, int opt, hipStream_t s) {
    if (a.nsl < 1 || opt != OPT_ADAM) return -1;  // (the lazy steps refuse wide rows)
    const int64_t units = (a.e_end - a.e_begin) * (int64_t)a.nsl;
    hipLaunchKernelGGL((k_entity_w<M, MODE>), dim3((unsigned)((units + 3) / 4)), dim3(256), 0, s, a);
    return (int)hipGetLastError();
  }
  static int rank(const RankArgs& a, hipStream_t s) {
    if (a.both_dirs) return -1;  // (one launch per direction for wide rows)
    hipLaunchKernelGGL((k_rank_prep_w<M, MODE>), dim3((unsigned)((a.nq + 3) / 4)), dim3(256), 0, s, a);
    int st = (int)hipGetLastError();
    if (st || a.prep_only) return st;
    const int64_t chunks = (a.E + a.cpw - 1) / a.cpw;
    hipLaunchKernelGGL((k_rank_scan_w<M, MODE>), dim3((unsigned)((a.nq * chunks + 3) / 4)), dim3(256), 0, s, a);
    return (int)hipGetLastError();
  }
};
