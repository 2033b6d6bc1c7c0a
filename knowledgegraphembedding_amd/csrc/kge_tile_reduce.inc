// kge_tile_reduce.inc — one 64 × 64 tile's reduction, the text of
// k_rank_tile's and tile_reduce's bodies (kge_kernels.inc; included inside a
// function, not a translation unit of its own).  Rows q0.. of q against rows
// e0.. of the table (GATHER: the rows arow / brow name, −1 for none), every
// pair's sum left in acc; ends on a barrier, so Qs / Es may be restaged at
// once.  The includer provides M, MODE, GATHER, C_ = TileCfg<M, SPLT>, T, BK,
// a (TileArgs), c (Consts), q0, e0, arow, brow, Qs, Es, acc and t, ty, tx.
  constexpr bool CPLX = C_::CPLX, PROT = C_::PROT, SPL = C_::SPL;
  constexpr int P = C_::P;
  // staging role: row sr, elements sk .. sk+3 of the slab (K % 4 == 0, so a
  // float4 is either wholly inside the row or wholly padding; padding terms
  // are phi(0, 0) = 0 for every model)
  const int sr = t >> 2, sk = (t & 3) * 4;
  const int64_t qrow = GATHER ? arow[sr] : 0, erow = GATHER ? brow[sr] : 0;  // (read by the gather pass only)
  // pRotatE reads the precomputed phase tables ([row][K][2], 2 float4 per
  // staged slot); complex rows their re and im halves; real rows one float4
  const float* qp = PROT ? a.qph + (qrow >= 0 ? qrow : 0) * (int64_t)(2 * a.K) + 2 * sk
                         : a.q + (qrow >= 0 ? qrow : 0) * (int64_t)a.Le + sk;
  const float* ep = PROT ? a.eph + (erow >= 0 ? erow : 0) * (int64_t)(2 * a.K) + 2 * sk
                         : a.ent + (erow >= 0 ? erow : 0) * (int64_t)a.Le + sk;
  constexpr int PF = PROT ? 2 : P;  // float4 loads per staged slot
  float4 rq[PF], re[PF];
  // counting pass: the block's 64 query rows and 64 candidate rows are each
  // contiguous, so one buffer descriptor per operand covers them and a row
  // past nq / E, or a slot past K, reads 0 from the hardware range check (its
  // offset set to the range's end) — no zero-fill moves and no branches
  const int64_t rlen = PROT ? 2 * (int64_t)a.K : a.Le;  // floats per staged row
  // (built in the gather pass too, where no load goes through them)
  const int64_t nqr = (a.nq - q0 < T) ? a.nq - q0 : T, ner = (a.E - e0 < T) ? a.E - e0 : T;
  const uint32_t qend = (uint32_t)(nqr * rlen * 4), eend = (uint32_t)((ner > 0 ? ner : 0) * rlen * 4);
  const auto qrs = buf_rsrc((PROT ? a.qph : a.q) + q0 * rlen, qend);
  const auto ers = buf_rsrc((PROT ? a.eph : a.ent) + (GATHER ? 0 : e0) * rlen, eend);
  auto fetch = [&](int k0) {
    const bool in = (k0 + sk) < a.K;
#pragma unroll
    for (int p = 0; p < PF; ++p) {
      const int64_t o = PROT ? (int64_t)2 * k0 + 4 * p : (int64_t)p * a.K + k0;
      if constexpr (GATHER) {
        rq[p] = (in && qrow >= 0) ? *reinterpret_cast<const float4*>(qp + o) : make_float4(0.f, 0.f, 0.f, 0.f);
        re[p] = (in && erow >= 0) ? *reinterpret_cast<const float4*>(ep + o) : make_float4(0.f, 0.f, 0.f, 0.f);
      } else {
        const uint32_t off = (uint32_t)((sr * rlen + (PROT ? 2 * sk : sk) + o) * 4);
        float x[4], y[4];
        buf_ld4(qrs, in ? off : qend, x);
        buf_ld4(ers, in ? off : eend, y);
        rq[p] = make_float4(x[0], x[1], x[2], x[3]);
        re[p] = make_float4(y[0], y[1], y[2], y[3]);
      }
    }
  };
  fetch(0);

#pragma unroll
  for (int i = 0; i < 4; ++i) acc[i][0] = acc[i][1] = tf2{0.f, 0.f};

  for (int k0 = 0; k0 < a.K; k0 += BK) {
    if constexpr (CPLX) {
      const float qr[4] = {rq[0].x, rq[0].y, rq[0].z, rq[0].w}, qi[4] = {rq[1].x, rq[1].y, rq[1].z, rq[1].w};
      const float er[4] = {re[0].x, re[0].y, re[0].z, re[0].w}, ei[4] = {re[1].x, re[1].y, re[1].z, re[1].w};
      // (RotatE: candidate sr's re at Es column sr, its im at T + sr;
      // ComplEx: its (re, im) pair in half (sr / 2) % 2 at (sr / 4)·4 + 2·(sr % 2))
      const int ec = ((sr & 2) ? T : 0) + (sr >> 2) * 4 + 2 * (sr & 1);
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        *reinterpret_cast<tf2*>(&Qs[sk + u][2 * sr]) = tf2{qr[u], qi[u]};
        if constexpr (M == ROTATE) {
          Es[sk + u][sr] = er[u];
          Es[sk + u][T + sr] = ei[u];
        } else {
          *reinterpret_cast<tf2*>(&Es[sk + u][ec]) = tf2{er[u], ei[u]};
        }
      }
    } else if constexpr (PROT) {
      // (sin q, cos q) and (cos e, sin e) of the candidate phase e / (range / π)
      // (model.py:245-246), evaluated once per element by launch_prot_phase
      // (Qs: query sr's (sin, cos) at 2·sr; Es: candidate sr's cos at
      // column sr, its sin at T + sr)
#pragma unroll
      for (int u = 0; u < 4; u += 2) {
        const float4 qv = rq[u >> 1], ev = re[u >> 1];
        *reinterpret_cast<tf2*>(&Qs[sk + u][2 * sr]) = tf2{qv.x, qv.y};
        *reinterpret_cast<tf2*>(&Qs[sk + u + 1][2 * sr]) = tf2{qv.z, qv.w};
        Es[sk + u][sr] = ev.x;
        Es[sk + u][T + sr] = ev.y;
        Es[sk + u + 1][sr] = ev.z;
        Es[sk + u + 1][T + sr] = ev.w;
      }
    } else if constexpr (SPL) {
      // TransE: query sr's element as the pair (q, q) at 2·sr
      const float4 e4 = re[0];
      *reinterpret_cast<tf2*>(&Qs[sk + 0][2 * sr]) = tf2{rq[0].x, rq[0].x};
      *reinterpret_cast<tf2*>(&Qs[sk + 1][2 * sr]) = tf2{rq[0].y, rq[0].y};
      *reinterpret_cast<tf2*>(&Qs[sk + 2][2 * sr]) = tf2{rq[0].z, rq[0].z};
      *reinterpret_cast<tf2*>(&Qs[sk + 3][2 * sr]) = tf2{rq[0].w, rq[0].w};
      Es[sk + 0][sr] = e4.x; Es[sk + 1][sr] = e4.y;
      Es[sk + 2][sr] = e4.z; Es[sk + 3][sr] = e4.w;
    } else {
      const float4 e4 = re[0];
      Qs[sk + 0][sr] = rq[0].x; Qs[sk + 1][sr] = rq[0].y;
      Qs[sk + 2][sr] = rq[0].z; Qs[sk + 3][sr] = rq[0].w;
      Es[sk + 0][sr] = e4.x; Es[sk + 1][sr] = e4.y;
      Es[sk + 2][sr] = e4.z; Es[sk + 3][sr] = e4.w;
    }
    __syncthreads();
    if (k0 + BK < a.K) fetch(k0 + BK);
    if constexpr (SPL) {
      // the next k's LDS operands are read before this k's arithmetic (the
      // unroll-4 loop waited on every k's reads: lgkmcnt(0) in front of its math)
      float4 ql[2][2], el[2];
      auto lds_ld = [&](int k, float4 (&qv)[2], float4& ev) {
        qv[0] = *reinterpret_cast<const float4*>(&Qs[k][ty * 8]);
        qv[1] = *reinterpret_cast<const float4*>(&Qs[k][ty * 8 + 4]);
        ev = *reinterpret_cast<const float4*>(&Es[k][tx * 4]);
      };
      lds_ld(0, ql[0], el[0]);
#pragma unroll
      for (int k = 0; k < BK; ++k) {
        if (k + 1 < BK) lds_ld(k + 1, ql[(k + 1) & 1], el[(k + 1) & 1]);
        TileMath<M, MODE>::transe_spl(ql[k & 1], el[k & 1], acc);
      }
    } else
#pragma unroll 4
    for (int k = 0; k < BK; ++k) {
      if constexpr (CPLX || PROT) {
        const float4 qa = *reinterpret_cast<const float4*>(&Qs[k][ty * 8]);
        const float4 qb = *reinterpret_cast<const float4*>(&Qs[k][ty * 8 + 4]);
        const float4 ea = *reinterpret_cast<const float4*>(&Es[k][tx * 4]);
        const float4 eb = *reinterpret_cast<const float4*>(&Es[k][T + tx * 4]);
        const tf2 q2[4] = {tf2{qa.x, qa.y}, tf2{qa.z, qa.w}, tf2{qb.x, qb.y}, tf2{qb.z, qb.w}};
        const tf2 e2[4] = {tf2{ea.x, ea.y}, tf2{ea.z, ea.w}, tf2{eb.x, eb.y}, tf2{eb.z, eb.w}};
        if constexpr (PROT) TileMath<M, MODE>::prot(q2, ea, eb, acc);
        else if constexpr (M == ROTATE) TileMath<M, MODE>::rot(q2, ea, eb, acc);
        else TileMath<M, MODE>::cplx(q2, e2, acc);
      } else {
        const float4 q4 = *reinterpret_cast<const float4*>(&Qs[k][ty * 4]);
        const float4 e4 = *reinterpret_cast<const float4*>(&Es[k][tx * 4]);
        TileMath<M, MODE>::real(q4, e4, acc, c);
      }
    }
    __syncthreads();
  }
