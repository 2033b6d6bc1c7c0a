// kge_row_walk.inc — the staged row walk of the evaluation kernels that score
// in the reference's operation order (kge_kernels.inc includes it once, inside
// namespace kge): a half-wave copies one table row into its own LDS slot, its
// 32 lanes score the row from there (the cascade of ref_score_half reads its
// elements in a data-dependent order, so it reads LDS), and the block counts
// the scores against the true one.  k_rank_cand, k_rank_rel and k_rshard_count
// walk with walk_rows; k_rank_refine and k_rsf_finish, whose items are decided
// at run time, stage with stage_row alone; all but k_rsf_finish, which counts
// in registers, count with count_scores.

// VW: floats per staging slot — 4 (16-byte loads and LDS writes) or 1
template <int VW>
struct RowSlot { using T = float; };
template <>
struct RowSlot<4> { using T = tf4; };  // (a native vector: an array of HIP's float4 struct went to scratch)

// One row of nT slots from global memory into the half's LDS slot row_l, four
// loads in flight per lane (one at a time left every load's latency exposed).
// The caller waits for the writes (s_waitcnt lgkmcnt(0)) before the half reads
// the row.
template <int VW>
__device__ __forceinline__ void stage_row(const float* src, float* row_l, int nT, int hl) {
  using T = typename RowSlot<VW>::T;
  const T* sT = reinterpret_cast<const T*>(src);
  T* const rT = reinterpret_cast<T*>(row_l);
  const T zero = T();
  for (int k0 = hl; k0 < nT; k0 += 128) {
    const bool b1 = k0 + 32 < nT, b2 = k0 + 64 < nT, b3 = k0 + 96 < nT;
    const T v0 = sT[k0], v1 = b1 ? sT[k0 + 32] : zero, v2 = b2 ? sT[k0 + 64] : zero, v3 = b3 ? sT[k0 + 96] : zero;
    rT[k0] = v0;
    if (b1) rT[k0 + 32] = v1;
    if (b2) rT[k0 + 64] = v2;
    if (b3) rT[k0 + 96] = v3;
  }
}

// The walk of one half-wave (lane hl of half `half`, one of the ns halves with
// a slot) over its items j = half, half + ns, ... < items.  item_src(i, ok&)
// gives the row address of the half's i-th item (called with i ascending, every
// i once) and may clear ok; score(j, row, ok) scores item j from `row`, which
// it may overwrite when the row is staged.  Three shapes:
//   PQ < 0   rows read where they lie, never written (row_l unused);
//   PQ > 0   rows of at most 32·PQ slots: the next item's row is loaded into
//            PQ registers per lane while this item is scored (the row loads
//            used to wait in front of every score), then written to the slot;
//   PQ == 0  wider rows, staged by stage_row without prefetch.
// PQ and VW are template parameters and both callables are inlined, so each
// kernel scores at one place of its text and the prefetched row stays in
// registers: with the shape chosen at run time inside one kernel it went to
// scratch.
// The half's 32 lanes read each other's LDS writes.  LDS operations of one wave
// complete in order, so waiting for this wave's own writes (lgkmcnt(0)) is all
// the synchronisation the slot needs before it is read; and a score depends on
// every element of the row, so the row's reads are done before the next item
// overwrites it — the compiler barrier after score keeps the compiler to that
// order.
template <int PQ, int VW, class Src, class Score>
__device__ __forceinline__ void walk_rows(int items, int half, int ns, int hl, float* row_l, int Le, Src item_src,
                                          Score score) {
  using T = typename RowSlot<VW>::T;
  const int nit = (items - half + ns - 1) / ns;  // the half's items (≤ 0: none)
  auto score_item = [&](int i, float* row, bool ok) __attribute__((always_inline)) {
    score(half + ns * i, row, ok);
    asm volatile("" ::: "memory");
  };
  if constexpr (PQ < 0) {
    for (int i = 0; i < nit; ++i) {
      bool ok = true;
      const float* src = item_src(i, ok);
      score_item(i, const_cast<float*>(src), ok);
    }
  } else {
    const int nT = Le / VW;
    if constexpr (PQ > 0) {
      T* const rT = reinterpret_cast<T*>(row_l);
      const T zero = T();
      T nx[PQ > 0 ? PQ : 1];
      bool nx_ok = true;
      auto fetch = [&](int i) __attribute__((always_inline)) {
        const T* sT = reinterpret_cast<const T*>(item_src(i, nx_ok));
#pragma unroll
        for (int u = 0; u < PQ; ++u) {
          const int k = hl + 32 * u;
          nx[u] = (k < nT) ? sT[k] : zero;
        }
      };
      if (nit > 0) fetch(0);
      for (int i = 0; i < nit; ++i) {
        const bool ok = nx_ok;
#pragma unroll
        for (int u = 0; u < PQ; ++u) {
          const int k = hl + 32 * u;
          if (k < nT) rT[k] = nx[u];
        }
        if (i + 1 < nit) fetch(i + 1);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        score_item(i, row_l, ok);
      }
    } else {
      for (int i = 0; i < nit; ++i) {
        bool ok = true;
        stage_row<VW>(item_src(i, ok), row_l, nT, hl);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        score_item(i, row_l, ok);
      }
    }
  }
}

// The block's count of the scores scr[0 .. n) against st, those skip(x) names
// left out: strictly greater into cnt_s[0], equal into cnt_s[1] (two LDS
// counters the caller zeroed behind a barrier; it reads them behind another).
// NaN scores count as neither.
template <class Skip>
__device__ __forceinline__ void count_scores(const float* scr, int n, float st, int* cnt_s, Skip skip) {
  const int tid = threadIdx.x;
  int g = 0, e_ = 0;
  for (int x = tid; x < n; x += 256) {
    if (skip(x)) continue;
    g += (scr[x] > st);
    e_ += (scr[x] == st);
  }
  g = (int)wave_sum((float)g);  // counts ≤ the 1024 scores of a chunk or list: exact in fp32
  e_ = (int)wave_sum((float)e_);
  if ((tid & 63) == 0 && (g | e_)) {
    atomicAdd(&cnt_s[0], g);
    atomicAdd(&cnt_s[1], e_);
  }
}

// (PQ, VW) of a walk over rows of Le floats: in place, or the smallest prefetch
// that holds a row of nT = Le / VW slots (0 past 512).  f(integral_constant PQ,
// integral_constant VW) launches the kernel instantiated for the pair.
template <class F>
int walk_variant(bool in_place, bool vec4, int Le, F f) {
  using std::integral_constant;
  if (in_place) return f(integral_constant<int, -1>{}, integral_constant<int, 1>{});
  const int nT = vec4 ? Le >> 2 : Le;  // slots per row
  auto by_width = [&](auto vw) {
    if (nT <= 128) return f(integral_constant<int, 4>{}, vw);
    if (nT <= 256) return f(integral_constant<int, 8>{}, vw);
    if (nT <= 512) return f(integral_constant<int, 16>{}, vw);
    return f(integral_constant<int, 0>{}, vw);
  };
  return vec4 ? by_width(integral_constant<int, 4>{}) : by_width(integral_constant<int, 1>{});
}
