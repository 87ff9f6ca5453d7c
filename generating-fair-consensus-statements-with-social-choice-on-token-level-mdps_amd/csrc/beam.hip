// beam.hip — whole beam-search scoring / decode steps in one launch.
#include "cs_kernels.cuh"

namespace {

// ---------------------------------------------------------------------------
// beam step: one launch from logits to the ordered candidates
// ---------------------------------------------------------------------------
// A whole beam-search scoring step after the LM head (beam_search.py:495-560) in ONE
// launch, one workgroup per (agent row, vocab split):
//   1. stream the split -> (m, s) partial (block_lse_partial, as lsg_stream_kernel);
//   2. the LAST workgroup to finish a row (arrival counter per row) merges the row's
//      partials in split order (one wave, lanes over splits: lsg_merge_kernel's
//      arithmetic), gathers the row's K candidate tokens and writes
//      U[a, b*K+j] = R[a, b] + lp (fp32, the method's cumulative reward);
//   3. MIN / MAX welfare is order-free, so each row finisher also folds its K
//      utilities into a per-candidate key with one device-scope atomicMax (ordered
//      float keys; MIN stores inverted keys), and the LAST row to finish (one more
//      counter) only reads the C keys back.  SUM / SUMLOG (order matters in fp64) are
//      folded by the last row over the agents in agent order (welfare_kernel's fold,
//      non-finite skipped).  When B*K <= kFusedSort the last row then sorts the
//      (value desc, index asc) keys in LDS (topk_kernel's keys).
//   The candidate ids and their logits are loaded before the stream starts, so the
//   gather costs no memory round trip after the row's lse is known.
// Bit-identical to cs_logsoftmax_gather + cs_welfare_reduce + cs_segmented_topk.
// Hand-offs use sc1 stores / loads and arrival counters (no fences, see st_sc1).
// Nobody waits on anybody, so the launch cannot stall; the last arrivers reset the
// counters to zero, which keeps the workspace reusable (and graph-replayable) without
// a memset.
// The hand-off primitives (st_sc1 / ld_sc1 / wait_stores / arrive) live in
// cs_kernels.cuh; tests/test_abi.py pins their sc1 lowering on this toolchain.
// Hand-off regions are padded so that every 128-byte line is read by ONE consumer
// workgroup, after all of it is published: a line is never in an L2 (per XCD) before its
// consumer's first read of it in the launch.
__host__ __device__ constexpr int64_t pad_line(int64_t n, int64_t elt_bytes) {
  return (n * elt_bytes + 127) / 128 * 128 / elt_bytes;
}

constexpr int kFusedSort = 1024;      // candidates sorted inside the launch
constexpr int kSelectMax = 256;       // n_order up to this: threshold selection, no full sort
constexpr int kBeamMaxRows = 65536;   // A * B (one arrival counter per row)
constexpr int kBeamMaxCand = 16384;   // B * K (one welfare key per candidate)
// workspace: [done counter | pad to 64 B][row counters][welfare keys][row partials]
constexpr size_t kBeamRowCntOff = 64;
constexpr size_t kBeamKeyOff = kBeamRowCntOff + sizeof(uint32_t) * kBeamMaxRows;
constexpr size_t kBeamCounterBytes = kBeamKeyOff + sizeof(uint32_t) * kBeamMaxCand;

// Welfare key of one utility for the atomic MIN / MAX fold: 0 = no finite value yet (the
// zeroed workspace state); order_key of a finite float is >= 0x00800000, so MAX keeps
// order_key(u) and MIN keeps ~order_key(u) (the largest inverted key is the minimum).
__device__ __forceinline__ uint32_t welfare_key(float u, bool is_min) {
  const uint32_t k = order_key(u);
  return is_min ? ~k : k;
}
__device__ __forceinline__ float welfare_from_key(uint32_t k, bool is_min) {
  if (k == 0u) return __builtin_nanf("");
  return key_to_float(is_min ? ~k : k);
}

__device__ __forceinline__ void welfare_fold(double& acc, bool& any, float u, int kind,
                                             double eps) {
  if (!__builtin_isfinite(u)) return;  // SKIP (and the masked tail of a batch)
  const double d = static_cast<double>(u);
  switch (kind) {
    case CS_WELFARE_MIN:
      acc = any ? fmin(acc, d) : d;
      break;
    case CS_WELFARE_MAX:
      acc = any ? fmax(acc, d) : d;
      break;
    case CS_WELFARE_SUM:
      acc += d;
      break;
    default:
      acc += log(fmax(d, eps));
      break;
  }
  any = true;
}

// Welfare of NQ candidates (c0, c0 + stride, ...) over all agents, in agent order; NQ x NA
// sc1 loads in flight per batch so the fold costs about one memory round trip per batch.
template <int NQ, int NA>
__device__ __forceinline__ void fold_candidates(uint32_t* U, int32_t A, int32_t C, int32_t c0,
                                                int32_t stride, int kind, double eps,
                                                double* acc, bool* any) {
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    acc[q] = 0.0;
    any[q] = false;
  }
  for (int32_t a0 = 0; a0 < A; a0 += NA) {
    float ub[NQ][NA];
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const int32_t c = c0 + q * stride;
#pragma unroll
      for (int j = 0; j < NA; ++j)
        ub[q][j] = (c < C && a0 + j < A)
                       ? __uint_as_float(ld_sc1(U + static_cast<int64_t>(a0 + j) * C + c))
                       : __builtin_nanf("");
    }
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
#pragma unroll
      for (int j = 0; j < NA; ++j) welfare_fold(acc[q], any[q], ub[q][j], kind, eps);
    }
  }
}

// The kept beams' cumulative rewards: out_kept[a][r] = U[a][ord[r]] (ord in LDS), all
// A * n_order loads spread over the block so they are in flight together (U was written
// by other workgroups: sc1 loads).
template <int BLOCK>
__device__ __forceinline__ void keep_columns(uint32_t* U, float* out_kept, const int32_t* ord,
                                             int32_t A, int32_t C, int32_t n_order) {
  const int32_t n = A * n_order;
  for (int32_t i = threadIdx.x; i < n; i += BLOCK) {
    const int32_t a = i / n_order;
    const int32_t r = i - a * n_order;
    out_kept[i] = __uint_as_float(ld_sc1(U + static_cast<int64_t>(a) * C + ord[r]));
  }
}

// Descending bitonic sort of n2 (a power of two <= KPT * BLOCK) distinct keys held in
// registers: element i = r * BLOCK + tid lives in kv[r] of thread tid.  Exchanges at
// stride < 64 go through wave shuffles (no barrier), at stride >= BLOCK between the
// thread's own registers, and only the strides in between through LDS, double-buffered
// so that each such pass costs one barrier.  For n2 = 1024 on 1024 threads: 10 LDS
// passes of the 55 instead of 55 barrier-separated LDS passes.
__device__ __forceinline__ unsigned long long bitonic_pick(unsigned long long a,
                                                           unsigned long long b, int i, int stride,
                                                           int size) {
  const bool keep_max = ((i & stride) == 0) == ((i & size) == 0);
  return keep_max ? (a > b ? a : b) : (a < b ? a : b);
}

template <int BLOCK, int KPT>
__device__ __forceinline__ void bitonic_desc_regs(unsigned long long (&kv)[KPT], int n2,
                                                  unsigned long long* buf0,
                                                  unsigned long long* buf1) {
  const int tid = threadIdx.x;
  bool flip = false;
  for (int size = 2; size <= n2; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      if (stride >= BLOCK) {
        const int rs = stride / BLOCK;
#pragma unroll
        for (int r = 0; r < KPT; ++r) {
          if ((r & rs) == 0 && (r | rs) < KPT) {
            const int i = r * BLOCK + tid;
            if (i < n2) {
              const unsigned long long a = kv[r], b = kv[r | rs];
              const bool desc = (i & size) == 0;
              if ((a < b) == desc) {
                kv[r] = b;
                kv[r | rs] = a;
              }
            }
          }
        }
      } else if (stride >= 64) {
        unsigned long long* buf = flip ? buf1 : buf0;
        flip = !flip;
#pragma unroll
        for (int r = 0; r < KPT; ++r) {
          const int i = r * BLOCK + tid;
          if (i < n2) buf[i] = kv[r];
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < KPT; ++r) {
          const int i = r * BLOCK + tid;
          if (i < n2) kv[r] = bitonic_pick(kv[r], buf[i ^ stride], i, stride, size);
        }
      } else {
#pragma unroll
        for (int r = 0; r < KPT; ++r) {
          const int i = r * BLOCK + tid;
          const unsigned long long b = __shfl_xor(kv[r], stride, 64);
          if (i < n2) kv[r] = bitonic_pick(kv[r], b, i, stride, size);
        }
      }
    }
  }
}

// LDS of the beam kernels' last-workgroup tail (welfare readback / fold, order, kept).
struct BeamLds {
  unsigned long long* keys;   // 2 * kFusedSort: bitonic buffers, or one 16 KB histogram
  unsigned long long* keys2;
  unsigned long long* sel_cand;  // kTopkCand
  float* sm_w;                   // kFusedSort
  int32_t* sm_ord;               // kFusedSort
  uint32_t* sm_tw;               // BLOCK / 64
  int* sm_res;                   // 2
  uint32_t* sm_n;
};

template <int BLOCK>
__device__ __forceinline__ void beam_order(const BeamLds& L, uint32_t* Uw, int32_t A, int32_t C,
                                           int32_t n_order, int32_t n2,
                                           int32_t* __restrict__ out_order,
                                           float* __restrict__ out_val,
                                           float* __restrict__ out_kept);

// Run by the last workgroup of a beam step once every U value (and, for MIN / MAX, every
// welfare key) is published: W for every candidate, then the order (radix-select top-n
// or the full bitonic sort) and the kept beams' rewards.
template <int BLOCK>
__device__ __forceinline__ void beam_tail(const BeamLds& L, uint32_t* Uw, uint32_t* wkey,
                                          float* __restrict__ W, int32_t A, int32_t C, int kind,
                                          double eps, int32_t n_order, int32_t n2,
                                          int32_t* __restrict__ out_order,
                                          float* __restrict__ out_val,
                                          float* __restrict__ out_kept) {
  const int tid = threadIdx.x;
  const bool order_free = kind == CS_WELFARE_MIN || kind == CS_WELFARE_MAX;
  const bool is_min = kind == CS_WELFARE_MIN;
  unsigned long long* keys = L.keys;
  unsigned long long* keys2 = L.keys2;
  unsigned long long* sel_cand = L.sel_cand;
  float* sm_w = L.sm_w;
  int32_t* sm_ord = L.sm_ord;
  uint32_t* sm_tw = L.sm_tw;
  int* sm_res = L.sm_res;
  uint32_t& sm_n = *L.sm_n;
  const bool sort_here = n_order > 0 && n2 <= kFusedSort;
  if (order_free) {
    for (int32_t c = tid; c < C; c += BLOCK) {
      const float w = welfare_from_key(ld_sc1(wkey + c), is_min);
      st_sc1(wkey + c, 0u);  // leave the workspace zeroed for the next call
      W[c] = w;
      if (sort_here) sm_w[c] = w;
    }
  } else {
    for (int32_t c = tid; c < C; c += BLOCK) {
      double acc[1];
      bool any[1];
      fold_candidates<1, 16>(Uw, A, C, c, BLOCK, kind, eps, acc, any);
      const float w = any[0] ? static_cast<float>(acc[0]) : __builtin_nanf("");
      W[c] = w;
      if (sort_here) sm_w[c] = w;
    }
  }
  if (!sort_here) return;  // block-uniform
  beam_order<BLOCK>(L, Uw, A, C, n_order, n2, out_order, out_val, out_kept);
}

// The order of the C welfare values in L.sm_w (written by the calling block): the n_order
// best (radix-select threshold / wave bound + rank counting, or the full bitonic sort) by
// (W desc, index asc), NaN last, and the kept beams' rewards out_kept[a][r] = U[a][order[r]].
template <int BLOCK>
__device__ __forceinline__ void beam_order(const BeamLds& L, uint32_t* Uw, int32_t A, int32_t C,
                                           int32_t n_order, int32_t n2,
                                           int32_t* __restrict__ out_order,
                                           float* __restrict__ out_val,
                                           float* __restrict__ out_kept) {
  const int tid = threadIdx.x;
  unsigned long long* keys = L.keys;
  unsigned long long* keys2 = L.keys2;
  unsigned long long* sel_cand = L.sel_cand;
  float* sm_w = L.sm_w;
  int32_t* sm_ord = L.sm_ord;
  uint32_t* sm_tw = L.sm_tw;
  int* sm_res = L.sm_res;
  uint32_t& sm_n = *L.sm_n;
  __syncthreads();
  if (n_order <= kSelectMax) {
    // the n_order best by histogram threshold + rank counting (as vocab_topk): the
    // candidates' (value, ~index) keys are distinct, so the order is the full sort's
    uint32_t* hist = reinterpret_cast<uint32_t*>(keys);      // keys + keys2: 16 KB
    unsigned long long* cand = sel_cand;
    if (tid == 0) sm_n = 0u;
    unsigned long long kc[kFusedSort / BLOCK];
#pragma unroll
    for (int r = 0; r < kFusedSort / BLOCK; ++r) {
      const int32_t c = r * BLOCK + tid;
      kc[r] = c < C ? (static_cast<unsigned long long>(order_key(sm_w[c])) << 32) |
                          static_cast<unsigned long long>(0xffffffffu - static_cast<uint32_t>(c))
                    : 0ull;
    }
    auto emit = [&](int r, unsigned long long key) {
      const int32_t c = static_cast<int32_t>(0xffffffffu - static_cast<uint32_t>(key & 0xffffffffull));
      out_order[r] = c;
      if (out_val) out_val[r] = sm_w[c];
      sm_ord[r] = c;
    };
    if (BLOCK <= 256 && n_order <= kWaveBoundMaxK) {
      // few kept beams (cs_beam_select's 256-thread block): the wave bound instead of
      // histogram passes (profiles/r01h_decode_tail_wave_bound.jsonl)
      __syncthreads();   // sm_n = 0 is visible before any append
      uint32_t lm = 0u;
#pragma unroll
      for (int r = 0; r < kFusedSort / BLOCK; ++r)
        if (kc[r]) lm = max(lm, static_cast<uint32_t>(kc[r] >> 32));
      const uint32_t t = wave_bound<BLOCK>(lm, n_order, sm_tw);
#pragma unroll
      for (int r = 0; r < kFusedSort / BLOCK; ++r) {
        if (kc[r] && static_cast<uint32_t>(kc[r] >> 32) >= t) {
          const uint32_t at = atomicAdd(&sm_n, 1u);
          if (at < kTopkCand) cand[at] = kc[r];
        }
      }
      __syncthreads();
      const uint32_t nc = sm_n;
      if (nc <= static_cast<uint32_t>(kTopkCand)) {  // block-uniform
        rank_candidates<BLOCK>(cand, static_cast<int>(nc), n_order, emit);
        if (out_kept) {
          __syncthreads();
          keep_columns<BLOCK>(Uw, out_kept, sm_ord, A, C, n_order);
        }
        return;
      }
      __syncthreads();
      if (tid == 0) sm_n = 0u;
    }
    const RadixCut cut = radix_select<BLOCK>(
        [&](auto f) {
#pragma unroll
          for (int r = 0; r < kFusedSort / BLOCK; ++r)
            if (kc[r]) f(kc[r]);
        },
        static_cast<uint32_t>(n_order), static_cast<uint32_t>(n_order + 64), hist, sm_tw, sm_res);
    if (cut.count <= kTopkCand) {  // block-uniform
#pragma unroll
      for (int r = 0; r < kFusedSort / BLOCK; ++r)
        if (kc[r] && (kc[r] >> cut.shift) >= cut.prefix) cand[atomicAdd(&sm_n, 1u)] = kc[r];
      __syncthreads();
      rank_candidates<BLOCK>(cand, static_cast<int>(sm_n), n_order, emit);
      if (out_kept) {
        __syncthreads();
        keep_columns<BLOCK>(Uw, out_kept, sm_ord, A, C, n_order);
      }
      return;
    }
    __syncthreads();  // the fallback sort below reuses keys / keys2
  }
  constexpr int KPT = kFusedSort / BLOCK;
  unsigned long long kv[KPT];
#pragma unroll
  for (int r = 0; r < KPT; ++r) {
    const int32_t c = r * BLOCK + tid;
    kv[r] = c < C ? (static_cast<unsigned long long>(order_key(sm_w[c])) << 32) |
                        static_cast<unsigned long long>(0xffffffffu - static_cast<uint32_t>(c))
                  : 0ull;
  }
  bitonic_desc_regs<BLOCK, KPT>(kv, n2, keys, keys2);
#pragma unroll
  for (int r = 0; r < KPT; ++r) {
    const int32_t i = r * BLOCK + tid;
    if (i < n_order) {
      const int32_t c = static_cast<int32_t>(0xffffffffu - static_cast<uint32_t>(kv[r] & 0xffffffffull));
      out_order[i] = c;
      if (out_val) out_val[i] = sm_w[c];
      sm_ord[i] = c;
    }
  }
  if (out_kept) {
    __syncthreads();
    keep_columns<BLOCK>(Uw, out_kept, sm_ord, A, C, n_order);
  }
}

#ifdef CS_TRACE_DECODE
// cs_beam_decode_step's phases, slots: 0 first block start (min), 1 last proposer chunk
// start, 2 last proposer chunk published, 3 last proposer merge done, 4 last row block start,
// 5 first row lse, 6 last row lse, 7 last beam gather done, 8 tail start, 9 tail end
// (wall_clock64 ticks)
__device__ unsigned long long g_dec_ts[16];
#define DEC_T(...) __VA_ARGS__
#else
#define DEC_T(...)
#endif

// ---------------------------------------------------------------------------
// what cs_beam_step's and cs_beam_decode_step's kernels share
// ---------------------------------------------------------------------------
// The LDS of a beam kernel, instantiated once per kernel as __shared__.  One pool: the bf16
// soft-cap table while a row streams, the proposer's and the tail's buffers otherwise (keys2
// directly after keys: the selection path uses the pair as one 16 KB histogram).  The pool
// comes first, so the 16-byte alignment it needs pads nothing.
template <int DT, bool CAP, bool FIXED, int BLOCK>
struct BeamSmem {
  static constexpr bool kTab = CapTable<DT, CAP, FIXED>::kOn;
  static constexpr int kPoolTail = 2 * kFusedSort + kTopkCand + kFusedSort;  // u64 words
  static constexpr int kPool = kTab && kCapTab / 2 > kPoolTail ? kCapTab / 2 : kPoolTail;
  alignas(16) unsigned long long pool[kPool];
  float sm_m[BLOCK / 64];
  float sm_s[BLOCK / 64];
  uint32_t sm_tw[2 * BLOCK / 64];
  int sm_res[2];
  uint32_t sm_n;
  int sm_last;   // a last-arriver decision, broadcast to the block

  __device__ __forceinline__ float* ctab() { return reinterpret_cast<float*>(pool); }
  __device__ __forceinline__ BeamLds view() {
    unsigned long long* sel_cand = pool + 2 * kFusedSort;
    float* sm_w = reinterpret_cast<float*>(sel_cand + kTopkCand);
    return BeamLds{pool, pool + kFusedSort, sel_cand, sm_w,
                   reinterpret_cast<int32_t*>(sm_w + kFusedSort), sm_tw, sm_res, &sm_n};
  }
};

// One work item (row, sitem) of the agent-row stream: the item's (m, s) partial in the
// streaming arithmetic of cs_logsoftmax_gather (block_lse_partial; split rows the canonical
// split form, split_partial, BLOCK / 256 splits per block), published; the row's last arriver
// merges the row's partials in split order (one wave, lanes over splits: lsg_merge_kernel's
// arithmetic) and leaves the row's arrival counter at zero.  Returns, block-uniformly, whether
// this block finished the row; then `lse` holds the row's log-sum-exp in thread 0.
template <int DT, bool CAP, bool FIXED, int BLOCK, int UNROLL>
__device__ __forceinline__ bool beam_row_stream(BeamSmem<DT, CAP, FIXED, BLOCK>& S,
                                                const char* __restrict__ rp, int32_t row,
                                                int32_t sitem, int32_t nsplit, int64_t split_len,
                                                int64_t vocab, float cap, float inv_cap,
                                                unsigned long long* __restrict__ part,
                                                uint32_t* __restrict__ row_cnt, float& lse) {
  const int tid = threadIdx.x;
  if constexpr (BeamSmem<DT, CAP, FIXED, BLOCK>::kTab) {
    build_cap_table<BLOCK>(S.ctab(), cap, inv_cap);
    __syncthreads();
  }
  int32_t split = 0;
  bool valid = true;
  const float2 ms =
      nsplit > 1 ? split_partial<DT, CAP, FIXED, BLOCK, true>(rp, sitem, nsplit, split_len, vocab, cap,
                                                        inv_cap, S.sm_m, S.sm_s, S.ctab(), split, valid)
                 : block_lse_partial<DT, CAP, FIXED, BLOCK, UNROLL, true>(rp, 0, vocab, cap, inv_cap,
                                                                    S.sm_m, S.sm_s, S.ctab());
  if (nsplit <= 1) {
    if (tid == 0) lse = ms.x + logf(ms.y);
    return true;
  }
  unsigned long long* rpart = part + static_cast<int64_t>(row) * pad_line(nsplit, 8);
  if (valid && tid % kSplitSub == 0) {
    st_sc1(rpart + split, (static_cast<unsigned long long>(__float_as_uint(ms.y)) << 32) |
                              __float_as_uint(ms.x));
    wait_stores();
  }
  __syncthreads();
  if (tid == 0) {
    const uint32_t nv = static_cast<uint32_t>(split_count(sitem, nsplit, BLOCK));
    S.sm_last = arrive(&row_cnt[row], nv) + nv == static_cast<uint32_t>(nsplit);
  }
  __syncthreads();
  if (!S.sm_last) return false;  // block-uniform
  if (tid < 64) {
    float m = -INFINITY, s = 0.0f;
    for (int j = tid; j < nsplit; j += 64) {
      const unsigned long long p = ld_sc1(rpart + j);
      lse_merge(m, s, __uint_as_float(static_cast<uint32_t>(p)),
                __uint_as_float(static_cast<uint32_t>(p >> 32)));
    }
    wave_lse_reduce(m, s);
    if (tid == 0) {
      lse = m + logf(s);
      st_sc1(row_cnt + row, 0u);
    }
  }
  return true;
}

// Candidate token t's logit in the row at rp; ids outside [0, vocab) are padding (!ok).
template <int DT>
__device__ __forceinline__ float beam_candidate_logit(const char* __restrict__ rp, int32_t t,
                                                      int64_t vocab, bool& ok) {
  ok = t >= 0 && t < vocab;
  return ok ? load_one<DT>(rp, t) : 0.0f;
}

// One (agent, candidate): u = r + (softcap(x) - lse), NaN for padding, published to U; MIN /
// MAX welfare is order-free, so a finite u is folded into the candidate's welfare key here.
template <bool CAP>
__device__ __forceinline__ void beam_store_utility(uint32_t* u_at, uint32_t* wkey_at, bool ok, float x,
                                                   float lse, float r, float cap, float inv_cap,
                                                   int kind) {
  float lp = __builtin_nanf("");
  if (ok) {
    if (CAP) x = softcap_fn(x, cap, inv_cap);
    lp = x - lse;
  }
  const float u = r + lp;
  st_sc1(u_at, __float_as_uint(u));
  if ((kind == CS_WELFARE_MIN || kind == CS_WELFARE_MAX) && __builtin_isfinite(u))
    __hip_atomic_fetch_max(wkey_at, welfare_key(u, kind == CS_WELFARE_MIN), __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
}

// The end of a beam launch: this block's U values (and welfare keys) are published, and the
// last of the n blocks that get here resets the counter and runs the tail.
template <int BLOCK, typename Smem>
__device__ __forceinline__ void beam_finish(Smem& S, uint32_t* done_cnt, uint32_t n, uint32_t* Uw,
                                            uint32_t* wkey, float* __restrict__ W, int32_t A,
                                            int32_t C, int kind, double eps, int32_t n_order,
                                            int32_t n2, int32_t* __restrict__ out_order,
                                            float* __restrict__ out_val,
                                            float* __restrict__ out_kept) {
  const int tid = threadIdx.x;
  wait_stores();
  __syncthreads();
  DEC_T(if (tid == 0) atomicMax(&g_dec_ts[7], wall_clock64());)
  if (tid == 0) S.sm_last = arrive(done_cnt) == n - 1u;
  __syncthreads();
  if (!S.sm_last) return;  // block-uniform
  if (tid == 0) st_sc1(done_cnt, 0u);
  DEC_T(if (tid == 0) g_dec_ts[8] = wall_clock64();)
  beam_tail<BLOCK>(S.view(), Uw, wkey, W, A, C, kind, eps, n_order, n2, out_order, out_val, out_kept);
  DEC_T(if (tid == 0) g_dec_ts[9] = wall_clock64();)
}

template <int DT, bool CAP, bool FIXED, int BLOCK, int UNROLL>
__global__ __launch_bounds__(BLOCK, BLOCK >= 1024 ? 8 : 4) void beam_step_kernel(
    const char* __restrict__ logits, int64_t vocab, int64_t ld_bytes, int32_t nsplit,
    int64_t split_len, int32_t A, int32_t B, int32_t K, const int32_t* __restrict__ tgt,
    const float* __restrict__ R, float cap, float inv_cap, int kind, double eps,
    unsigned long long* __restrict__ part, uint32_t* __restrict__ row_cnt,
    uint32_t* __restrict__ done_cnt, uint32_t* __restrict__ wkey, float* __restrict__ U,
    float* __restrict__ W, int32_t n_order, int32_t n2, int32_t* __restrict__ out_order,
    float* __restrict__ out_val, float* __restrict__ out_kept) {
  __shared__ BeamSmem<DT, CAP, FIXED, BLOCK> S;
  __shared__ float sm_lse;
  const int tid = threadIdx.x;
  const int32_t rows = A * B;
  const int32_t C = B * K;
  const int64_t item = blockIdx.x;
  const int32_t per_row = nsplit > 1 ? split_items(nsplit, BLOCK) : 1;
  const int32_t row = static_cast<int32_t>(item / per_row);
  const int32_t sitem = static_cast<int32_t>(item - static_cast<int64_t>(row) * per_row);
  const int32_t ag = row / B;
  const int32_t bm = row - ag * B;
  const char* rp = logits + row * ld_bytes;
  uint32_t* Uw = reinterpret_cast<uint32_t*>(U);
  // the candidate ids and their logits are read now (used only at the row finish), so
  // the finisher's gather costs no memory round trip after the lse is known
  bool ok;
  const float xg = beam_candidate_logit<DT>(rp, (tid < K) ? tgt[bm * K + tid] : -1, vocab, ok);

  // 1. stream, 2. row finish by the row's last arriver
  float row_lse = 0.0f;
  if (!beam_row_stream<DT, CAP, FIXED, BLOCK, UNROLL>(S, rp, row, sitem, nsplit, split_len, vocab, cap,
                                                      inv_cap, part, row_cnt, row_lse))
    return;  // block-uniform
  if (tid == 0) sm_lse = row_lse;
  __syncthreads();
  const float r0 = R[row];
  const float lse = sm_lse;
  for (int32_t j = tid; j < K; j += BLOCK) {
    float x = xg;
    bool okj = ok;
    // K > BLOCK: the remaining ids the early read did not cover
    if (j >= BLOCK) x = beam_candidate_logit<DT>(rp, tgt[bm * K + j], vocab, okj);
    beam_store_utility<CAP>(Uw + static_cast<int64_t>(ag) * C + bm * K + j, wkey + bm * K + j, okj, x,
                            lse, r0, cap, inv_cap, kind);
  }

  // 3. welfare + order by the last row
  beam_finish<BLOCK>(S, done_cnt, static_cast<uint32_t>(rows), Uw, wkey, W, A, C, kind, eps, n_order, n2,
                     out_order, out_val, out_kept);
}

// The decode launch: 1024-thread blocks, so split rows take four canonical splits per block
// (split_partial) and the proposer keeps its 16 * 1024-element chunks (per-rank C3: 43.98 ->
// 26.4 us, profiles/r05e_beam_ab_*.jsonl; 256-thread blocks measured slower at C1 too, 17.8 vs
// 16.9 us, r05f_beam_ab.jsonl), 2 16-byte vectors in flight per lane in the agent rows.
constexpr int kDecodeBlock = 1024;
constexpr int kDecodeUnroll = 2;
constexpr int kPropPrio = 2;   // instruction-issue priority of the proposer waves
// elements per lane of a proposer chunk (8 32-bit keys for fp32): 16-bit logits are held raw
// (two per register) and their order keys recomputed on each pass, so twice the elements fit
// the registers of the 32-bit keys -- half the proposer workgroups, and C3's whole grid
// (256 agent rows + 16 beams x 16 chunks) is resident in one round on 256 CUs
// (profiles/r04b_decode_rawkeys_ab.jsonl)
constexpr int kp1024(int dtype) { return dtype != CS_F32 ? 16 : 8; }
// ---------------------------------------------------------------------------
// beam decode step: proposer + scoring in ONE launch
// ---------------------------------------------------------------------------
// cs_vocab_topk on the B reference-policy rows and cs_beam_step on the A*B agent rows
// in one grid, so the proposer's latency hides under the agent-row stream:
//   * blocks [0, B * nchunk): proposer, one per (beam, 16 * BLOCK-element chunk) of the
//     reference row: the chunk's K best composite keys by radix select + rank counting
//     (as vocab_topk_chunk_kernel), handed off; the last chunk of a beam merges the
//     chunk winners the same way and publishes the beam's K candidate ids (out_ids);
//   * blocks [B * nchunk, ...): one per (agent row, vocab split), the beam step's stream;
//     the row's last split publishes the row's log-sum-exp;
//   * per beam an arrival counter takes A + 1 arrivals (its A agent rows and its
//     proposer); the LAST arriver gathers all A x K candidates of that beam (ids, row
//     lse, logits), writes U and folds MIN / MAX welfare keys;
//   * the last beam to finish runs the beam step's tail (beam_tail).
// Proposer blocks come first in the grid, so they are dispatched first.  No block waits
// on another (last-arriver hand-offs only), so the launch cannot stall.  Bit-identical to
// cs_vocab_topk + cs_beam_step (same selection, same lse arithmetic, same U formula).
// Proposer keys per lane: kp1024 (8 32-bit keys, 16 raw 16-bit values; more would spill) when
// that still gives >= 128 proposer workgroups, else 4 (few beams, e.g. C5's B = 8), so the
// proposer finishes under the agent-row stream (tools/beam_ab.py --sweep;
// profiles/r01f_beam_ab*.jsonl).
int decode_kp(int32_t B, int64_t vocab, int32_t K, int dtype) {
  const int big = kp1024(dtype);
  const int64_t nbig = B * ((vocab + big * kDecodeBlock - 1) / (big * static_cast<int64_t>(kDecodeBlock)));
  const int64_t n4c = (vocab + 4LL * kDecodeBlock - 1) / (4LL * kDecodeBlock);
  return (nbig < 128 && n4c * K <= 16384) ? 4 : big;
}
// Grid order: the agent-row blocks first when they leave workgroup slots free for the
// proposer (C3: 256 rows on 256 CUs x 2 slots), the proposer first when the rows alone
// fill the chip (C5: 512 rows) — then the rows would starve the proposer to the end.
int decode_rows_first(int64_t row_blocks) {
  static int n_cu = 0;
  if (n_cu == 0) {
    int dev = 0, v = 0;
    if (hipGetDevice(&dev) == hipSuccess &&
        hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0)
      n_cu = v;
    else
      n_cu = 256;
  }
  const int64_t slots = static_cast<int64_t>(n_cu) * 2;   // 1024-thread workgroups per CU
  return row_blocks < slots ? 1 : 0;
}
constexpr int kBeamMaxBeams = 4096;

template <int DT, bool CAP, bool FIXED, int BLOCK, int UNROLL, int KP>
__global__ __launch_bounds__(BLOCK, BLOCK >= 1024 ? 8 : 4) void beam_decode_kernel(
    const char* __restrict__ ref, int64_t ld_ref_bytes, int32_t nchunk_p, int32_t rows_first,
    int32_t ref_vec,
    const char* __restrict__ logits, int64_t vocab, int64_t ld_bytes, int32_t nsplit,
    int64_t split_len, int32_t A, int32_t B, int32_t K, const float* __restrict__ R, float cap,
    float inv_cap, int kind, double eps, unsigned long long* __restrict__ part,
    unsigned long long* __restrict__ ppart, uint32_t* __restrict__ row_cnt,
    uint32_t* __restrict__ prop_cnt, uint32_t* __restrict__ beam_cnt,
    uint32_t* __restrict__ done_cnt, uint32_t* __restrict__ wkey, uint32_t* __restrict__ lse_ws,
    uint32_t* __restrict__ ids_ws, int32_t* __restrict__ out_ids, float* __restrict__ U, float* __restrict__ W, int32_t n_order,
    int32_t n2, int32_t* __restrict__ out_order, float* __restrict__ out_val,
    float* __restrict__ out_kept) {
  __shared__ BeamSmem<DT, CAP, FIXED, BLOCK> S;
  // the proposer's names for its part of the LDS
  unsigned long long* sel_cand = S.view().sel_cand;
  int32_t* sm_ord = S.view().sm_ord;
  uint32_t* sm_tw = S.sm_tw;
  int* sm_res = S.sm_res;
  uint32_t& sm_n = S.sm_n;
  int& sm_last = S.sm_last;
  uint32_t* hist = reinterpret_cast<uint32_t*>(S.pool);  // keys + keys2: 16 KB
  const int tid = threadIdx.x;
  const int32_t C = B * K;
  const int32_t n_prop = B * nchunk_p;
  uint32_t* Uw = reinterpret_cast<uint32_t*>(U);
  DEC_T(const unsigned long long q0 = wall_clock64(); if (tid == 0) atomicMin(&g_dec_ts[0], q0);)
  int32_t gb;  // the beam this block arrives at
  bool ids_in_lds = false;  // this block merged beam gb's proposer: its ids are in LDS

  const int32_t n_rowblk = static_cast<int32_t>(gridDim.x) - n_prop;
  // block role: proposer blocks first in the grid, or after the row blocks
  const int32_t pblk = rows_first ? static_cast<int32_t>(blockIdx.x) - n_rowblk
                                  : static_cast<int32_t>(blockIdx.x);
  const int32_t rblk = rows_first ? static_cast<int32_t>(blockIdx.x)
                                  : static_cast<int32_t>(blockIdx.x) - n_prop;
  if (pblk >= 0 && pblk < n_prop) {
    // ---- proposer chunk ----
    // the proposer's short latency chain goes first when it shares a CU with a streaming
    // row block (instruction issue priority; the stream is bandwidth-bound, not issue-bound)
    __builtin_amdgcn_s_setprio(kPropPrio);
    DEC_T(if (tid == 0) atomicMax(&g_dec_ts[1], q0);)
    constexpr int CH = KP * BLOCK;
    const int32_t b = pblk / nchunk_p;
    const int32_t chunk = pblk - b * nchunk_p;
    const char* rp = ref + b * ld_ref_bytes;
    const int64_t v0 = static_cast<int64_t>(chunk) * CH;
    const int n = static_cast<int>(min(static_cast<int64_t>(CH), vocab - v0));
    // 32-bit order keys in registers (the token id is implied by (j, lane)): half the
    // registers of 64-bit composite keys, so the 1024-thread variant does not spill.  RAW
    // (16-bit logits): the raw values instead, two per register, each pass recomputing the
    // identical key order_key(softcap(x)) from them (a few VALU ops per element per pass)
    constexpr bool RAW = DT != CS_F32;
    constexpr int NWORD = RAW ? (KP + 1) / 2 : KP;
    uint32_t okey[NWORD];
    constexpr int EPV = Elt<DT>::kPerVec;
    constexpr int RG = KP < EPV ? KP : EPV;   // RAW: consecutive elements per lane group
    const bool vec = KP % EPV == 0 && ref_vec && n == CH;
    if (vec) {
      // whole 16-byte-aligned chunk: KP / EPV non-temporal 16-byte loads per lane, all in
      // flight at once (element (j / EPV * BLOCK + tid) * EPV + j % EPV in okey[j]; RAW: in
      // half j % 2 of word j / 2, the loaded vectors as they are)
      const u32x4* vp = reinterpret_cast<const u32x4*>(rp + v0 * Elt<DT>::kSize);
      u32x4 q[KP / EPV > 0 ? KP / EPV : 1];
#pragma unroll
      for (int j = 0; j < KP / EPV; ++j) q[j] = __builtin_nontemporal_load(vp + j * BLOCK + tid);
#pragma unroll
      for (int j = 0; j < KP / EPV; ++j) {
        if constexpr (RAW) {
#pragma unroll
          for (int e = 0; e < 4; ++e) okey[j * 4 + e] = q[j][e];
        } else {
          float v[EPV];
          unpack_vec<DT>(q[j], v);
#pragma unroll
          for (int e = 0; e < EPV; ++e)
            okey[j * EPV + e] = order_key(CAP ? softcap_fn(v[e], cap, inv_cap) : v[e]);
        }
      }
    } else {
      if constexpr (RAW) {
#pragma unroll
        for (int w = 0; w < NWORD; ++w) okey[w] = 0u;
      }
#pragma unroll
      for (int j = 0; j < KP; ++j) {
        // RAW: the vector path's element order (one index formula for both paths; groups
        // of min(KP, EPV) consecutive elements per lane)
        const int i = RAW ? (j / RG * BLOCK + tid) * RG + j % RG : tid + BLOCK * j;
        if constexpr (RAW) {
          const uint32_t b = i < n ? reinterpret_cast<const uint16_t*>(rp)[v0 + i] : 0u;
          okey[j >> 1] |= b << ((j & 1) * 16);
        } else {
          float x = 0.0f;
          if (i < n) x = load_one<DT>(rp, v0 + i);
          okey[j] = order_key(CAP ? softcap_fn(x, cap, inv_cap) : x);
        }
      }
    }
    auto key32 = [&](int j) -> uint32_t {   // the order key of element j
      if constexpr (RAW) {
        const uint32_t b = (okey[j >> 1] >> ((j & 1) * 16)) & 0xffffu;
        float x;
        if constexpr (DT == CS_BF16) x = __uint_as_float(b << 16);
        else x = static_cast<float>(__builtin_bit_cast(_Float16, static_cast<uint16_t>(b)));
        return order_key(CAP ? softcap_fn(x, cap, inv_cap) : x);
      } else {
        return okey[j];
      }
    };
    // RAW: before each pass over the keys the raw words are named as modified (an empty
    // asm), so the compiler recomputes the keys per pass instead of hoisting all KP of them
    // out of the radix loop into registers (which spills at 64 VGPRs)
    int lbase = tid * RG;    // RAW: element j of this lane is lbase + (j / RG) * BLOCK * RG + j % RG
    auto fresh = [&]() {
      if constexpr (RAW) {
#pragma unroll
        for (int w = 0; w < NWORD; ++w) asm volatile("" : "+v"(okey[w]));
        asm volatile("" : "+v"(lbase));   // nor the KP element indices
      }
    };
    auto local = [&](int j) -> int {   // element of okey[j] within the chunk
      if constexpr (RAW) return lbase + (j / RG) * (BLOCK * RG) + j % RG;
      return vec ? (j / EPV * BLOCK + tid) * EPV + j % EPV : tid + BLOCK * j;
    };
    auto key_of = [&](int j) -> unsigned long long {
      return (static_cast<unsigned long long>(key32(j)) << 32) |
             static_cast<unsigned long long>(0xffffffffu - static_cast<uint32_t>(v0 + local(j)));
    };
    if (tid == 0) sm_n = 0u;
    DEC_T(if (tid == 0) atomicMax(&g_dec_ts[10], wall_clock64());)
    // radix select, no wave bound: in these 1024-thread blocks the bound's registers slow the
    // agent-row stream more than the bound saves (profiles/r01h_decode_wave_bound.jsonl)
    const RadixCut cut = radix_select<BLOCK>(
        [&](auto f) {
          fresh();
#pragma unroll
          for (int j = 0; j < KP; ++j)
            if (local(j) < n) f(key_of(j));
        },
        static_cast<uint32_t>(K), static_cast<uint32_t>(2 * K + 64), hist, sm_tw, sm_res);
    fresh();
#pragma unroll
    for (int j = 0; j < KP; ++j) {
      if (local(j) < n) {
        const unsigned long long kj = key_of(j);
        if ((kj >> cut.shift) >= cut.prefix) sel_cand[atomicAdd(&sm_n, 1u)] = kj;
      }
    }
    __syncthreads();
    DEC_T(if (tid == 0) atomicMax(&g_dec_ts[11], wall_clock64());)
    const int32_t nkeys = nchunk_p * K;
    unsigned long long* pr = ppart + static_cast<int64_t>(b) * pad_line(nkeys, 8);
    unsigned long long* out = pr + static_cast<int64_t>(chunk) * K;
    const int nc = static_cast<int>(sm_n);
    rank_candidates<BLOCK>(sel_cand, nc, K, [&](int r, unsigned long long kc) { st_sc1(out + r, kc); });
    for (int r = nc + tid; r < K; r += BLOCK) st_sc1(out + r, 0ull);
    wait_stores();
    __syncthreads();
    DEC_T(if (tid == 0) { const unsigned long long q = wall_clock64(); atomicMax(&g_dec_ts[2], q);
                          atomicMin(&g_dec_ts[12], q); })
    if (tid == 0) {
      sm_last = arrive(&prop_cnt[b]) == static_cast<uint32_t>(nchunk_p - 1);
      sm_n = 0u;
    }
    __syncthreads();
    if (!sm_last) return;  // block-uniform
    if (tid == 0) st_sc1(prop_cnt + b, 0u);
    // the beam's K best among the chunk winners -> its candidate ids.  The winners are
    // read once (all loads in flight together) into registers when they fit, not again
    // per radix level and for the collection.
    constexpr int MR = 4;
    unsigned long long mk[MR];
    const bool cached = nkeys <= MR * BLOCK;
    if (cached) {
#pragma unroll
      for (int r = 0; r < MR; ++r) {
        const int i = tid + r * BLOCK;
        mk[r] = i < nkeys ? ld_sc1(pr + i) : 0ull;
      }
    }
    auto each_key = [&](auto f) {
      if (cached) {
#pragma unroll
        for (int r = 0; r < MR; ++r)
          if (mk[r]) f(mk[r]);
      } else {
        for (int i = tid; i < nkeys; i += BLOCK) {
          const unsigned long long c = ld_sc1(pr + i);
          if (c) f(c);
        }
      }
    };
    const RadixCut mcut = radix_select<BLOCK>(
        each_key, static_cast<uint32_t>(K), static_cast<uint32_t>(2 * K + 64), hist, sm_tw, sm_res);
    each_key([&](unsigned long long c) {
      if ((c >> mcut.shift) >= mcut.prefix) sel_cand[atomicAdd(&sm_n, 1u)] = c;
    });
    __syncthreads();
    const int mc = static_cast<int>(sm_n);
    // the ids also stay in LDS: when this block gathers the beam it reads them there
    uint32_t* sm_ids = reinterpret_cast<uint32_t*>(sm_ord);
    rank_candidates<BLOCK>(sel_cand, mc, K, [&](int r, unsigned long long c) {
      const uint32_t id = 0xffffffffu - static_cast<uint32_t>(c & 0xffffffffull);
      st_sc1(ids_ws + b * pad_line(K, 4) + r, id);
      sm_ids[r] = id;
      out_ids[b * K + r] = static_cast<int32_t>(id);
    });
    for (int r = mc + tid; r < K; r += BLOCK) {
      st_sc1(ids_ws + b * pad_line(K, 4) + r, 0xffffffffu);
      sm_ids[r] = 0xffffffffu;
      out_ids[b * K + r] = -1;
    }
    ids_in_lds = true;
    DEC_T(if (tid == 0) atomicMax(&g_dec_ts[3], wall_clock64());)
    gb = b;
  } else {
    // ---- agent row stream ----
    const int64_t item = rblk;
    const int32_t per_row = nsplit > 1 ? split_items(nsplit, BLOCK) : 1;
    const int32_t row = static_cast<int32_t>(item / per_row);
    const int32_t sitem = static_cast<int32_t>(item - static_cast<int64_t>(row) * per_row);
    // the beam step's stream (the same bits: a 1024-thread launch, proposer chunks of 16 * 1024
    // elements, takes split rows four splits per block); the row's finisher publishes its lse
    float row_lse = 0.0f;
    if (!beam_row_stream<DT, CAP, FIXED, BLOCK, UNROLL>(S, logits + row * ld_bytes, row, sitem, nsplit,
                                                        split_len, vocab, cap, inv_cap, part, row_cnt,
                                                        row_lse))
      return;  // block-uniform
    if (tid == 0) st_sc1(lse_ws + (row % B) * pad_line(A, 4) + row / B, __float_as_uint(row_lse));
    gb = row % B;
    DEC_T(if (tid == 0) { const unsigned long long q = wall_clock64(); atomicMax(&g_dec_ts[4], q0);
                          atomicMin(&g_dec_ts[5], q); atomicMax(&g_dec_ts[6], q); })
  }

  // ---- arrival at beam gb (A agent rows + its proposer); the last one gathers ----
  wait_stores();
  __syncthreads();
  if (tid == 0) sm_last = arrive(&beam_cnt[gb]) == static_cast<uint32_t>(A);
  __syncthreads();
  if (!sm_last) return;  // block-uniform
  if (tid == 0) st_sc1(beam_cnt + gb, 0u);
  for (int32_t i = tid; i < A * K; i += BLOCK) {
    const int32_t a = i / K;
    const int32_t j = i - a * K;
    const int32_t row = a * B + gb;
    const int32_t t = static_cast<int32_t>(ids_in_lds ? reinterpret_cast<const uint32_t*>(sm_ord)[j]
                                                      : ld_sc1(ids_ws + gb * pad_line(K, 4) + j));
    const float lse = __uint_as_float(ld_sc1(lse_ws + gb * pad_line(A, 4) + a));
    bool ok;
    const float x = beam_candidate_logit<DT>(logits + row * ld_bytes, t, vocab, ok);
    beam_store_utility<CAP>(Uw + static_cast<int64_t>(a) * C + gb * K + j, wkey + gb * K + j, ok, x, lse,
                            R[row], cap, inv_cap, kind);
  }
  beam_finish<BLOCK>(S, done_cnt, static_cast<uint32_t>(B), Uw, wkey, W, A, C, kind, eps, n_order, n2,
                     out_order, out_val, out_kept);
}

}  // namespace

namespace {
// cs_beam_select: one workgroup orders C <= kFusedSort welfare values and keeps the
// rewards of the n_order best columns (beam_order), after the agent-sharded all-reduce.
constexpr int kSelectBlock = 256;
__global__ __launch_bounds__(kSelectBlock) void beam_select_kernel(
    const float* __restrict__ Win, int32_t C, int unfill, uint32_t* __restrict__ Uw, int32_t A,
    float* __restrict__ W_out, int32_t n_order, int32_t n2, int32_t* __restrict__ out_order,
    float* __restrict__ out_val, float* __restrict__ out_kept) {
  __shared__ __attribute__((aligned(16))) unsigned long long pool[2 * kFusedSort + kTopkCand + kFusedSort];
  __shared__ uint32_t sm_tw[2 * kSelectBlock / 64];
  __shared__ int sm_res[2];
  __shared__ uint32_t sm_n;
  unsigned long long* sel_cand = pool + 2 * kFusedSort;
  float* sm_w = reinterpret_cast<float*>(sel_cand + kTopkCand);
  int32_t* sm_ord = reinterpret_cast<int32_t*>(sm_w + kFusedSort);
  const BeamLds L{pool, pool + kFusedSort, sel_cand, sm_w, sm_ord, sm_tw, sm_res, &sm_n};
  for (int32_t c = threadIdx.x; c < C; c += kSelectBlock) {
    float w = Win[c];
    if ((unfill == CS_UNFILL_POSINF && w == INFINITY) || (unfill == CS_UNFILL_NEGINF && w == -INFINITY))
      w = __builtin_nanf("");
    sm_w[c] = w;
    if (W_out) W_out[c] = w;
  }
  beam_order<kSelectBlock>(L, Uw, A, C, n_order, n2, out_order, out_val, out_kept);
}
}  // namespace

namespace {
// The limits cs_beam_step and cs_beam_decode_step share (rows = A * B, C = B * K).
int check_beam_args(const char* fn, int64_t rows, int64_t C, int32_t n_order, const float* out_kept,
                    int welfare_kind, float softcap) {
  const std::string w = std::string(fn) + ": ";
  if (C > kBeamMaxCand) return fail(CS_ERR_INVALID, w + "B*K exceeds 16384");
  if (rows > kBeamMaxRows) return fail(CS_ERR_INVALID, w + "A*B exceeds 65536");
  if (n_order < 0 || n_order > C) return fail(CS_ERR_INVALID, w + "need 0 <= n_order <= B*K");
  if (out_kept && (n_order == 0 || C > kFusedSort))
    return fail(CS_ERR_INVALID, w + "out_kept needs n_order > 0 and B*K <= 1024");
  if (welfare_kind < CS_WELFARE_MIN || welfare_kind > CS_WELFARE_MAX)
    return fail(CS_ERR_INVALID, w + "unknown welfare kind");
  return check_softcap(fn, softcap);
}

// the head of both workspaces: [done counter | pad to 64 B][row counters][welfare keys]
struct BeamCounters {
  uint32_t *done_cnt, *row_cnt, *wkey;
};
BeamCounters beam_counters(char* wsb) {
  return {reinterpret_cast<uint32_t*>(wsb), reinterpret_cast<uint32_t*>(wsb + kBeamRowCntOff),
          reinterpret_cast<uint32_t*>(wsb + kBeamKeyOff)};
}

// More candidates than the launch sorts (n2 > kFusedSort): the launch wrote W, the order
// comes from cs_segmented_topk's kernel behind it.
void beam_sort_after(hipStream_t st, const float* W, int64_t C, int32_t n2, int32_t n_order,
                     int32_t* out_order, float* out_order_val) {
  if (n_order > 0 && n2 > kFusedSort)
    launch_big_lds<&topk_kernel>(kTopkLdsMax, dim3(1), dim3(256),   // B*K > 8192: 128 KiB
                                 static_cast<size_t>(n2) * sizeof(unsigned long long), st, W,
                                 static_cast<int32_t>(C), C, n2, n_order, out_order, out_order_val);
}
}  // namespace

extern "C" {

int cs_beam_select(const float* W, int32_t C, int unfill, const float* U, int32_t A,
                   int32_t n_order, float* out_W, int32_t* out_order, float* out_order_val,
                   float* out_kept, cs_stream_t stream) {
  const char* w = "cs_beam_select: ";
  if (C <= 0 || C > kFusedSort) return fail(CS_ERR_INVALID, std::string(w) + "need 0 < C <= 1024");
  if (n_order <= 0 || n_order > C) return fail(CS_ERR_INVALID, std::string(w) + "need 0 < n_order <= C");
  if (unfill != CS_UNFILL_NONE && unfill != CS_UNFILL_POSINF && unfill != CS_UNFILL_NEGINF)
    return fail(CS_ERR_INVALID, std::string(w) + "unknown unfill mode");
  if (A < 0) return fail(CS_ERR_INVALID, std::string(w) + "need A >= 0");
  if (!W || !out_order || (out_kept && A > 0 && !U))
    return fail(CS_ERR_INVALID, std::string(w) + "NULL pointer");
  const int32_t n2 = next_pow2(C);
  hipLaunchKernelGGL(beam_select_kernel, dim3(1), dim3(kSelectBlock), 0,
                     static_cast<hipStream_t>(stream), W, C, unfill,
                     reinterpret_cast<uint32_t*>(const_cast<float*>(U)), out_kept ? A : 0, out_W,
                     n_order, n2, out_order, out_order_val, out_kept);
  return check_launch("cs_beam_select");
}

size_t cs_beam_step_workspace_size(int64_t rows, int64_t vocab) {
  if (rows <= 0 || vocab <= 0) return 0;
  const SplitPlan p = plan_split(rows, vocab, CS_BF16);
  const SplitPlan q = plan_split(rows, vocab, CS_F32);
  const int64_t ns = p.nsplit > q.nsplit ? p.nsplit : q.nsplit;
  return kBeamCounterBytes + static_cast<size_t>(rows) * pad_line(ns, 8) * sizeof(unsigned long long);
}

int cs_beam_step(const void* logits, int dtype, int32_t A, int32_t B, int64_t vocab, int64_t ld,
                 const int32_t* targets, int32_t K, const float* rewards_in, float softcap,
                 int welfare_kind, float eps, float* out_U, float* out_W, int32_t n_order,
                 int32_t* out_order, float* out_order_val, float* out_kept, void* workspace,
                 size_t workspace_bytes, cs_stream_t stream) {
  const char* fn = "cs_beam_step";
  if (int rc = check_logits(fn, dtype, vocab, ld)) return rc;
  if (A < 0 || B < 0 || K < 0) return fail(CS_ERR_INVALID, std::string(fn) + ": need A, B, K >= 0");
  const int64_t rows = static_cast<int64_t>(A) * B;
  const int64_t C = static_cast<int64_t>(B) * K;
  if (int rc = check_beam_args(fn, rows, C, n_order, out_kept, welfare_kind, softcap)) return rc;
  if (C == 0) return CS_OK;
  if (A == 0) return fail(CS_ERR_INVALID, std::string(fn) + ": no agents");
  if (!logits || !targets || !rewards_in || !out_U || !out_W || (n_order > 0 && !out_order))
    return fail(CS_ERR_INVALID, std::string(fn) + ": NULL pointer");
  if (int rc = check_elt_aligned(fn, logits, dtype)) return rc;
  const SplitPlan plan = plan_split(rows, vocab, dtype);
  const size_t need = kBeamCounterBytes + static_cast<size_t>(rows) * pad_line(plan.nsplit, 8) *
                                              sizeof(unsigned long long);
  if (int rc = check_workspace(fn, workspace, workspace_bytes, need)) return rc;
  if (int rc = check_grid(fn, rows * plan.nsplit)) return rc;
  char* wsb = static_cast<char*>(workspace);
  const BeamCounters c = beam_counters(wsb);
  auto* part = reinterpret_cast<unsigned long long*>(wsb + kBeamCounterBytes);
  const int64_t ld_bytes = ld * elt_size(dtype);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const float inv_cap = softcap > 0.0f ? 1.0f / softcap : 0.0f;
  const int32_t n2 = next_pow2(C);
  const char* lg = static_cast<const char*>(logits);
  // the same streaming arithmetic as cs_logsoftmax_gather (bit-identical lse): unsplit rows
  // one 1024-thread block x 2 vectors per lane, split rows the canonical split form
  // (split_partial), four splits per 1024-thread block
  const dim3 grid(static_cast<uint32_t>(rows * (plan.nsplit > 1 ? split_items(plan.nsplit, 1024) : 1)));
  dispatch_dtype_cap_fixed(dtype, softcap, [&](auto dt, auto cap, auto fixed) {
    hipLaunchKernelGGL(
        (beam_step_kernel<decltype(dt)::value, decltype(cap)::value, decltype(fixed)::value, 1024, 2>),
        grid, dim3(1024), 0, st, lg, vocab, ld_bytes, plan.nsplit, plan.split_len, A, B, K, targets,
        rewards_in, softcap, inv_cap, welfare_kind, static_cast<double>(eps), part, c.row_cnt,
        c.done_cnt, c.wkey, out_U, out_W, n_order, n2, out_order, out_order_val, out_kept);
  });
  beam_sort_after(st, out_W, C, n2, n_order, out_order, out_order_val);
  return check_launch("cs_beam_step");
}

namespace {
// cs_beam_decode_step workspace: [cs_beam_step counters | proposer counters | beam
// counters][row lse][proposer chunk winners][split partials]
struct DecodeLayout {
  SplitPlan plan;
  int32_t kp;
  int32_t nchunk_p;
  size_t lse_off, ids_off, ppart_off, part_off, total;
};
DecodeLayout decode_layout(int32_t A, int32_t B, int64_t vocab, int32_t K, int dtype) {
  DecodeLayout d;
  const int64_t rows = static_cast<int64_t>(A) * B;
  d.plan = plan_split(rows, vocab, dtype);
  d.kp = decode_kp(B, vocab, K, dtype);
  const int64_t ch = static_cast<int64_t>(d.kp) * kDecodeBlock;
  d.nchunk_p = static_cast<int32_t>((vocab + ch - 1) / ch);
  d.lse_off = kBeamCounterBytes + 2 * sizeof(uint32_t) * kBeamMaxBeams;
  d.ids_off = d.lse_off + sizeof(uint32_t) * static_cast<size_t>(B) * pad_line(A, 4);
  d.ppart_off = d.ids_off + sizeof(uint32_t) * static_cast<size_t>(B) * pad_line(K, 4);
  d.part_off = d.ppart_off + sizeof(unsigned long long) * static_cast<size_t>(B) *
                                 pad_line(static_cast<int64_t>(d.nchunk_p) * K, 8);
  d.total = d.part_off + sizeof(unsigned long long) * static_cast<size_t>(rows) *
                             pad_line(d.plan.nsplit, 8);
  return d;
}
}  // namespace

#ifdef CS_TRACE_DECODE
// diagnostics build only: copy the phase timestamps of the last launch and reset them
int cs_trace_read(unsigned long long* out) {
  (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_dec_ts), sizeof(g_dec_ts));
  unsigned long long init[16];
  for (int i = 0; i < 16; ++i) init[i] = (i == 0 || i == 5 || i == 12) ? ~0ull : 0ull;
  (void)hipMemcpyToSymbol(HIP_SYMBOL(g_dec_ts), init, sizeof(init));
  return 0;
}
#endif

size_t cs_beam_decode_workspace_size(int32_t A, int32_t B, int64_t vocab, int32_t K) {
  if (A <= 0 || B <= 0 || vocab <= 0 || K <= 0) return 0;
  const DecodeLayout p = decode_layout(A, B, vocab, K, CS_BF16);
  const DecodeLayout q = decode_layout(A, B, vocab, K, CS_F32);
  return p.total > q.total ? p.total : q.total;
}

int cs_beam_decode_step(const void* ref_logits, int64_t ld_ref, const void* logits, int64_t ld,
                        int dtype, int32_t A, int32_t B, int64_t vocab, int32_t K, float softcap,
                        const float* rewards_in, int welfare_kind, float eps, int32_t* out_ids,
                        float* out_U, float* out_W, int32_t n_order, int32_t* out_order,
                        float* out_order_val, float* out_kept, void* workspace,
                        size_t workspace_bytes, cs_stream_t stream) {
  const char* fn = "cs_beam_decode_step";
  const std::string w = std::string(fn) + ": ";
  if (int rc = check_logits(fn, dtype, vocab, ld)) return rc;
  if (ld_ref < vocab) return fail(CS_ERR_INVALID, w + "need ld_ref >= vocab");
  if (A <= 0 || B <= 0 || K <= 0) return fail(CS_ERR_INVALID, w + "need A, B, K > 0");
  if (K > 256 || K > vocab) return fail(CS_ERR_INVALID, w + "need K <= min(256, vocab)");
  const int64_t rows = static_cast<int64_t>(A) * B;
  const int64_t C = static_cast<int64_t>(B) * K;
  if (int rc = check_beam_args(fn, rows, C, n_order, out_kept, welfare_kind, softcap)) return rc;
  if (B > kBeamMaxBeams) return fail(CS_ERR_INVALID, w + "B exceeds 4096");
  if (!ref_logits || !logits || !rewards_in || !out_ids || !out_U || !out_W ||
      (n_order > 0 && !out_order))
    return fail(CS_ERR_INVALID, w + "NULL pointer");
  if (int rc = check_elt_aligned(fn, logits, dtype)) return rc;
  if (int rc = check_elt_aligned(fn, ref_logits, dtype)) return rc;
  const DecodeLayout d = decode_layout(A, B, vocab, K, dtype);
  if (static_cast<int64_t>(d.nchunk_p) * K > 16384)
    return fail(CS_ERR_INVALID, w + "proposer chunks x K exceeds 16384");
  if (int rc = check_workspace(fn, workspace, workspace_bytes, d.total)) return rc;
  const int64_t row_blocks = rows * (d.plan.nsplit > 1 ? split_items(d.plan.nsplit, kDecodeBlock) : 1);
  const int64_t grid = static_cast<int64_t>(B) * d.nchunk_p + row_blocks;
  if (int rc = check_grid(fn, grid)) return rc;
  char* wsb = static_cast<char*>(workspace);
  const BeamCounters c = beam_counters(wsb);
  auto* prop_cnt = reinterpret_cast<uint32_t*>(wsb + kBeamCounterBytes);
  auto* beam_cnt = prop_cnt + kBeamMaxBeams;
  auto* lse_ws = reinterpret_cast<uint32_t*>(wsb + d.lse_off);
  auto* ids_ws = reinterpret_cast<uint32_t*>(wsb + d.ids_off);
  auto* ppart = reinterpret_cast<unsigned long long*>(wsb + d.ppart_off);
  auto* part = reinterpret_cast<unsigned long long*>(wsb + d.part_off);
  const int64_t esz = elt_size(dtype);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const float inv_cap = softcap > 0.0f ? 1.0f / softcap : 0.0f;
  const int32_t n2 = next_pow2(C);
  const char* rg = static_cast<const char*>(ref_logits);
  const char* lg = static_cast<const char*>(logits);
  const int32_t rows_first = decode_rows_first(row_blocks);
  // 16-byte vector loads in the proposer when every reference row starts 16-B aligned
  const int32_t ref_vec = (reinterpret_cast<uintptr_t>(ref_logits) % 16 == 0 &&
                           (ld_ref * esz) % 16 == 0) ? 1 : 0;
  dispatch_dtype_cap_fixed(dtype, softcap, [&](auto dt, auto cap, auto fixed) {
    constexpr int DT = decltype(dt)::value;
    auto go = [&](auto kp) {
      hipLaunchKernelGGL((beam_decode_kernel<DT, decltype(cap)::value, decltype(fixed)::value, kDecodeBlock,
                                             kDecodeUnroll, decltype(kp)::value>),
                         dim3(grid), dim3(kDecodeBlock), 0, st, rg, ld_ref * esz, d.nchunk_p, rows_first,
                         ref_vec, lg, vocab, ld * esz, d.plan.nsplit, d.plan.split_len, A, B, K,
                         rewards_in, softcap, inv_cap, welfare_kind, static_cast<double>(eps), part,
                         ppart, c.row_cnt, prop_cnt, beam_cnt, c.done_cnt, c.wkey, lse_ws, ids_ws,
                         out_ids, out_U, out_W, n_order, n2, out_order, out_order_val, out_kept);
    };
    if (d.kp == 4) go(std::integral_constant<int, 4>{});
    else go(std::integral_constant<int, kp1024(DT)>{});
  });
  beam_sort_after(st, out_W, C, n2, n_order, out_order, out_order_val);
  return check_launch("cs_beam_decode_step");
}

}  // extern "C"
