// proposer.hip — candidate proposers: vocab top-k and seeded sampling.
#include "cs_kernels.cuh"

namespace {

// One (row, 4096-element chunk) per workgroup: the chunk's k largest composite keys
// (order key, ~token id), descending, zero-padded when the chunk holds fewer than k.
template <int DT, bool CAP>
__global__ __launch_bounds__(256) void vocab_topk_chunk_kernel(
    const char* __restrict__ logits, int64_t vocab, int64_t ld_bytes, int32_t nchunk, int32_t k,
    float cap, float inv_cap, unsigned long long* __restrict__ part) {
  // 32 KB: histogram (16 KB) + candidates (8 KB), or the whole chunk for the fallback sort
  __shared__ __attribute__((aligned(16))) unsigned long long lds[kTopkChunk];
  __shared__ uint32_t sm_w[4];
  __shared__ int sm_res[2];
  __shared__ uint32_t sm_n;
  uint32_t* hist = reinterpret_cast<uint32_t*>(lds);
  unsigned long long* cand = lds + kTopkBins / 2;
  const int tid = threadIdx.x;
  const int64_t row = blockIdx.x / nchunk;
  const int32_t chunk = static_cast<int32_t>(blockIdx.x - row * nchunk);
  const char* rp = logits + row * ld_bytes;
  const int64_t v0 = static_cast<int64_t>(chunk) * kTopkChunk;
  const int n = static_cast<int>(min(static_cast<int64_t>(kTopkChunk), vocab - v0));
#ifdef CS_TRACE_TOPK
  const unsigned long long q0 = wall_clock64();
#endif
  unsigned long long key[kTopkPer];
#pragma unroll
  for (int j = 0; j < kTopkPer; ++j) {
    const int i = tid + 256 * j;
    float x = 0.0f;
    if (i < n) x = load_any<DT>(rp, v0 + i);
    key[j] = 0ull;
    if (i < n) {
      if (CAP) x = softcap_fn(x, cap, inv_cap);
      key[j] = (static_cast<unsigned long long>(order_key(x)) << 32) |
               static_cast<unsigned long long>(0xffffffffu - static_cast<uint32_t>(v0 + i));
    }
  }
  if (tid == 0) sm_n = 0u;
#ifdef CS_TRACE_TOPK
  __syncthreads();
  const unsigned long long q1 = wall_clock64();
#endif
  const RadixCut cut = radix_select<256>(
      [&](auto f) {
#pragma unroll
        for (int j = 0; j < kTopkPer; ++j)
          if (key[j]) f(key[j]);
      },
      static_cast<uint32_t>(k), static_cast<uint32_t>(2 * k + 64), hist, sm_w, sm_res);
#ifdef CS_TRACE_TOPK
  const unsigned long long q2 = wall_clock64();
#endif
  unsigned long long* out = part + (row * nchunk + chunk) * static_cast<int64_t>(k);
  if (cut.count <= kTopkCand) {  // block-uniform (always, unless > 1024 keys tie exactly)
#pragma unroll
    for (int j = 0; j < kTopkPer; ++j)
      if (key[j] && (key[j] >> cut.shift) >= cut.prefix) cand[atomicAdd(&sm_n, 1u)] = key[j];
    __syncthreads();
    const int nc = static_cast<int>(sm_n);
    rank_candidates(cand, nc, k, [&](int r, unsigned long long kc) { out[r] = kc; });
    for (int r = nc + tid; r < k; r += 256) out[r] = 0ull;
#ifdef CS_TRACE_TOPK
    __syncthreads();
    if (tid == 0 && blockIdx.x % 97 == 0)
      printf("TOPK chunk %d load %llu select %llu rank %llu nc %d levels %d (x10ns)\n", (int)blockIdx.x,
             q1 - q0, q2 - q1, wall_clock64() - q2, nc, (52 - cut.shift) / 12 + 1);
#endif
    return;
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < kTopkPer; ++j) lds[tid + 256 * j] = key[j];
  __syncthreads();
  bitonic_desc(lds, kTopkChunk, tid, 256);
  for (int r = tid; r < k; r += 256) out[r] = lds[r];
}

__device__ __forceinline__ void emit_token(int32_t* ids, float* vals, int64_t at,
                                           unsigned long long c) {
  ids[at] = static_cast<int32_t>(0xffffffffu - static_cast<uint32_t>(c & 0xffffffffull));
  if (vals) vals[at] = key_to_float(static_cast<uint32_t>(c >> 32));
}

// One row per workgroup: the k largest of the row's nkeys chunk winners (zero = padding).
// Dynamic LDS: max(n2, 4096) keys (histogram + candidates, or the fallback sort).
__global__ __launch_bounds__(256) void vocab_topk_merge_kernel(
    const unsigned long long* __restrict__ part, int32_t nkeys, int32_t n2, int32_t k,
    int32_t* __restrict__ out_ids, float* __restrict__ out_vals) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long mk[];
  __shared__ uint32_t sm_w[4];
  __shared__ int sm_res[2];
  __shared__ uint32_t sm_n;
  uint32_t* hist = reinterpret_cast<uint32_t*>(mk);
  unsigned long long* cand = mk + kTopkBins / 2;
  const int tid = threadIdx.x;
  const int64_t row = blockIdx.x;
  const unsigned long long* pr = part + row * nkeys;
  if (tid == 0) sm_n = 0u;
  const RadixCut cut = radix_select<256>(
      [&](auto f) {
        for (int i = tid; i < nkeys; i += 256) {
          const unsigned long long c = pr[i];
          if (c) f(c);
        }
      },
      static_cast<uint32_t>(k), static_cast<uint32_t>(2 * k + 64), hist, sm_w, sm_res);
  if (cut.count <= kTopkCand) {  // block-uniform
    for (int i = tid; i < nkeys; i += 256) {
      const unsigned long long c = pr[i];
      if (c && (c >> cut.shift) >= cut.prefix) cand[atomicAdd(&sm_n, 1u)] = c;
    }
    __syncthreads();
    const int nc = static_cast<int>(sm_n);
    rank_candidates(cand, nc, k,
                    [&](int r, unsigned long long c) { emit_token(out_ids, out_vals, row * k + r, c); });
    for (int r = nc + tid; r < k; r += 256) emit_token(out_ids, out_vals, row * k + r, 0ull);
    return;
  }
  __syncthreads();
  for (int i = tid; i < n2; i += 256) mk[i] = (i < nkeys) ? pr[i] : 0ull;
  __syncthreads();
  bitonic_desc(mk, n2, tid, 256);
  for (int r = tid; r < k; r += 256) emit_token(out_ids, out_vals, row * k + r, mk[r]);
}

// Counter-based uniform strictly inside (0, 1): splitmix64 finaliser of (seed, token), top
// 23 bits + 0.5 (exactly representable in fp32).  oracle/oracle.py:cs_uniform restates it
// bit for bit.
__device__ __forceinline__ float cs_uniform(unsigned long long seed, unsigned long long v) {
  unsigned long long x = seed * 0x9E3779B97F4A7C15ull + (v + 1ull) * 0xD1B54A32D192ED03ull;
  x ^= x >> 30;
  x *= 0xBF58476D1CE4E5B9ull;
  x ^= x >> 27;
  x *= 0x94D049BB133111EBull;
  x ^= x >> 31;
  return (static_cast<float>(static_cast<uint32_t>(x >> 41)) + 0.5f) * (1.0f / 8388608.0f);
}

struct DrawBest {
  float s;
  int32_t idx;
};

__device__ __forceinline__ void draw_merge(float& s, int32_t& i, float s2, int32_t i2) {
  if (s2 > s || (s2 == s && i2 < i)) {
    s = s2;
    i = i2;
  }
}

// The streaming stage's two template axes.  STEP (cs_sample_step, cs_sample_step_ex): the row's
// one seed is derived on the device from (base seed, *step), and a finished stream's workgroups
// leave before they touch its row.  TABLES: how many LDS bitmaps over the workgroup's slice of
// the vocabulary.  1 (cs_sample_step with a bias list): the listed tokens take bias_value in
// fp32 before the soft-cap.  2 (the *_ex entries): a second bitmap marks the row's seen tokens,
// which take the repetition penalty after the soft-cap, and with `greedy` the score is the
// transformed logit itself (no seed read, no Gumbel noise).  3 (the *_dfa entries): the two
// bitmaps of 2, and one bit per token read from GLOBAL memory -- row dfa_state[row] of the
// automaton's token masks -- whose clear bit makes the transformed logit -inf: out of the
// log-sum-exp and, by the never-drawn rule, out of the draw.
struct StepIn {
  const int32_t* step;
  const int32_t* done;
  const int32_t* bias_ids;
  int32_t n_bias;
  float bias_value;
  // the *_ex entries only
  const int32_t* seen_ids;     // ragged per-row lists: seen_ids[seen_off[r] : seen_off[r+1]]
  const int32_t* seen_off;     // NULL: no list
  const int32_t* out_tokens;   // step entry: out_tokens[s][0 : out_len[s]] joins the seen set
  const int32_t* out_len;
  int32_t max_tokens;
  float penalty;               // 1: off, the seen set is not looked at
  int32_t greedy;
  // the *_dfa entries only
  const uint32_t* masks;       // [n_states][mask_words], bit v of row q: token v drawable in q
  const int32_t* dfa_state;    // per row; a state outside [0, n_states) allows nothing
  int32_t mask_words, n_states;
};
constexpr unsigned long long kSeedMul = 1000003ull;   // runtime.draw_seed
constexpr int64_t kMaxBiasSlice = 1 << 19;            // bitmap <= 64 KB of LDS
constexpr size_t kExLdsLimit = 2 * (kMaxBiasSlice / 8);   // the two bitmaps of an *_ex slice

// transformers' RepetitionPenaltyLogitsProcessor on one fp32 logit (a true division)
__device__ __forceinline__ float penalise(float x, float penalty) {
  return x < 0.0f ? x * penalty : __fdiv_rn(x, penalty);
}

// wave-wide: is token i among ids[0 : n)?
__device__ __forceinline__ bool wave_listed(const int32_t* ids, int64_t n, int32_t i, int lane) {
  bool hit = false;
  for (int64_t j = lane; j < n; j += 64) hit |= ids[j] == i;
  return __ballot(hit) != 0ull;
}

// how many generated tokens of a stream join its seen set: out_len, kept inside the buffer
__device__ __forceinline__ int32_t seen_out_len(int32_t len, int32_t max_tokens) {
  return len < 0 ? 0 : (len > max_tokens ? max_tokens : len);
}

// wave-wide: is token i in row's seen set (its list, and the n_gen generated tokens at gen)?
__device__ __forceinline__ bool wave_seen(const StepIn& in, int64_t row, int32_t i, int lane,
                                          const int32_t* gen, int32_t n_gen) {
  if (in.penalty == 1.0f) return false;
  bool hit = false;
  if (in.seen_off) {
    const int64_t a = in.seen_off[row];
    hit = wave_listed(in.seen_ids + a, in.seen_off[row + 1] - a, i, lane);
  }
  if (n_gen > 0) hit |= wave_listed(gen, n_gen, i, lane);
  return hit;
}

// Token i's transformed logit: the one statement of the rule, for the streaming stage and for
// every log-probability (no list: biased = seen = false)
template <int DT, bool CAP>
__device__ __forceinline__ float ex_logit(const char* rp, int64_t i, bool biased, bool seen,
                                          const StepIn& in, float cap, float inv_cap) {
  float x = load_any<DT>(rp, i);
  if (biased) x += in.bias_value;
  if (CAP) x = softcap_fn(x, cap, inv_cap);
  if (seen) x = penalise(x, in.penalty);
  return x;
}

// the LDS bitmaps: one bit per token of the workgroup's slice [v0, v1)
__device__ __forceinline__ void mark(uint32_t* bits, int64_t id, int64_t v0, int64_t v1) {
  if (id >= v0 && id < v1) atomicOr(&bits[(id - v0) >> 5], 1u << ((id - v0) & 31));
}
__device__ __forceinline__ bool marked(const uint32_t* bits, int64_t o) {
  return (bits[o >> 5] >> (o & 31)) & 1u;
}

template <int DT, bool CAP, bool STEP, int TABLES>
__global__ __launch_bounds__(256) void vocab_sample_kernel(
    const char* __restrict__ logits, int64_t vocab, int64_t ld_bytes, int32_t nsplit,
    int64_t split_len, float inv_temp, float cap, float inv_cap,
    const unsigned long long* __restrict__ seeds, int32_t n_draw, float2* __restrict__ lse_part,
    DrawBest* __restrict__ draw_part, StepIn in) {
  extern __shared__ uint32_t sm_bias[];   // TABLES >= 1; the seen bitmap (TABLES == 2) after it
  __shared__ float sm_m[4], sm_s[4];
  __shared__ float sm_bs[4][kMaxDraws];
  __shared__ int32_t sm_bi[4][kMaxDraws];
  const int tid = threadIdx.x;
  const int64_t bid = blockIdx.x;
  const int64_t row = bid / nsplit;
  if (STEP && in.done[row] != 0) return;   // block-uniform, before any barrier
  const int32_t split = static_cast<int32_t>(bid - row * nsplit);
  const char* rp = logits + row * ld_bytes;
  const int64_t v0 = static_cast<int64_t>(split) * split_len;
  const int64_t v1 = min(vocab, v0 + split_len);
  const int nw = static_cast<int>((v1 - v0 + 31) >> 5);
  uint32_t* sm_seen = sm_bias + nw;
  constexpr int kBitmaps = TABLES > 2 ? 2 : TABLES;
  if (TABLES > 0) {
    for (int w = tid; w < kBitmaps * nw; w += 256) sm_bias[w] = 0u;
    __syncthreads();
    for (int j = tid; j < in.n_bias; j += 256) mark(sm_bias, in.bias_ids[j], v0, v1);
    if (TABLES >= 2 && in.penalty != 1.0f) {
      if (in.seen_off) {
        const int64_t b = in.seen_off[row + 1];
        for (int64_t j = in.seen_off[row] + tid; j < b; j += 256)
          mark(sm_seen, in.seen_ids[j], v0, v1);
      }
      if (STEP) {
        const int32_t len = seen_out_len(in.out_len[row], in.max_tokens);
        for (int j = tid; j < len; j += 256)
          mark(sm_seen, in.out_tokens[row * in.max_tokens + j], v0, v1);
      }
    }
    __syncthreads();
  }
  const bool greedy = TABLES >= 2 && in.greedy != 0;
  const uint32_t* allow = nullptr;   // TABLES == 3: the mask row of the row's state
  if (TABLES == 3) {
    const int32_t q = in.dfa_state[row];
    if (q >= 0 && q < in.n_states) allow = in.masks + static_cast<int64_t>(q) * in.mask_words;
  }
  unsigned long long sd[kMaxDraws];
  float bs[kMaxDraws];
  int32_t bi[kMaxDraws];
#pragma unroll
  for (int d = 0; d < kMaxDraws; ++d) {
    sd[d] = (d < n_draw && !greedy) ? seeds[row * n_draw + d] : 0ull;
    bs[d] = -INFINITY;
    bi[d] = 0x7fffffff;
  }
  if (STEP && !greedy)   // n_draw = 1
    sd[0] = sd[0] * kSeedMul + static_cast<unsigned long long>(static_cast<int64_t>(*in.step));
  float m = -INFINITY, s = 0.0f;
  bool saw_nan = false;
  for (int64_t v = v0 + tid; v < v1; v += 256) {
    const bool biased = TABLES > 0 && marked(sm_bias, v - v0);
    const bool seen = TABLES >= 2 && marked(sm_seen, v - v0);
    // a clear bit: the logit is not loaded at all (measured 1.5 us per step cheaper at 64 x
    // 128,256 than loading it beside the mask word and discarding it)
    const bool dead = TABLES == 3 && !(allow && ((allow[v >> 5] >> (v & 31)) & 1u));
    const float y =
        dead ? -INFINITY : ex_logit<DT, CAP>(rp, v, biased, seen, in, cap, inv_cap) * inv_temp;
    saw_nan |= y != y;
    lse_accum<1>(m, s, &y);
#pragma unroll
    for (int d = 0; d < kMaxDraws; ++d) {
      if (d < n_draw) {
        float sc = y;
        if (!greedy) {
          const float u = cs_uniform(sd[d], static_cast<unsigned long long>(v));
          sc = y - logf(-logf(u));
        }
        if (sc > bs[d]) {
          bs[d] = sc;
          bi[d] = static_cast<int32_t>(v);
        }
      }
    }
  }
  // a NaN token must poison the row's lse wherever it sits, also one that arrives while
  // (m, s) is still empty (lse_accum leaves (0, NaN) then; saw_nan does not depend on it):
  // (0, NaN) survives every merge, also with empty partners
  if (saw_nan) {
    if (m == -INFINITY) m = 0.0f;
    s = __builtin_nanf("");
  }
  wave_lse_reduce(m, s);
#pragma unroll
  for (int d = 0; d < kMaxDraws; ++d) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      const float s2 = __shfl_xor(bs[d], o, 64);
      const int32_t i2 = __shfl_xor(bi[d], o, 64);
      draw_merge(bs[d], bi[d], s2, i2);
    }
  }
  const int wave = tid >> 6;
  if ((tid & 63) == 0) {
    sm_m[wave] = m;
    sm_s[wave] = s;
#pragma unroll
    for (int d = 0; d < kMaxDraws; ++d) {
      sm_bs[wave][d] = bs[d];
      sm_bi[wave][d] = bi[d];
    }
  }
  __syncthreads();
  if (tid == 0) {
    float mm = sm_m[0], ss = sm_s[0];
    for (int w = 1; w < 4; ++w) lse_merge(mm, ss, sm_m[w], sm_s[w]);
    lse_part[bid] = make_float2(mm, ss);
  }
  if (tid < n_draw) {
    float b = sm_bs[0][tid];
    int32_t i = sm_bi[0][tid];
    for (int w = 1; w < 4; ++w) draw_merge(b, i, sm_bs[w][tid], sm_bi[w][tid]);
    draw_part[bid * n_draw + tid] = DrawBest{b, i};
  }
}

// The split merge of every second stage, called by a whole wave: the row's lse (to every lane)
// and draw column `col` merged in split order, so that ties keep the lower token id.  One
// body, so the plain and the step entries agree on the id and on the lse bit for bit.  No
// split offered a candidate (every logit -inf or NaN), or col >= n_draw: idx 0x7fffffff.
__device__ __forceinline__ DrawBest merge_splits(const float2* __restrict__ lse_part,
                                                 const DrawBest* __restrict__ draw_part,
                                                 int64_t row, int32_t nsplit, int32_t n_draw,
                                                 int32_t col, int lane, float& lse) {
  float m = -INFINITY, s = 0.0f;
  for (int j = lane; j < nsplit; j += 64) {
    const float2 p = lse_part[row * nsplit + j];
    lse_merge(m, s, p.x, p.y);
  }
  wave_lse_reduce(m, s);
  lse = m + logf(s);
  float b = -INFINITY;
  int32_t i = 0x7fffffff;
  if (col < n_draw) {
    for (int j = 0; j < nsplit; ++j) {
      const DrawBest p = draw_part[(row * nsplit + j) * n_draw + col];
      draw_merge(b, i, p.s, p.idx);
    }
  }
  return DrawBest{b, i};
}

// Second stage of the plain entries, one wave per row: lane d owns draw d (n_draw <= 16).
// EX (cs_vocab_sample_ex): the drawn token's log-probability is taken on its transformed
// logit, so the wave looks every draw's id up in the bias and seen lists.
template <int DT, bool CAP, bool EX>
__global__ __launch_bounds__(64) void vocab_sample_merge_kernel(
    const char* __restrict__ logits, int64_t ld_bytes, int32_t nsplit, float inv_temp, float cap,
    float inv_cap, const float2* __restrict__ lse_part, const DrawBest* __restrict__ draw_part,
    int32_t n_draw, int32_t* __restrict__ out_ids, float* __restrict__ out_lp, StepIn in) {
  const int64_t row = blockIdx.x;
  const int lane = threadIdx.x;
  float lse;
  const int32_t i = merge_splits(lse_part, draw_part, row, nsplit, n_draw, lane, lane, lse).idx;
  bool biased = false, seen = false;
  if constexpr (EX) {
    for (int d = 0; d < n_draw; ++d) {
      const int32_t id = __shfl(i, d, 64);
      const bool b = wave_listed(in.bias_ids, in.n_bias, id, lane);
      const bool sn = wave_seen(in, row, id, lane, nullptr, 0);
      if (lane == d) {
        biased = b;
        seen = sn;
      }
    }
  }
  if (lane < n_draw) {
    // no candidate: id -1 and NaN, nothing read
    const bool none = i == 0x7fffffff;
    out_ids[row * n_draw + lane] = none ? -1 : i;
    if (out_lp) {
      float lp = __builtin_nanf("");
      if (!none)
        lp = ex_logit<DT, CAP>(logits + row * ld_bytes, i, biased, seen, in, cap, inv_cap) *
                 inv_temp - lse;
      out_lp[row * n_draw + lane] = lp;
    }
  }
}

// The stop strings of cs_sample_step_ex, passed by value: the bytes of string k are
// bytes[off[k] : off[k+1]], at most kMaxStopSeq strings of at most kMaxStopLen bytes.
constexpr int kMaxDfaStates = 1024;   // cs_dfa_token_masks and the *_dfa entries
constexpr int kMaxStopSeq = 8;
constexpr int kMaxStopLen = 32;
struct StopSeqs {
  const uint8_t* tok_bytes;   // token v's bytes: tok_bytes[tok_off[v] : tok_off[v+1]]
  const int32_t* tok_off;
  uint8_t* tail;              // [S][kMaxStopLen]: the last tail_len[s] < 32 bytes of the stream
  int32_t* tail_len;
  int32_t n_seq;
  int32_t off[kMaxStopSeq + 1];
  uint8_t bytes[kMaxStopSeq * kMaxStopLen];
  // cs_sample_step_dfa: the automaton an appended token's bytes are walked through
  const int16_t* trans;       // [n_states][256], -1 dead; NULL: no automaton
  int32_t* dfa_state;         // [S]
  int32_t n_states;
};
struct NoStopSeqs {};

// The state after token i's bytes from state q: -1 once a byte has no transition (or q is no
// state), q itself for a token with no bytes.
__device__ __forceinline__ int32_t dfa_walk(const StopSeqs& sq, int32_t q, int32_t i) {
  const int32_t t0 = sq.tok_off[i], t1 = sq.tok_off[i + 1];
  for (int32_t p = t0; p < t1; ++p) {
    if (q < 0 || q >= sq.n_states) return -1;
    q = sq.trans[q * 256 + sq.tok_bytes[p]];
  }
  return (q < 0 || q >= sq.n_states) ? -1 : q;
}

// Wave-wide, after token i was appended to stream `row`: does a stop string end inside the
// token's bytes in the window tail ++ bytes(i)?  Lanes take the end positions; every byte of
// the new tail is read before any is written (a lane's store waits for the wave's loads).
__device__ __forceinline__ bool stop_window(const StopSeqs& sq, int64_t row, int32_t i, int lane) {
  const int32_t t0 = sq.tok_off[i];
  const int32_t nb = sq.tok_off[i + 1] - t0;
  if (nb <= 0) return false;   // a special token: the window stands
  int32_t tl = sq.tail_len[row];
  tl = tl < 0 ? 0 : (tl > kMaxStopLen - 1 ? kMaxStopLen - 1 : tl);
  uint8_t* tail = sq.tail + row * kMaxStopLen;
  const uint8_t* tb = sq.tok_bytes + t0;
  const int32_t wl = tl + nb;
  auto at = [&](int32_t p) -> uint8_t { return p < tl ? tail[p] : tb[p - tl]; };
  bool hit = false;
  for (int32_t e = tl + 1 + lane; e <= wl && !hit; e += 64) {   // e: one past the last byte
    for (int k = 0; k < sq.n_seq && !hit; ++k) {
      const int32_t o = sq.off[k], len = sq.off[k + 1] - o;
      if (len > e) continue;
      bool same = true;
      for (int32_t j = 0; j < len && same; ++j) same = at(e - len + j) == sq.bytes[o + j];
      hit = same;
    }
  }
  const int32_t nt = wl < kMaxStopLen - 1 ? wl : kMaxStopLen - 1;
  const uint8_t keep = lane < nt ? at(wl - nt + lane) : uint8_t{0};
  if (lane < nt) tail[lane] = keep;
  if (lane == 0) sq.tail_len[row] = nt;
  return __ballot(hit) != 0ull;
}

// cs_sample_step's second stage, one wave per stream: merge_splits (so the id and the log-prob
// are vocab_sample_merge_kernel's bits), then the stream's state update and the next step's
// input token.  Lane 0 of every workgroup adds
// (1 << 32 | still alive) to the workspace's one counter word; the last arrival has the
// number of unfinished streams in the low half, writes it and leaves the word at zero.
// EX (cs_sample_step_ex): the log-probability is taken on the transformed logit (bias,
// soft-cap, penalty over the seen list and the tokens generated so far), and an appended
// token runs the stop-string window.
template <int DT, bool CAP, bool EX>
__global__ __launch_bounds__(64) void sample_step_merge_kernel(
    const char* __restrict__ logits, int64_t ld_bytes, int32_t nsplit, float inv_temp, float cap,
    float inv_cap, const float2* __restrict__ lse_part, const DrawBest* __restrict__ draw_part,
    StepIn in, const int32_t* __restrict__ stop_ids, int32_t n_stop, int32_t max_tokens,
    int32_t pad_id, int32_t* __restrict__ done, int32_t* __restrict__ out_len,
    int32_t* __restrict__ out_tokens, float* __restrict__ out_lp,
    long long* __restrict__ next_tok, int32_t* __restrict__ n_alive,
    unsigned long long* __restrict__ arrivals, std::conditional_t<EX, StopSeqs, NoStopSeqs> sq) {
  const int64_t row = blockIdx.x;
  const int lane = threadIdx.x;
  int32_t next = pad_id;
  uint32_t alive = 0u;
  if (done[row] == 0) {   // block-uniform
    float lse;
    const int32_t i = merge_splits(lse_part, draw_part, row, nsplit, 1, 0, lane, lse).idx;
    const bool biased = wave_listed(in.bias_ids, in.n_bias, i, lane);
    bool seen = false;
    if constexpr (EX)   // the seen set as the streaming stage saw it: before this step's append
      seen = wave_seen(in, row, i, lane, out_tokens + row * max_tokens,
                       seen_out_len(out_len[row], max_tokens));
    int32_t appended = 0;
    if (lane == 0) {
      bool stop = i == 0x7fffffff;   // no drawable logit: the stream ends
      for (int j = 0; j < n_stop; ++j) stop |= stop_ids[j] == i;
      const int32_t len = out_len[row];
      // a length outside [0, max_tokens) has no slot to append to: the stream ends as well
      if (stop || len < 0 || len >= max_tokens) {
        done[row] = 1;
      } else {
        const int64_t at = row * max_tokens + len;
        out_tokens[at] = i;
        if (out_lp)
          out_lp[at] = ex_logit<DT, CAP>(logits + row * ld_bytes, i, biased, seen, in, cap,
                                         inv_cap) * inv_temp - lse;
        out_len[row] = len + 1;
        appended = 1;
        if (len + 1 == max_tokens) {
          done[row] = 1;
        } else {
          next = i;
          alive = 1u;
        }
      }
    }
    if constexpr (EX) {
      if (sq.trans && lane == 0 && appended != 0)
        sq.dfa_state[row] = dfa_walk(sq, sq.dfa_state[row], i);
      if (sq.n_seq > 0 && __shfl(appended, 0, 64) != 0) {   // wave-uniform
        if (stop_window(sq, row, i, lane) && lane == 0) {
          done[row] = 1;   // the token stays appended: the host's cut sees the whole occurrence
          next = pad_id;
          alive = 0u;
        }
      }
    }
  }
  if (lane == 0) {
    next_tok[row] = next;
    const unsigned long long old = __hip_atomic_fetch_add(
        arrivals, (1ull << 32) | alive, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if ((old >> 32) == static_cast<unsigned long long>(gridDim.x) - 1ull) {
      n_alive[0] = static_cast<int32_t>((old & 0xffffffffull) + alive);
      __hip_atomic_store(arrivals, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

int32_t topk_nchunk(int64_t vocab) {
  return static_cast<int32_t>((vocab + kTopkChunk - 1) / kTopkChunk);
}

// What the four sampling entries share once their own argument checks have passed:
// cs_vocab_sample's split plan (for every entry and dtype: one plan is what makes their bits
// one), the workspace carved into [arrival word |] lse_part | draw_part, and the launches'
// scalars.
struct SampleCall {
  int dtype;
  SplitPlan plan;
  uint32_t rows, grid;            // grid: one streaming workgroup per (row, split)
  unsigned long long* arrivals;   // the step entries' counter word
  float2* lse_part;
  DrawBest* draw_part;
  const char* lg;
  int64_t vocab, ld_bytes;
  float cap, inv_cap, inv_t;
  const unsigned long long* seeds;
  int32_t n_draw;
  hipStream_t st;
};

// `slice_msg`: the entry's text for a slice that outgrows its LDS bitmaps, NULL without bitmaps.
// temperature 0 (greedy, the *_ex entries) scores the logit itself.
int plan_sample(SampleCall& c, const char* fn, const void* logits, int dtype, int64_t rows,
                int64_t vocab, int64_t ld, float temperature, float softcap, const uint64_t* seeds,
                int32_t n_draw, void* workspace, size_t workspace_bytes, bool arrival_word,
                const char* slice_msg, cs_stream_t stream) {
  c.plan = plan_split(rows, vocab, CS_F32);   // elementwise loop: same split for every dtype
  if (int rc = check_grid(fn, rows * c.plan.nsplit)) return rc;
  if (slice_msg && c.plan.split_len > kMaxBiasSlice)
    return fail(CS_ERR_INVALID, std::string(fn) + slice_msg);
  const size_t head = arrival_word ? sizeof(unsigned long long) : 0;
  if (int rc = check_workspace(fn, workspace, workspace_bytes,
                               head + cs_vocab_sample_workspace_size(rows, vocab, n_draw)))
    return rc;
  c.dtype = dtype;
  c.rows = static_cast<uint32_t>(rows);
  c.grid = static_cast<uint32_t>(rows * c.plan.nsplit);
  c.arrivals = static_cast<unsigned long long*>(workspace);
  c.lse_part = reinterpret_cast<float2*>(static_cast<char*>(workspace) + head);
  c.draw_part = reinterpret_cast<DrawBest*>(c.lse_part + rows * c.plan.nsplit);
  c.lg = static_cast<const char*>(logits);
  c.vocab = vocab;
  c.ld_bytes = ld * elt_size(dtype);
  c.cap = softcap;
  c.inv_cap = softcap > 0.0f ? 1.0f / softcap : 0.0f;
  c.inv_t = temperature == 0.0f ? 1.0f : 1.0f / temperature;
  c.seeds = reinterpret_cast<const unsigned long long*>(seeds);
  c.n_draw = n_draw;
  c.st = static_cast<hipStream_t>(stream);
  return CS_OK;
}

// The streaming stage.  Beside the kernel's static arrays the two bitmaps of an *_ex slice pass
// the default 64 KiB of LDS from about 2^18 tokens (the one bitmap of a biased step at 2^19),
// so the limit is raised before it is met.
template <int DT, bool CAP, bool STEP, int TABLES>
void launch_stream(const SampleCall& c, const StepIn& in) {
  const size_t lds =
      (TABLES > 2 ? 2 : TABLES) * static_cast<size_t>((c.plan.split_len + 31) / 32) * sizeof(uint32_t);
  launch_big_lds<&vocab_sample_kernel<DT, CAP, STEP, TABLES>, 60 * 1024>(
      kExLdsLimit, dim3(c.grid), dim3(256), lds, c.st, c.lg, c.vocab, c.ld_bytes, c.plan.nsplit,
      c.plan.split_len, c.inv_t, c.cap, c.inv_cap, c.seeds, c.n_draw, c.lse_part, c.draw_part, in);
}

// both stages of the plain entries (TABLES 0: cs_vocab_sample, 2: cs_vocab_sample_ex,
// 3: cs_vocab_sample_dfa; a drawn token's bit is set, so the merge stage is that of 2)
template <int TABLES>
int launch_plain(const char* fn, const SampleCall& c, const StepIn& in, int32_t* out_ids,
                 float* out_lp) {
  dispatch_dtype_cap(c.dtype, c.cap, [&](auto dt, auto cap) {
    constexpr int DT = decltype(dt)::value;
    constexpr bool CAP = decltype(cap)::value;
    launch_stream<DT, CAP, false, TABLES>(c, in);
    hipLaunchKernelGGL((vocab_sample_merge_kernel<DT, CAP, TABLES >= 2>), dim3(c.rows), dim3(64), 0,
                       c.st, c.lg, c.ld_bytes, c.plan.nsplit, c.inv_t, c.cap, c.inv_cap, c.lse_part,
                       c.draw_part, c.n_draw, out_ids, out_lp, in);
  });
  return check_launch(fn);
}

// the state arguments of the two step entries
struct StepState {
  const int32_t* stop_ids;
  int32_t n_stop, max_tokens, pad_id;
  int32_t *done, *out_len, *out_tokens;
  float* out_lp;   // optional
  int64_t* next_tok;
  int32_t* n_alive;
};

// `bad_counts`: the entry's own text when one of its list counts is out of range, else NULL
int check_step_state(const char* fn, int64_t S, int64_t vocab, const StepState& s,
                     const char* bad_counts) {
  if (S < 0) return fail(CS_ERR_INVALID, std::string(fn) + ": need S >= 0");
  if (bad_counts) return fail(CS_ERR_INVALID, std::string(fn) + bad_counts);
  if (s.max_tokens < 1) return fail(CS_ERR_INVALID, std::string(fn) + ": need max_tokens >= 1");
  if (s.pad_id < 0 || s.pad_id >= vocab)
    return fail(CS_ERR_INVALID, std::string(fn) + ": pad_id outside [0, vocab)");
  return CS_OK;
}

// a greedy step reads no seed
bool step_ptr_missing(const void* logits, const uint64_t* base_seeds, bool greedy, const StepIn& in,
                      const StepState& s) {
  return !logits || (!greedy && !base_seeds) || !in.step || !s.done || !s.out_len ||
         !s.out_tokens || !s.next_tok || !s.n_alive || (in.n_bias > 0 && !in.bias_ids) ||
         (s.n_stop > 0 && !s.stop_ids);
}

// both stages of the step entries (TABLES 0 or 1: cs_sample_step, 2: cs_sample_step_ex,
// 3: cs_sample_step_dfa)
template <int TABLES, typename Seqs>
int launch_step(const char* fn, const SampleCall& c, const StepIn& in, const StepState& s,
                const Seqs& sq) {
  dispatch_dtype_cap(c.dtype, c.cap, [&](auto dt, auto cap) {
    constexpr int DT = decltype(dt)::value;
    constexpr bool CAP = decltype(cap)::value;
    launch_stream<DT, CAP, true, TABLES>(c, in);
    hipLaunchKernelGGL((sample_step_merge_kernel<DT, CAP, TABLES >= 2>), dim3(c.rows), dim3(64), 0,
                       c.st, c.lg, c.ld_bytes, c.plan.nsplit, c.inv_t, c.cap, c.inv_cap, c.lse_part,
                       c.draw_part, in, s.stop_ids, s.n_stop, s.max_tokens, s.pad_id, s.done,
                       s.out_len, s.out_tokens, s.out_lp, reinterpret_cast<long long*>(s.next_tok),
                       s.n_alive, c.arrivals, sq);
  });
  return check_launch(fn);
}

// temperature 0 is greedy; a penalty of 1 is off
int check_controls(const char* fn, float temperature, float penalty, int32_t n_bias) {
  if (!(temperature >= 0.0f) || std::isinf(temperature))
    return fail(CS_ERR_INVALID, std::string(fn) + ": temperature must be finite and >= 0");
  if (!(penalty > 0.0f) || std::isinf(penalty))
    return fail(CS_ERR_INVALID, std::string(fn) + ": repetition_penalty must be finite and > 0");
  if (n_bias < 0 || n_bias > 1024)
    return fail(CS_ERR_INVALID, std::string(fn) + ": need 0 <= n_bias <= 1024");
  return CS_OK;
}

// The automaton arguments of the *_dfa entries (masks != NULL), checked by check_dfa.
struct DfaArgs {
  const uint32_t* masks;
  int64_t mask_words;
  int32_t n_states;
  const int32_t* state;    // plain entry: read; step entry: read and advanced
  const int16_t* trans;    // step entry only
};

int check_dfa(const char* fn, const DfaArgs& d, int64_t vocab, bool step, const void* tok_bytes,
              const void* tok_off) {
  if (d.n_states < 1 || d.n_states > kMaxDfaStates)
    return fail(CS_ERR_INVALID, std::string(fn) + ": need 1 <= n_states <= 1024");
  if (d.mask_words < (vocab + 31) / 32 || d.mask_words > INT32_MAX)
    return fail(CS_ERR_INVALID, std::string(fn) + ": mask_words below ceil(vocab / 32)");
  if (!d.state || (step && (!d.trans || !tok_bytes || !tok_off)))
    return fail(CS_ERR_INVALID, std::string(fn) + ": NULL pointer");
  return CS_OK;
}

void set_dfa(StepIn& in, const DfaArgs& d) {
  in.masks = d.masks;
  in.dfa_state = d.state;
  in.mask_words = static_cast<int32_t>(d.mask_words);
  in.n_states = d.n_states;
}

// cs_dfa_token_masks: one thread per (state, token), a wave's ballot is two mask words.
__global__ __launch_bounds__(256) void dfa_token_masks_kernel(
    const int16_t* __restrict__ trans, const uint8_t* __restrict__ accept, int32_t n_states,
    const uint8_t* __restrict__ tok_bytes, const int32_t* __restrict__ tok_off, int64_t vocab,
    int64_t words, const int32_t* __restrict__ stop_ids, int32_t n_stop,
    uint32_t* __restrict__ masks) {
  const int32_t q0 = blockIdx.y;
  const int64_t v = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  bool alive = false;
  if (v < vocab) {
    bool is_stop = false;
    for (int j = 0; j < n_stop; ++j) is_stop |= stop_ids[j] == v;
    if (is_stop) {
      alive = accept[q0] != 0;
    } else {
      const int32_t t0 = tok_off[v], t1 = tok_off[v + 1];
      int32_t q = q0;
      for (int32_t p = t0; p < t1 && q >= 0; ++p) {
        q = trans[q * 256 + tok_bytes[p]];
        if (q >= n_states) q = -1;   // no state: a malformed table reads nothing out of bounds
      }
      alive = t1 > t0 && q >= 0;
    }
  }
  const unsigned long long bits = __ballot(alive);
  const int lane = threadIdx.x & 63;
  const int64_t w = (v - lane) >> 5;   // the wave's first word
  if (lane == 0 && w < words) masks[q0 * words + w] = static_cast<uint32_t>(bits);
  if (lane == 32 && w + 1 < words) masks[q0 * words + w + 1] = static_cast<uint32_t>(bits >> 32);
}

// cs_vocab_sample_ex (dfa NULL) and cs_vocab_sample_dfa with masks
int vocab_sample_ex_body(const char* fn, const void* logits, int dtype, int64_t rows, int64_t vocab,
                         int64_t ld, float temperature, float softcap, const uint64_t* seeds,
                         int32_t n_draw, const int32_t* bias_ids, int32_t n_bias, float bias_value,
                         float repetition_penalty, const int32_t* seen_ids, const int32_t* seen_off,
                         const DfaArgs* dfa, int32_t* out_ids, float* out_lp, void* workspace,
                         size_t workspace_bytes, cs_stream_t stream) {
  if (int rc = check_logits(fn, dtype, vocab, ld)) return rc;
  if (rows < 0 || n_draw <= 0 || n_draw > kMaxDraws)
    return fail(CS_ERR_INVALID, std::string(fn) + ": need rows >= 0 and 0 < n_draw <= 16");
  if (int rc = check_controls(fn, temperature, repetition_penalty, n_bias)) return rc;
  if (int rc = check_softcap(fn, softcap)) return rc;
  if (dfa)
    if (int rc = check_dfa(fn, *dfa, vocab, false, nullptr, nullptr)) return rc;
  if (rows == 0) return CS_OK;
  const bool greedy = temperature == 0.0f;
  const bool penalised = repetition_penalty != 1.0f && seen_off != nullptr;
  if (!logits || !out_ids || (!greedy && !seeds) || (n_bias > 0 && !bias_ids) ||
      (seen_off && !seen_ids))
    return fail(CS_ERR_INVALID, std::string(fn) + ": NULL pointer");
  if (!dfa && !greedy && !penalised && n_bias == 0)   // every control off: the old entry, its kernels
    return cs_vocab_sample(logits, dtype, rows, vocab, ld, temperature, softcap, seeds, n_draw,
                           out_ids, out_lp, workspace, workspace_bytes, stream);
  SampleCall c;
  if (int rc = plan_sample(c, fn, logits, dtype, rows, vocab, ld, temperature, softcap, seeds, n_draw,
                           workspace, workspace_bytes, false,
                           ": a biased or penalised row slice exceeds 2^19 tokens", stream))
    return rc;
  StepIn in{};
  in.bias_ids = bias_ids;
  in.n_bias = n_bias;
  in.bias_value = bias_value;
  in.seen_ids = penalised ? seen_ids : nullptr;
  in.seen_off = penalised ? seen_off : nullptr;
  in.penalty = penalised ? repetition_penalty : 1.0f;
  in.greedy = greedy;
  if (!dfa) return launch_plain<2>(fn, c, in, out_ids, out_lp);
  set_dfa(in, *dfa);
  return launch_plain<3>(fn, c, in, out_ids, out_lp);
}

// cs_sample_step_ex (dfa NULL) and cs_sample_step_dfa with masks
int sample_step_ex_body(const char* fn, const void* logits, int dtype, int64_t S, int64_t vocab,
                        int64_t ld, float temperature, float softcap, const uint64_t* base_seeds,
                        const int32_t* step, const int32_t* bias_ids, int32_t n_bias,
                        float bias_value, float repetition_penalty, const int32_t* seen_ids,
                        const int32_t* seen_off, const int32_t* stop_ids, int32_t n_stop,
                        const uint8_t* tok_bytes, const int32_t* tok_off, const uint8_t* stop_bytes,
                        const int32_t* stop_off, int32_t n_stop_seq, uint8_t* tail, int32_t* tail_len,
                        const DfaArgs* dfa, int32_t* dfa_state, int32_t max_tokens, int32_t pad_id,
                        int32_t* done, int32_t* out_len, int32_t* out_tokens, float* out_lp,
                        int64_t* next_tok, int32_t* n_alive, void* workspace, size_t workspace_bytes,
                        cs_stream_t stream) {
  StepIn in{step, done, bias_ids, n_bias, bias_value};
  const StepState state{stop_ids, n_stop, max_tokens, pad_id, done, out_len, out_tokens, out_lp,
                        next_tok, n_alive};
  if (int rc = check_logits(fn, dtype, vocab, ld)) return rc;
  const char* bad_counts =
      (n_stop < 0 || n_stop > 16) ? ": need 0 <= n_stop <= 16"
      : (n_stop_seq < 0 || n_stop_seq > kMaxStopSeq) ? ": need 0 <= n_stop_seq <= 8" : nullptr;
  if (int rc = check_step_state(fn, S, vocab, state, bad_counts)) return rc;
  if (int rc = check_controls(fn, temperature, repetition_penalty, n_bias)) return rc;
  if (int rc = check_softcap(fn, softcap)) return rc;
  if (dfa)
    if (int rc = check_dfa(fn, *dfa, vocab, true, tok_bytes, tok_off)) return rc;
  StopSeqs sq{};
  if (n_stop_seq > 0) {
    if (!stop_bytes || !stop_off) return fail(CS_ERR_INVALID, std::string(fn) + ": NULL pointer");
    for (int k = 0; k < n_stop_seq; ++k) {   // stop_bytes / stop_off are host memory
      const int64_t len = static_cast<int64_t>(stop_off[k + 1]) - stop_off[k];
      if (stop_off[0] != 0 || len < 1 || len > kMaxStopLen)
        return fail(CS_ERR_INVALID, std::string(fn) + ": a stop string needs 1 to 32 bytes");
    }
    sq.n_seq = n_stop_seq;
    for (int k = 0; k <= n_stop_seq; ++k) sq.off[k] = stop_off[k];
    for (int j = 0; j < stop_off[n_stop_seq]; ++j) sq.bytes[j] = stop_bytes[j];
    sq.tail = tail;
    sq.tail_len = tail_len;
  }
  if (n_stop_seq > 0 || dfa) {
    sq.tok_bytes = tok_bytes;
    sq.tok_off = tok_off;
  }
  if (S == 0) return CS_OK;
  const bool greedy = temperature == 0.0f;
  const bool penalised = repetition_penalty != 1.0f;
  if (step_ptr_missing(logits, base_seeds, greedy, in, state) || (seen_off && !seen_ids) ||
      (n_stop_seq > 0 && (!tok_bytes || !tok_off || !tail || !tail_len)))
    return fail(CS_ERR_INVALID, std::string(fn) + ": NULL pointer");
  if (!dfa && !greedy && !penalised && n_stop_seq == 0)   // every control off: the old entry, its kernels
    return cs_sample_step(logits, dtype, S, vocab, ld, temperature, softcap, base_seeds, step,
                          bias_ids, n_bias, bias_value, stop_ids, n_stop, max_tokens, pad_id, done,
                          out_len, out_tokens, out_lp, next_tok, n_alive, workspace, workspace_bytes,
                          stream);
  SampleCall c;
  if (int rc = plan_sample(c, fn, logits, dtype, S, vocab, ld, temperature, softcap, base_seeds, 1,
                           workspace, workspace_bytes, true,
                           ": a biased or penalised row slice exceeds 2^19 tokens", stream))
    return rc;
  in.seen_ids = penalised ? seen_ids : nullptr;
  in.seen_off = penalised ? seen_off : nullptr;
  in.out_tokens = out_tokens;
  in.out_len = out_len;
  in.max_tokens = max_tokens;
  in.penalty = repetition_penalty;
  in.greedy = greedy;
  if (!dfa) return launch_step<2>(fn, c, in, state, sq);
  set_dfa(in, *dfa);
  sq.trans = dfa->trans;
  sq.dfa_state = dfa_state;
  sq.n_states = dfa->n_states;
  return launch_step<3>(fn, c, in, state, sq);
}

}  // namespace

extern "C" {

size_t cs_vocab_topk_workspace_size(int64_t rows, int64_t vocab, int32_t k) {
  if (rows <= 0 || vocab <= 0 || k <= 0) return 0;
  return static_cast<size_t>(rows) * topk_nchunk(vocab) * static_cast<size_t>(k) *
         sizeof(unsigned long long);
}

int cs_vocab_topk(const void* logits, int dtype, int64_t rows, int64_t vocab, int64_t ld, int32_t k,
                  float softcap, int32_t* out_ids, float* out_vals, void* workspace,
                  size_t workspace_bytes, cs_stream_t stream) {
  const char* fn = "cs_vocab_topk";
  if (int rc = check_logits(fn, dtype, vocab, ld)) return rc;
  if (rows < 0 || k <= 0 || k > 256 || k > vocab)
    return fail(CS_ERR_INVALID, std::string(fn) + ": need rows >= 0 and 0 < k <= min(256, vocab)");
  if (int rc = check_softcap(fn, softcap)) return rc;
  if (rows == 0) return CS_OK;
  if (!logits || !out_ids) return fail(CS_ERR_INVALID, std::string(fn) + ": NULL pointer");
  const int32_t nchunk = topk_nchunk(vocab);
  const int64_t nkeys = static_cast<int64_t>(nchunk) * (k < kTopkChunk ? k : kTopkChunk);
  if (nkeys > 16384) return fail(CS_ERR_INVALID, std::string(fn) + ": vocab chunks x k exceeds 16384");
  if (int rc = check_grid(fn, rows * nchunk)) return rc;
  // (the chunk winners are 64-bit words, but this entry point has never asked for an aligned
  // workspace)
  if (int rc = check_workspace(fn, workspace, workspace_bytes,
                               cs_vocab_topk_workspace_size(rows, vocab, k), 1))
    return rc;
  auto* part = static_cast<unsigned long long*>(workspace);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int64_t ld_bytes = ld * elt_size(dtype);
  const float inv_cap = softcap > 0.0f ? 1.0f / softcap : 0.0f;
  const char* lg = static_cast<const char*>(logits);
  dispatch_dtype_cap(dtype, softcap, [&](auto dt, auto cap) {
    hipLaunchKernelGGL((vocab_topk_chunk_kernel<decltype(dt)::value, decltype(cap)::value>),
                       dim3(static_cast<uint32_t>(rows * nchunk)), dim3(256), 0, st, lg, vocab,
                       ld_bytes, nchunk, k, softcap, inv_cap, part);
  });
  const int32_t n2 = next_pow2(nkeys);
  const int32_t lds_keys = n2 > kTopkChunk ? n2 : kTopkChunk;
  // up to 16384 keys: 128 KiB of dynamic LDS
  launch_big_lds<&vocab_topk_merge_kernel>(kTopkLdsMax, dim3(static_cast<uint32_t>(rows)), dim3(256),
                                           static_cast<size_t>(lds_keys) * sizeof(unsigned long long),
                                           st, part, static_cast<int32_t>(nkeys), n2, k, out_ids,
                                           out_vals);
  return check_launch("cs_vocab_topk");
}

size_t cs_vocab_sample_workspace_size(int64_t rows, int64_t vocab, int32_t n_draw) {
  if (rows <= 0 || vocab <= 0 || n_draw <= 0) return 0;
  const SplitPlan p = plan_split(rows, vocab, CS_F32);  // elementwise loop: same split for every dtype
  return static_cast<size_t>(rows) * p.nsplit * (sizeof(float2) + n_draw * sizeof(DrawBest));
}

int cs_vocab_sample(const void* logits, int dtype, int64_t rows, int64_t vocab, int64_t ld,
                    float temperature, float softcap, const uint64_t* seeds, int32_t n_draw,
                    int32_t* out_ids, float* out_lp, void* workspace, size_t workspace_bytes,
                    cs_stream_t stream) {
  const char* fn = "cs_vocab_sample";
  if (int rc = check_logits(fn, dtype, vocab, ld)) return rc;
  if (rows < 0 || n_draw <= 0 || n_draw > kMaxDraws)
    return fail(CS_ERR_INVALID, std::string(fn) + ": need rows >= 0 and 0 < n_draw <= 16");
  if (!(temperature > 0.0f) || std::isinf(temperature))
    return fail(CS_ERR_INVALID, std::string(fn) + ": temperature must be finite and > 0");
  if (int rc = check_softcap(fn, softcap)) return rc;
  if (rows == 0) return CS_OK;
  if (!logits || !seeds || !out_ids) return fail(CS_ERR_INVALID, std::string(fn) + ": NULL pointer");
  SampleCall c;
  if (int rc = plan_sample(c, fn, logits, dtype, rows, vocab, ld, temperature, softcap, seeds, n_draw,
                           workspace, workspace_bytes, false, nullptr, stream))
    return rc;
  return launch_plain<0>(fn, c, StepIn{}, out_ids, out_lp);
}

// workspace: the arrival word, then the partials of cs_vocab_sample with one draw
size_t cs_sample_step_workspace_size(int64_t S, int64_t vocab) {
  if (S <= 0 || vocab <= 0) return 0;
  return sizeof(unsigned long long) + cs_vocab_sample_workspace_size(S, vocab, 1);
}

int cs_sample_step(const void* logits, int dtype, int64_t S, int64_t vocab, int64_t ld,
                   float temperature, float softcap, const uint64_t* base_seeds,
                   const int32_t* step, const int32_t* bias_ids, int32_t n_bias, float bias_value,
                   const int32_t* stop_ids, int32_t n_stop, int32_t max_tokens, int32_t pad_id,
                   int32_t* done, int32_t* out_len, int32_t* out_tokens, float* out_lp,
                   int64_t* next_tok, int32_t* n_alive, void* workspace, size_t workspace_bytes,
                   cs_stream_t stream) {
  const char* fn = "cs_sample_step";
  const StepIn in{step, done, bias_ids, n_bias, bias_value};
  const StepState state{stop_ids, n_stop, max_tokens, pad_id, done, out_len, out_tokens, out_lp,
                        next_tok, n_alive};
  if (int rc = check_logits(fn, dtype, vocab, ld)) return rc;
  const bool bad_counts = n_bias < 0 || n_bias > 1024 || n_stop < 0 || n_stop > 16;
  if (int rc = check_step_state(fn, S, vocab, state,
                                bad_counts ? ": need 0 <= n_bias <= 1024 and 0 <= n_stop <= 16" : nullptr))
    return rc;
  if (!(temperature > 0.0f) || std::isinf(temperature))
    return fail(CS_ERR_INVALID, std::string(fn) + ": temperature must be finite and > 0");
  if (int rc = check_softcap(fn, softcap)) return rc;
  if (S == 0) return CS_OK;
  if (step_ptr_missing(logits, base_seeds, false, in, state))
    return fail(CS_ERR_INVALID, std::string(fn) + ": NULL pointer");
  SampleCall c;
  if (int rc = plan_sample(c, fn, logits, dtype, S, vocab, ld, temperature, softcap, base_seeds, 1,
                           workspace, workspace_bytes, true,
                           n_bias > 0 ? ": a biased row slice exceeds 2^19 tokens" : nullptr, stream))
    return rc;
  return n_bias > 0 ? launch_step<1>(fn, c, in, state, NoStopSeqs{})
                    : launch_step<0>(fn, c, in, state, NoStopSeqs{});
}

size_t cs_vocab_sample_ex_workspace_size(int64_t rows, int64_t vocab, int32_t n_draw) {
  return cs_vocab_sample_workspace_size(rows, vocab, n_draw);
}

int cs_vocab_sample_ex(const void* logits, int dtype, int64_t rows, int64_t vocab, int64_t ld,
                       float temperature, float softcap, const uint64_t* seeds, int32_t n_draw,
                       const int32_t* bias_ids, int32_t n_bias, float bias_value,
                       float repetition_penalty, const int32_t* seen_ids, const int32_t* seen_off,
                       int32_t* out_ids, float* out_lp, void* workspace, size_t workspace_bytes,
                       cs_stream_t stream) {
  return vocab_sample_ex_body("cs_vocab_sample_ex", logits, dtype, rows, vocab, ld, temperature,
                              softcap, seeds, n_draw, bias_ids, n_bias, bias_value,
                              repetition_penalty, seen_ids, seen_off, nullptr, out_ids, out_lp,
                              workspace, workspace_bytes, stream);
}

size_t cs_sample_step_ex_workspace_size(int64_t S, int64_t vocab) {
  return cs_sample_step_workspace_size(S, vocab);
}

int cs_sample_step_ex(const void* logits, int dtype, int64_t S, int64_t vocab, int64_t ld,
                      float temperature, float softcap, const uint64_t* base_seeds,
                      const int32_t* step, const int32_t* bias_ids, int32_t n_bias, float bias_value,
                      float repetition_penalty, const int32_t* seen_ids, const int32_t* seen_off,
                      const int32_t* stop_ids, int32_t n_stop, const uint8_t* tok_bytes,
                      const int32_t* tok_off, const uint8_t* stop_bytes, const int32_t* stop_off,
                      int32_t n_stop_seq, uint8_t* tail, int32_t* tail_len, int32_t max_tokens,
                      int32_t pad_id, int32_t* done, int32_t* out_len, int32_t* out_tokens,
                      float* out_lp, int64_t* next_tok, int32_t* n_alive, void* workspace,
                      size_t workspace_bytes, cs_stream_t stream) {
  return sample_step_ex_body("cs_sample_step_ex", logits, dtype, S, vocab, ld, temperature, softcap,
                             base_seeds, step, bias_ids, n_bias, bias_value, repetition_penalty,
                             seen_ids, seen_off, stop_ids, n_stop, tok_bytes, tok_off, stop_bytes,
                             stop_off, n_stop_seq, tail, tail_len, nullptr, nullptr, max_tokens,
                             pad_id, done, out_len, out_tokens, out_lp, next_tok, n_alive, workspace,
                             workspace_bytes, stream);
}

int cs_dfa_token_masks(const int16_t* trans, const uint8_t* accept, int32_t n_states,
                       const uint8_t* tok_bytes, const int32_t* tok_off, int64_t vocab,
                       const int32_t* stop_ids, int32_t n_stop, uint32_t* masks,
                       cs_stream_t stream) {
  const char* fn = "cs_dfa_token_masks";
  if (n_states < 1 || n_states > kMaxDfaStates)
    return fail(CS_ERR_INVALID, std::string(fn) + ": need 1 <= n_states <= 1024");
  if (vocab <= 0 || vocab > INT32_MAX)
    return fail(CS_ERR_INVALID, std::string(fn) + ": need 0 < vocab < 2^31");
  if (n_stop < 0 || n_stop > 16)
    return fail(CS_ERR_INVALID, std::string(fn) + ": need 0 <= n_stop <= 16");
  if (!trans || !accept || !tok_bytes || !tok_off || !masks || (n_stop > 0 && !stop_ids))
    return fail(CS_ERR_INVALID, std::string(fn) + ": NULL pointer");
  const int64_t words = (vocab + 31) / 32;
  hipLaunchKernelGGL(dfa_token_masks_kernel,
                     dim3(static_cast<uint32_t>((vocab + 255) / 256), static_cast<uint32_t>(n_states)),
                     dim3(256), 0, static_cast<hipStream_t>(stream), trans, accept, n_states,
                     tok_bytes, tok_off, vocab, words, stop_ids, n_stop, masks);
  return check_launch(fn);
}

size_t cs_vocab_sample_dfa_workspace_size(int64_t rows, int64_t vocab, int32_t n_draw) {
  return cs_vocab_sample_workspace_size(rows, vocab, n_draw);
}

int cs_vocab_sample_dfa(const void* logits, int dtype, int64_t rows, int64_t vocab, int64_t ld,
                        float temperature, float softcap, const uint64_t* seeds, int32_t n_draw,
                        const int32_t* bias_ids, int32_t n_bias, float bias_value,
                        float repetition_penalty, const int32_t* seen_ids, const int32_t* seen_off,
                        const uint32_t* masks, int64_t mask_words, int32_t n_states,
                        const int32_t* dfa_state, int32_t* out_ids, float* out_lp, void* workspace,
                        size_t workspace_bytes, cs_stream_t stream) {
  if (!masks)   // no automaton: the old entry, its kernels
    return cs_vocab_sample_ex(logits, dtype, rows, vocab, ld, temperature, softcap, seeds, n_draw,
                              bias_ids, n_bias, bias_value, repetition_penalty, seen_ids, seen_off,
                              out_ids, out_lp, workspace, workspace_bytes, stream);
  const DfaArgs dfa{masks, mask_words, n_states, dfa_state, nullptr};
  return vocab_sample_ex_body("cs_vocab_sample_dfa", logits, dtype, rows, vocab, ld, temperature,
                              softcap, seeds, n_draw, bias_ids, n_bias, bias_value,
                              repetition_penalty, seen_ids, seen_off, &dfa, out_ids, out_lp,
                              workspace, workspace_bytes, stream);
}

size_t cs_sample_step_dfa_workspace_size(int64_t S, int64_t vocab) {
  return cs_sample_step_workspace_size(S, vocab);
}

int cs_sample_step_dfa(const void* logits, int dtype, int64_t S, int64_t vocab, int64_t ld,
                       float temperature, float softcap, const uint64_t* base_seeds,
                       const int32_t* step, const int32_t* bias_ids, int32_t n_bias, float bias_value,
                       float repetition_penalty, const int32_t* seen_ids, const int32_t* seen_off,
                       const int32_t* stop_ids, int32_t n_stop, const uint8_t* tok_bytes,
                       const int32_t* tok_off, const uint8_t* stop_bytes, const int32_t* stop_off,
                       int32_t n_stop_seq, uint8_t* tail, int32_t* tail_len, const uint32_t* masks,
                       int64_t mask_words, const int16_t* trans, int32_t n_states,
                       int32_t* dfa_state, int32_t max_tokens, int32_t pad_id, int32_t* done,
                       int32_t* out_len, int32_t* out_tokens, float* out_lp, int64_t* next_tok,
                       int32_t* n_alive, void* workspace, size_t workspace_bytes,
                       cs_stream_t stream) {
  if (!masks)   // no automaton: the old entry, its kernels
    return cs_sample_step_ex(logits, dtype, S, vocab, ld, temperature, softcap, base_seeds, step,
                             bias_ids, n_bias, bias_value, repetition_penalty, seen_ids, seen_off,
                             stop_ids, n_stop, tok_bytes, tok_off, stop_bytes, stop_off, n_stop_seq,
                             tail, tail_len, max_tokens, pad_id, done, out_len, out_tokens, out_lp,
                             next_tok, n_alive, workspace, workspace_bytes, stream);
  const DfaArgs dfa{masks, mask_words, n_states, dfa_state, trans};
  return sample_step_ex_body("cs_sample_step_dfa", logits, dtype, S, vocab, ld, temperature, softcap,
                             base_seeds, step, bias_ids, n_bias, bias_value, repetition_penalty,
                             seen_ids, seen_off, stop_ids, n_stop, tok_bytes, tok_off, stop_bytes,
                             stop_off, n_stop_seq, tail, tail_len, &dfa, dfa_state, max_tokens,
                             pad_id, done, out_len, out_tokens, out_lp, next_tok, n_alive, workspace,
                             workspace_bytes, stream);
}

}  // extern "C"
