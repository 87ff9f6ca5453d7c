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

// What cs_sample_step adds to the streaming stage (SampleMode > kSamplePlain): the row's one
// seed is derived on the device from (base seed, *step), a finished stream's workgroups leave
// before they touch its row, and (kSampleStepBias) the listed tokens take bias_value in fp32
// before the soft-cap, looked up in an LDS bitmap over the workgroup's slice of the vocabulary.
// What the *_ex entries add (kSamplePlainEx, kSampleStepEx): a second bitmap beside the bias
// one marks the row's seen tokens, which take the repetition penalty after the soft-cap, and
// with `greedy` the score is the transformed logit itself (no seed read, no Gumbel noise).
enum SampleMode {
  kSamplePlain = 0, kSampleStep = 1, kSampleStepBias = 2, kSamplePlainEx = 3, kSampleStepEx = 4
};
constexpr bool mode_is_step(int m) { return m == kSampleStep || m == kSampleStepBias || m == kSampleStepEx; }
constexpr bool mode_is_ex(int m) { return m == kSamplePlainEx || m == kSampleStepEx; }
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

// token i's transformed logit, as the streaming stage of the *_ex modes computes it
template <int DT, bool CAP>
__device__ __forceinline__ float ex_logit(const char* rp, int32_t i, bool biased, bool seen,
                                          const StepIn& in, float cap, float inv_cap) {
  float x = load_any<DT>(rp, i);
  if (biased) x += in.bias_value;
  if (CAP) x = softcap_fn(x, cap, inv_cap);
  if (seen) x = penalise(x, in.penalty);
  return x;
}

template <int DT, bool CAP, int MODE>
__global__ __launch_bounds__(256) void vocab_sample_kernel(
    const char* __restrict__ logits, int64_t vocab, int64_t ld_bytes, int32_t nsplit,
    int64_t split_len, float inv_temp, float cap, float inv_cap,
    const unsigned long long* __restrict__ seeds, int32_t n_draw, float2* __restrict__ lse_part,
    DrawBest* __restrict__ draw_part, StepIn in) {
  // kSampleStepBias: one bit per token of [v0, v1); the *_ex modes: the seen bitmap after it
  extern __shared__ uint32_t sm_bias[];
  __shared__ float sm_m[4], sm_s[4];
  __shared__ float sm_bs[4][kMaxDraws];
  __shared__ int32_t sm_bi[4][kMaxDraws];
  const int tid = threadIdx.x;
  const int64_t bid = blockIdx.x;
  const int64_t row = bid / nsplit;
  if (mode_is_step(MODE) && in.done[row] != 0) return;   // block-uniform, before any barrier
  const int32_t split = static_cast<int32_t>(bid - row * nsplit);
  const char* rp = logits + row * ld_bytes;
  const int64_t v0 = static_cast<int64_t>(split) * split_len;
  const int64_t v1 = min(vocab, v0 + split_len);
  const int nw = static_cast<int>((v1 - v0 + 31) >> 5);
  uint32_t* sm_seen = sm_bias + nw;
  if (MODE == kSampleStepBias || mode_is_ex(MODE)) {
    for (int w = tid; w < (mode_is_ex(MODE) ? 2 * nw : nw); w += 256) sm_bias[w] = 0u;
    __syncthreads();
    for (int j = tid; j < in.n_bias; j += 256) {
      const int64_t id = in.bias_ids[j];
      if (id >= v0 && id < v1) atomicOr(&sm_bias[(id - v0) >> 5], 1u << ((id - v0) & 31));
    }
    if (mode_is_ex(MODE) && in.penalty != 1.0f) {
      if (in.seen_off) {
        const int64_t b = in.seen_off[row + 1];
        for (int64_t j = in.seen_off[row] + tid; j < b; j += 256) {
          const int64_t id = in.seen_ids[j];
          if (id >= v0 && id < v1) atomicOr(&sm_seen[(id - v0) >> 5], 1u << ((id - v0) & 31));
        }
      }
      if (MODE == kSampleStepEx) {
        const int32_t len = seen_out_len(in.out_len[row], in.max_tokens);
        for (int j = tid; j < len; j += 256) {
          const int64_t id = in.out_tokens[row * in.max_tokens + j];
          if (id >= v0 && id < v1) atomicOr(&sm_seen[(id - v0) >> 5], 1u << ((id - v0) & 31));
        }
      }
    }
    __syncthreads();
  }
  const bool greedy = mode_is_ex(MODE) && in.greedy != 0;
  unsigned long long sd[kMaxDraws];
  float bs[kMaxDraws];
  int32_t bi[kMaxDraws];
#pragma unroll
  for (int d = 0; d < kMaxDraws; ++d) {
    sd[d] = (d < n_draw && !greedy) ? seeds[row * n_draw + d] : 0ull;
    bs[d] = -INFINITY;
    bi[d] = 0x7fffffff;
  }
  if (mode_is_step(MODE) && !greedy)   // n_draw = 1
    sd[0] = sd[0] * kSeedMul + static_cast<unsigned long long>(static_cast<int64_t>(*in.step));
  float m = -INFINITY, s = 0.0f;
  bool saw_nan = false;
  for (int64_t v = v0 + tid; v < v1; v += 256) {
    float x = load_any<DT>(rp, v);
    const int64_t o = v - v0;
    if (MODE == kSampleStepBias || mode_is_ex(MODE)) {
      if ((sm_bias[o >> 5] >> (o & 31)) & 1u) x += in.bias_value;
    }
    if (CAP) x = softcap_fn(x, cap, inv_cap);
    if (mode_is_ex(MODE)) {
      if ((sm_seen[o >> 5] >> (o & 31)) & 1u) x = penalise(x, in.penalty);
    }
    const float y = x * inv_temp;
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
  // lse_accum drops a NaN that arrives while (m, s) is still empty (fmaxf(-inf, NaN) is
  // -inf), but a NaN token must poison the row's lse wherever it sits: (0, NaN) survives
  // every merge, also with empty partners
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

// EX (cs_vocab_sample_ex): the drawn token's log-probability is taken on its transformed
// logit, so the wave looks every draw's id up in the bias and seen lists.
template <int DT, bool CAP, bool EX = false>
__global__ __launch_bounds__(64) void vocab_sample_merge_kernel(
    const char* __restrict__ logits, int64_t ld_bytes, int32_t nsplit, float inv_temp, float cap,
    float inv_cap, const float2* __restrict__ lse_part, const DrawBest* __restrict__ draw_part,
    int32_t n_draw, int32_t* __restrict__ out_ids, float* __restrict__ out_lp, StepIn in) {
  const int64_t row = blockIdx.x;
  const int lane = threadIdx.x;
  float m = -INFINITY, s = 0.0f;
  for (int j = lane; j < nsplit; j += 64) {
    const float2 p = lse_part[row * nsplit + j];
    lse_merge(m, s, p.x, p.y);
  }
  wave_lse_reduce(m, s);
  const float lse = m + logf(s);
  if (EX) {
    float b = -INFINITY;
    int32_t i = 0x7fffffff;
    if (lane < n_draw) {   // n_draw <= 16: lane d merges draw d, in split order as below
      for (int j = 0; j < nsplit; ++j) {
        const DrawBest p = draw_part[(row * nsplit + j) * n_draw + lane];
        draw_merge(b, i, p.s, p.idx);
      }
    }
    for (int d = 0; d < n_draw; ++d) {
      const int32_t id = __shfl(i, d, 64);
      const bool none = id == 0x7fffffff;
      const bool biased = wave_listed(in.bias_ids, in.n_bias, id, lane);
      const bool seen = wave_seen(in, row, id, lane, nullptr, 0);
      if (lane == d) {
        out_ids[row * n_draw + d] = none ? -1 : id;
        if (out_lp) {
          float lp = __builtin_nanf("");
          if (!none)
            lp = ex_logit<DT, CAP>(logits + row * ld_bytes, id, biased, seen, in, cap, inv_cap) *
                     inv_temp - lse;
          out_lp[row * n_draw + d] = lp;
        }
      }
    }
    return;
  }
  for (int d = lane; d < n_draw; d += 64) {
    float b = -INFINITY;
    int32_t i = 0x7fffffff;
    for (int j = 0; j < nsplit; ++j) {  // split order: ties keep the lower token id
      const DrawBest p = draw_part[(row * nsplit + j) * n_draw + d];
      draw_merge(b, i, p.s, p.idx);
    }
    // no split offered a candidate (every logit -inf or NaN): id -1 and NaN, nothing read
    const bool none = i == 0x7fffffff;
    out_ids[row * n_draw + d] = none ? -1 : i;
    if (out_lp) {
      float lp = __builtin_nanf("");
      if (!none) {
        float x = load_any<DT>(logits + row * ld_bytes, i);
        if (CAP) x = softcap_fn(x, cap, inv_cap);
        lp = x * inv_temp - lse;
      }
      out_lp[row * n_draw + d] = lp;
    }
  }
}

// The stop strings of cs_sample_step_ex, passed by value: the bytes of string k are
// bytes[off[k] : off[k+1]], at most kMaxStopSeq strings of at most kMaxStopLen bytes.
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
};
struct NoStopSeqs {};

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

// cs_sample_step's second stage, one wave per stream: the split merge of
// vocab_sample_merge_kernel (same order, so the id and the log-prob are its bits), then the
// stream's state update and the next step's input token.  Lane 0 of every workgroup adds
// (1 << 32 | still alive) to the workspace's one counter word; the last arrival has the
// number of unfinished streams in the low half, writes it and leaves the word at zero.
// EX (cs_sample_step_ex): the log-probability is taken on the transformed logit (bias,
// soft-cap, penalty over the seen list and the tokens generated so far), and an appended
// token runs the stop-string window.
template <int DT, bool CAP, bool EX = false>
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
    float m = -INFINITY, s = 0.0f;
    for (int j = lane; j < nsplit; j += 64) {
      const float2 p = lse_part[row * nsplit + j];
      lse_merge(m, s, p.x, p.y);
    }
    wave_lse_reduce(m, s);
    const float lse = m + logf(s);
    float b = -INFINITY;
    int32_t i = 0x7fffffff;
    for (int j = 0; j < nsplit; ++j) {  // split order: ties keep the lower token id
      const DrawBest p = draw_part[row * nsplit + j];
      draw_merge(b, i, p.s, p.idx);
    }
    bool hit = false;
    for (int j = lane; j < in.n_bias; j += 64) hit |= in.bias_ids[j] == i;
    const bool biased = __ballot(hit) != 0ull;
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
        if (out_lp) {
          if constexpr (EX) {
            out_lp[at] = ex_logit<DT, CAP>(logits + row * ld_bytes, i, biased, seen, in, cap,
                                           inv_cap) * inv_temp - lse;
          } else {
            float x = load_any<DT>(logits + row * ld_bytes, i);
            if (biased) x += in.bias_value;
            if (CAP) x = softcap_fn(x, cap, inv_cap);
            out_lp[at] = x * inv_temp - lse;
          }
        }
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

// The two bitmaps of an *_ex slice, and their launch: beside the kernel's static arrays they
// pass the default 64 KiB of LDS from about 2^18 tokens per slice, so the limit is raised
// (once per kernel) before the default is met.
size_t ex_lds_bytes(int64_t split_len) {
  return 2 * static_cast<size_t>((split_len + 31) / 32) * sizeof(uint32_t);
}
// The attribute is set once per PROCESS and instantiation (a function-local static): right for
// this project, which runs one process per GPU.  A process that launched on a second device
// would have to raise the limit there as well; a refusal shows only as the launch's own error.
template <auto Kernel, typename... Args>
void launch_tables(dim3 grid, size_t lds, hipStream_t st, Args... args) {
  if (lds > 60 * 1024) {
    static const hipError_t raised =
        hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel),
                            hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(kExLdsLimit));
    (void)raised;  // a refusal shows as the launch's own error
  }
  hipLaunchKernelGGL(Kernel, grid, dim3(256), lds, st, args...);
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
  hipLaunchKernelGGL(vocab_topk_merge_kernel, dim3(static_cast<uint32_t>(rows)), dim3(256),
                     static_cast<size_t>(lds_keys) * sizeof(unsigned long long), st, part,
                     static_cast<int32_t>(nkeys), n2, k, out_ids, out_vals);
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
  const SplitPlan plan = plan_split(rows, vocab, CS_F32);
  if (int rc = check_grid(fn, rows * plan.nsplit)) return rc;
  if (int rc = check_workspace(fn, workspace, workspace_bytes,
                               cs_vocab_sample_workspace_size(rows, vocab, n_draw)))
    return rc;
  auto* lse_part = static_cast<float2*>(workspace);
  auto* draw_part = reinterpret_cast<DrawBest*>(lse_part + rows * plan.nsplit);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int64_t ld_bytes = ld * elt_size(dtype);
  const float inv_cap = softcap > 0.0f ? 1.0f / softcap : 0.0f;
  const float inv_t = 1.0f / temperature;
  const char* lg = static_cast<const char*>(logits);
  const auto* sd = reinterpret_cast<const unsigned long long*>(seeds);
  dispatch_dtype_cap(dtype, softcap, [&](auto dt, auto cap) {
    constexpr int DT = decltype(dt)::value;
    constexpr bool CAP = decltype(cap)::value;
    hipLaunchKernelGGL((vocab_sample_kernel<DT, CAP, kSamplePlain>),
                       dim3(static_cast<uint32_t>(rows * plan.nsplit)), dim3(256), 0, st, lg, vocab,
                       ld_bytes, plan.nsplit, plan.split_len, inv_t, softcap, inv_cap, sd, n_draw,
                       lse_part, draw_part, StepIn{});
    hipLaunchKernelGGL((vocab_sample_merge_kernel<DT, CAP>), dim3(static_cast<uint32_t>(rows)), dim3(64),
                       0, st, lg, ld_bytes, plan.nsplit, inv_t, softcap, inv_cap, lse_part, draw_part,
                       n_draw, out_ids, out_lp, StepIn{});
  });
  return check_launch("cs_vocab_sample");
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
  if (int rc = check_logits(fn, dtype, vocab, ld)) return rc;
  if (S < 0) return fail(CS_ERR_INVALID, std::string(fn) + ": need S >= 0");
  if (n_bias < 0 || n_bias > 1024 || n_stop < 0 || n_stop > 16)
    return fail(CS_ERR_INVALID, std::string(fn) + ": need 0 <= n_bias <= 1024 and 0 <= n_stop <= 16");
  if (max_tokens < 1) return fail(CS_ERR_INVALID, std::string(fn) + ": need max_tokens >= 1");
  if (pad_id < 0 || pad_id >= vocab)
    return fail(CS_ERR_INVALID, std::string(fn) + ": pad_id outside [0, vocab)");
  if (!(temperature > 0.0f) || std::isinf(temperature))
    return fail(CS_ERR_INVALID, std::string(fn) + ": temperature must be finite and > 0");
  if (int rc = check_softcap(fn, softcap)) return rc;
  if (S == 0) return CS_OK;
  if (!logits || !base_seeds || !step || !done || !out_len || !out_tokens || !next_tok || !n_alive ||
      (n_bias > 0 && !bias_ids) || (n_stop > 0 && !stop_ids))
    return fail(CS_ERR_INVALID, std::string(fn) + ": NULL pointer");
  const SplitPlan plan = plan_split(S, vocab, CS_F32);   // cs_vocab_sample's, for its bits
  if (int rc = check_grid(fn, S * plan.nsplit)) return rc;
  if (n_bias > 0 && plan.split_len > kMaxBiasSlice)
    return fail(CS_ERR_INVALID, std::string(fn) + ": a biased row slice exceeds 2^19 tokens");
  if (int rc = check_workspace(fn, workspace, workspace_bytes, cs_sample_step_workspace_size(S, vocab)))
    return rc;
  auto* arrivals = static_cast<unsigned long long*>(workspace);
  auto* lse_part = reinterpret_cast<float2*>(arrivals + 1);
  auto* draw_part = reinterpret_cast<DrawBest*>(lse_part + S * plan.nsplit);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int64_t ld_bytes = ld * elt_size(dtype);
  const float inv_cap = softcap > 0.0f ? 1.0f / softcap : 0.0f;
  const float inv_t = 1.0f / temperature;
  const char* lg = static_cast<const char*>(logits);
  const auto* sd = reinterpret_cast<const unsigned long long*>(base_seeds);
  const StepIn in{step, done, bias_ids, n_bias, bias_value};
  const dim3 grid(static_cast<uint32_t>(S * plan.nsplit));
  const size_t bitmap = static_cast<size_t>((plan.split_len + 31) / 32) * sizeof(uint32_t);
  dispatch_dtype_cap(dtype, softcap, [&](auto dt, auto cap) {
    constexpr int DT = decltype(dt)::value;
    constexpr bool CAP = decltype(cap)::value;
    if (n_bias > 0)
      hipLaunchKernelGGL((vocab_sample_kernel<DT, CAP, kSampleStepBias>), grid, dim3(256), bitmap, st,
                         lg, vocab, ld_bytes, plan.nsplit, plan.split_len, inv_t, softcap, inv_cap,
                         sd, 1, lse_part, draw_part, in);
    else
      hipLaunchKernelGGL((vocab_sample_kernel<DT, CAP, kSampleStep>), grid, dim3(256), 0, st, lg,
                         vocab, ld_bytes, plan.nsplit, plan.split_len, inv_t, softcap, inv_cap, sd,
                         1, lse_part, draw_part, in);
    hipLaunchKernelGGL((sample_step_merge_kernel<DT, CAP>), dim3(static_cast<uint32_t>(S)), dim3(64),
                       0, st, lg, ld_bytes, plan.nsplit, inv_t, softcap, inv_cap, lse_part, draw_part,
                       in, stop_ids, n_stop, max_tokens, pad_id, done, out_len, out_tokens, out_lp,
                       reinterpret_cast<long long*>(next_tok), n_alive, arrivals, NoStopSeqs{});
  });
  return check_launch("cs_sample_step");
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
  const char* fn = "cs_vocab_sample_ex";
  if (int rc = check_logits(fn, dtype, vocab, ld)) return rc;
  if (rows < 0 || n_draw <= 0 || n_draw > kMaxDraws)
    return fail(CS_ERR_INVALID, std::string(fn) + ": need rows >= 0 and 0 < n_draw <= 16");
  if (int rc = check_controls(fn, temperature, repetition_penalty, n_bias)) return rc;
  if (int rc = check_softcap(fn, softcap)) return rc;
  if (rows == 0) return CS_OK;
  const bool greedy = temperature == 0.0f;
  const bool penalised = repetition_penalty != 1.0f && seen_off != nullptr;
  if (!logits || !out_ids || (!greedy && !seeds) || (n_bias > 0 && !bias_ids) ||
      (seen_off && !seen_ids))
    return fail(CS_ERR_INVALID, std::string(fn) + ": NULL pointer");
  if (!greedy && !penalised && n_bias == 0)   // every control off: the old entry, its kernels
    return cs_vocab_sample(logits, dtype, rows, vocab, ld, temperature, softcap, seeds, n_draw,
                           out_ids, out_lp, workspace, workspace_bytes, stream);
  const SplitPlan plan = plan_split(rows, vocab, CS_F32);
  if (int rc = check_grid(fn, rows * plan.nsplit)) return rc;
  if (plan.split_len > kMaxBiasSlice)
    return fail(CS_ERR_INVALID, std::string(fn) + ": a biased or penalised row slice exceeds 2^19 tokens");
  if (int rc = check_workspace(fn, workspace, workspace_bytes,
                               cs_vocab_sample_workspace_size(rows, vocab, n_draw)))
    return rc;
  auto* lse_part = static_cast<float2*>(workspace);
  auto* draw_part = reinterpret_cast<DrawBest*>(lse_part + rows * plan.nsplit);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int64_t ld_bytes = ld * elt_size(dtype);
  const float inv_cap = softcap > 0.0f ? 1.0f / softcap : 0.0f;
  const float inv_t = greedy ? 1.0f : 1.0f / temperature;
  const char* lg = static_cast<const char*>(logits);
  const auto* sd = reinterpret_cast<const unsigned long long*>(seeds);
  StepIn in{};
  in.bias_ids = bias_ids;
  in.n_bias = n_bias;
  in.bias_value = bias_value;
  in.seen_ids = penalised ? seen_ids : nullptr;
  in.seen_off = penalised ? seen_off : nullptr;
  in.penalty = penalised ? repetition_penalty : 1.0f;
  in.greedy = greedy;
  const dim3 grid(static_cast<uint32_t>(rows * plan.nsplit));
  dispatch_dtype_cap(dtype, softcap, [&](auto dt, auto cap) {
    constexpr int DT = decltype(dt)::value;
    constexpr bool CAP = decltype(cap)::value;
    launch_tables<&vocab_sample_kernel<DT, CAP, kSamplePlainEx>>(
        grid, ex_lds_bytes(plan.split_len), st, lg, vocab, ld_bytes, plan.nsplit, plan.split_len, inv_t, softcap, inv_cap,
        sd, n_draw, lse_part, draw_part, in);
    hipLaunchKernelGGL((vocab_sample_merge_kernel<DT, CAP, true>), dim3(static_cast<uint32_t>(rows)),
                       dim3(64), 0, st, lg, ld_bytes, plan.nsplit, inv_t, softcap, inv_cap, lse_part,
                       draw_part, n_draw, out_ids, out_lp, in);
  });
  return check_launch(fn);
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
  const char* fn = "cs_sample_step_ex";
  if (int rc = check_logits(fn, dtype, vocab, ld)) return rc;
  if (S < 0) return fail(CS_ERR_INVALID, std::string(fn) + ": need S >= 0");
  if (n_stop < 0 || n_stop > 16)
    return fail(CS_ERR_INVALID, std::string(fn) + ": need 0 <= n_stop <= 16");
  if (n_stop_seq < 0 || n_stop_seq > kMaxStopSeq)
    return fail(CS_ERR_INVALID, std::string(fn) + ": need 0 <= n_stop_seq <= 8");
  if (max_tokens < 1) return fail(CS_ERR_INVALID, std::string(fn) + ": need max_tokens >= 1");
  if (pad_id < 0 || pad_id >= vocab)
    return fail(CS_ERR_INVALID, std::string(fn) + ": pad_id outside [0, vocab)");
  if (int rc = check_controls(fn, temperature, repetition_penalty, n_bias)) return rc;
  if (int rc = check_softcap(fn, softcap)) return rc;
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
    sq.tok_bytes = tok_bytes;
    sq.tok_off = tok_off;
    sq.tail = tail;
    sq.tail_len = tail_len;
  }
  if (S == 0) return CS_OK;
  const bool greedy = temperature == 0.0f;
  const bool penalised = repetition_penalty != 1.0f;
  if (!logits || (!greedy && !base_seeds) || !step || !done || !out_len || !out_tokens || !next_tok ||
      !n_alive || (n_bias > 0 && !bias_ids) || (n_stop > 0 && !stop_ids) || (seen_off && !seen_ids) ||
      (n_stop_seq > 0 && (!tok_bytes || !tok_off || !tail || !tail_len)))
    return fail(CS_ERR_INVALID, std::string(fn) + ": NULL pointer");
  if (!greedy && !penalised && n_stop_seq == 0)   // every control off: the old entry, its kernels
    return cs_sample_step(logits, dtype, S, vocab, ld, temperature, softcap, base_seeds, step,
                          bias_ids, n_bias, bias_value, stop_ids, n_stop, max_tokens, pad_id, done,
                          out_len, out_tokens, out_lp, next_tok, n_alive, workspace, workspace_bytes,
                          stream);
  const SplitPlan plan = plan_split(S, vocab, CS_F32);   // cs_vocab_sample's, for its bits
  if (int rc = check_grid(fn, S * plan.nsplit)) return rc;
  if (plan.split_len > kMaxBiasSlice)
    return fail(CS_ERR_INVALID, std::string(fn) + ": a biased or penalised row slice exceeds 2^19 tokens");
  if (int rc = check_workspace(fn, workspace, workspace_bytes, cs_sample_step_workspace_size(S, vocab)))
    return rc;
  auto* arrivals = static_cast<unsigned long long*>(workspace);
  auto* lse_part = reinterpret_cast<float2*>(arrivals + 1);
  auto* draw_part = reinterpret_cast<DrawBest*>(lse_part + S * plan.nsplit);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int64_t ld_bytes = ld * elt_size(dtype);
  const float inv_cap = softcap > 0.0f ? 1.0f / softcap : 0.0f;
  const float inv_t = greedy ? 1.0f : 1.0f / temperature;
  const char* lg = static_cast<const char*>(logits);
  const auto* sd = reinterpret_cast<const unsigned long long*>(base_seeds);
  StepIn in{step, done, bias_ids, n_bias, bias_value};
  in.seen_ids = penalised ? seen_ids : nullptr;
  in.seen_off = penalised ? seen_off : nullptr;
  in.out_tokens = out_tokens;
  in.out_len = out_len;
  in.max_tokens = max_tokens;
  in.penalty = repetition_penalty;
  in.greedy = greedy;
  const dim3 grid(static_cast<uint32_t>(S * plan.nsplit));
  dispatch_dtype_cap(dtype, softcap, [&](auto dt, auto cap) {
    constexpr int DT = decltype(dt)::value;
    constexpr bool CAP = decltype(cap)::value;
    launch_tables<&vocab_sample_kernel<DT, CAP, kSampleStepEx>>(
        grid, ex_lds_bytes(plan.split_len), st, lg, vocab, ld_bytes, plan.nsplit, plan.split_len, inv_t, softcap, inv_cap,
        sd, 1, lse_part, draw_part, in);
    hipLaunchKernelGGL((sample_step_merge_kernel<DT, CAP, true>), dim3(static_cast<uint32_t>(S)),
                       dim3(64), 0, st, lg, ld_bytes, plan.nsplit, inv_t, softcap, inv_cap, lse_part,
                       draw_part, in, stop_ids, n_stop, max_tokens, pad_id, done, out_len, out_tokens,
                       out_lp, reinterpret_cast<long long*>(next_tok), n_alive, arrivals, sq);
  });
  return check_launch(fn);
}

}  // extern "C"
