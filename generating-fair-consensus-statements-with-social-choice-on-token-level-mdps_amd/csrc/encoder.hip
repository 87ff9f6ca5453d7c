// encoder.hip — the elementwise side of the bidirectional text encoder (BERT-style, post-LN:
// BAAI/bge-*-en-v1.5) and the evaluator's cosine-similarity utilities:
//
//   embed_ln_kernel        word[id] + position[offset in text] + token_type[0], LayerNorm, over
//                          a ragged batch given as cu_seqlens (no padding)
//   add_ln_kernel          LayerNorm(x + residual) * w + b (post-LN: mean AND variance, with a
//                          bias; norm.hip's add_rms_kernel is the RMSNorm of the decoders)
//   gelu_kernel            erf-GELU, 0.5 x (1 + erf(x / sqrt 2))
//   cosine_welfare_kernel  1 - scipy.spatial.distance.cosine of every (agent, statement) pair
//                          and the three welfare folds over agents, in fp64 (one launch)
//
// The LayerNorms sum and normalise in fp32 and round once, to the bf16 output: the sum
// x + residual (word + position + type) is never rounded on its own.  The reference reaches
// all of this through a hosted embedding API (src/utils.py:376-407) and folds the similarities
// in Python (src/evaluation.py:232-307).  The encoder's attention is in attn.hip.
#include "cs_kernels.cuh"

namespace {

constexpr int kEncThreads = 256;
constexpr int kEncMaxD = 8 * kEncThreads;   // one 16-byte vector per thread

// LayerNorm of the row whose 8 elements x[] this thread holds (has: v < d / 8), two passes
// over registers: mean, then the variance about it (a constant row has variance exactly 0).
__device__ __forceinline__ void layer_norm_row(float (&x)[8], bool has, int v, int64_t d, float eps,
                                               const uint16_t* __restrict__ w,
                                               const uint16_t* __restrict__ b, uint16_t* y,
                                               float (&red)[2][kEncThreads / 64]) {
  u16x8 wv, bv;
  if (has) {
    wv = *reinterpret_cast<const u16x8*>(w + 8 * v);
    bv = *reinterpret_cast<const u16x8*>(b + 8 * v);
  }
  float s = 0.0f;
  if (has) {
#pragma unroll
    for (int e = 0; e < 8; ++e) s += x[e];
  }
  const float mean = block_sum<kEncThreads>(s, red[0]) / static_cast<float>(d);
  float ss = 0.0f;
  if (has) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      x[e] -= mean;
      ss = fmaf(x[e], x[e], ss);
    }
  }
  const float rstd = 1.0f / sqrtf(block_sum<kEncThreads>(ss, red[1]) / static_cast<float>(d) + eps);
  if (has) {
    u16x8 out;
#pragma unroll
    for (int e = 0; e < 8; ++e) out[e] = bf16_bits((x[e] * rstd) * bf(wv[e]) + bf(bv[e]));
    *reinterpret_cast<u16x8*>(y + 8 * v) = out;
  }
}

// one workgroup per token.  A token outside every text, an id outside the vocabulary or a
// position past the table: the row is zeros and *status = CS_ERR_INVALID (a plain store of
// one value: no order among the writers matters)
__global__ __launch_bounds__(kEncThreads) void embed_ln_kernel(
    const int32_t* __restrict__ ids, const int32_t* __restrict__ cu, int32_t n_text,
    const uint16_t* __restrict__ word, int32_t vocab, const uint16_t* __restrict__ pos,
    int32_t n_pos, const uint16_t* __restrict__ type0, const uint16_t* __restrict__ w,
    const uint16_t* __restrict__ b, int64_t d, float eps, uint16_t* __restrict__ y, int64_t ldy,
    int32_t* status) {
  __shared__ float red[2][kEncThreads / 64];
  const int64_t tok = blockIdx.x;
  const int v = threadIdx.x;
  const bool has = v < static_cast<int>(d >> 3);
  // the text of this token: the last t with cu[t] <= tok (workgroup-uniform)
  int lo = 0, hi = n_text;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (cu[mid] <= tok) lo = mid;
    else hi = mid;
  }
  const int64_t p = tok - cu[lo];
  const int32_t id = ids[tok];
  const bool ok = p >= 0 && tok < cu[lo + 1] && p < n_pos && id >= 0 && id < vocab;
  if (!ok) {
    if (has) *reinterpret_cast<u16x8*>(y + tok * ldy + 8 * v) = u16x8{0, 0, 0, 0, 0, 0, 0, 0};
    if (threadIdx.x == 0) *status = CS_ERR_INVALID;
    return;
  }
  float x[8];
  if (has) {
    const u16x8 a = *reinterpret_cast<const u16x8*>(word + static_cast<int64_t>(id) * d + 8 * v);
    const u16x8 q = *reinterpret_cast<const u16x8*>(pos + p * d + 8 * v);
    const u16x8 t = *reinterpret_cast<const u16x8*>(type0 + 8 * v);
#pragma unroll
    for (int e = 0; e < 8; ++e) x[e] = (bf(a[e]) + bf(t[e])) + bf(q[e]);
  }
  layer_norm_row(x, has, v, d, eps, w, b, y + tok * ldy, red);
}

// one workgroup per row; y may alias x or r (every element is loaded before the first barrier
// and stored after the last by the same thread)
__global__ __launch_bounds__(kEncThreads) void add_ln_kernel(
    const uint16_t* x_, int64_t ldx, const uint16_t* r_, int64_t ldr,
    const uint16_t* __restrict__ w, const uint16_t* __restrict__ b, int64_t d, float eps,
    uint16_t* y, int64_t ldy) {
  __shared__ float red[2][kEncThreads / 64];
  const int64_t row = blockIdx.x;
  const int v = threadIdx.x;
  const bool has = v < static_cast<int>(d >> 3);
  float x[8];
  if (has) {
    const u16x8 a = *reinterpret_cast<const u16x8*>(x_ + row * ldx + 8 * v);
    if (r_) {
      const u16x8 r = *reinterpret_cast<const u16x8*>(r_ + row * ldr + 8 * v);
#pragma unroll
      for (int e = 0; e < 8; ++e) x[e] = bf(a[e]) + bf(r[e]);
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) x[e] = bf(a[e]);
    }
  }
  layer_norm_row(x, has, v, d, eps, w, b, y + row * ldy, red);
}

// grid rows * nb (nb = ceil(F / (8 * 256)) blocks per row): 8 outputs per thread
__global__ __launch_bounds__(kEncThreads) void gelu_kernel(const uint16_t* x, int64_t ldx, int64_t F,
                                                           int nb, uint16_t* y, int64_t ldy) {
  const int64_t r = blockIdx.x / nb;
  const int64_t j = (static_cast<int64_t>(blockIdx.x % nb) * kEncThreads + threadIdx.x) * 8;
  if (j >= F) return;
  const u16x8 a = *reinterpret_cast<const u16x8*>(x + r * ldx + j);
  u16x8 o;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const float t = bf(a[e]);
    o[e] = bf16_bits((0.5f * t) * (1.0f + erff(t * 0.70710678118654752f)));
  }
  *reinterpret_cast<u16x8*>(y + r * ldy + j) = o;
}

// three fp64 sums over the workgroup at once, every thread gets the totals: wave butterfly,
// then the wave sums in wave order
__device__ __forceinline__ void sum3(double (&v)[3], double (*red)[3]) {
#pragma unroll
  for (int k = 0; k < 3; ++k) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v[k] += shfl_xor_f64(v[k], o);
  }
  __syncthreads();   // the last totals are read
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < 3; ++k) red[threadIdx.x >> 6][k] = v[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    double t = 0.0;
#pragma unroll
    for (int i = 0; i < kEncThreads / 64; ++i) t += red[i][k];
    v[k] = t;
  }
}

// one workgroup per statement s: for every agent a (in order) u.v, u.u, v.v in fp64, the
// similarity by the reference's rules, and thread 0's running min / sum / sum-log over the
// finite ones (Python's left-to-right sums, src/evaluation.py:278-307)
__global__ __launch_bounds__(kEncThreads) void cosine_welfare_kernel(
    const float* __restrict__ Es, int64_t lds_, const float* __restrict__ Ea, int64_t lda,
    const uint8_t* __restrict__ valid_s, const uint8_t* __restrict__ valid_a, int32_t S, int32_t A,
    int64_t d, double eps, double* __restrict__ cos_out, double* __restrict__ welfare) {
  __shared__ double red[kEncThreads / 64][3];
  const int s = blockIdx.x;
  const float* u = Es + s * lds_;
  const bool vs = !valid_s || valid_s[s] != 0;
  const double nan = __longlong_as_double(0x7ff8000000000000LL);
  double wmin = 0.0, wsum = 0.0, wlog = 0.0;
  int n_fin = 0;
  for (int a = 0; a < A; ++a) {
    const float* v = Ea + a * lda;
    double acc[3] = {0.0, 0.0, 0.0};
    for (int64_t i = threadIdx.x; i < d; i += kEncThreads) {
      const double x = static_cast<double>(u[i]), y = static_cast<double>(v[i]);
      acc[0] = fma(x, y, acc[0]);
      acc[1] = fma(x, x, acc[1]);
      acc[2] = fma(y, y, acc[2]);
    }
    sum3(acc, red);
    if (threadIdx.x == 0) {
      const double uv = acc[0], uu = acc[1], vv = acc[2];
      double c;
      if (!vs || (valid_a && valid_a[a] == 0)) {
        c = nan;
      } else if (uu == 0.0 || vv == 0.0) {
        c = 0.0;
      } else {
        double dist = 1.0 - uv / sqrt(uu * vv);
        dist = dist < 0.0 ? 0.0 : (dist > 2.0 ? 2.0 : dist);   // NaN stays NaN
        c = 1.0 - dist;
        if (!isfinite(c)) c = nan;
      }
      cos_out[static_cast<int64_t>(a) * S + s] = c;
      if (isfinite(c)) {
        wmin = n_fin == 0 ? c : (c < wmin ? c : wmin);
        wsum += c;
        wlog += log(c > eps ? c : eps);
        ++n_fin;
      }
    }
  }
  if (threadIdx.x == 0) {
    welfare[s] = n_fin ? wmin : nan;
    welfare[static_cast<int64_t>(S) + s] = n_fin ? wsum : nan;
    welfare[2 * static_cast<int64_t>(S) + s] = n_fin ? wlog : nan;
  }
}

int check_ln_shape(const std::string& nm, int64_t rows, int64_t d) {
  if (rows < 0 || d <= 0) return fail(CS_ERR_INVALID, nm + ": bad shape");
  if (d % 8 != 0 || d > kEncMaxD) return fail(CS_ERR_INVALID, nm + ": d must be a multiple of 8 and <= 2048");
  if (rows > 0x7fffffffLL) return fail(CS_ERR_INVALID, nm + ": too many rows");
  return CS_OK;
}

}  // namespace

extern "C" {

int cs_embed_layer_norm(const int32_t* ids, const int32_t* cu_seqlens, int32_t n_text, int64_t n_tok,
                        int32_t max_seqlen, const void* word_emb, int32_t vocab, const void* pos_emb,
                        int32_t n_pos, const void* type_emb, const void* weight, const void* bias,
                        int64_t d, float eps, void* y, int64_t ldy, int32_t* status,
                        cs_stream_t stream) {
  const std::string nm = "cs_embed_layer_norm";
  if (n_text < 0) return fail(CS_ERR_INVALID, nm + ": bad shape");
  if (const int rc = check_ln_shape(nm, n_tok, d)) return rc;
  if (vocab <= 0 || n_pos <= 0) return fail(CS_ERR_INVALID, nm + ": empty vocabulary or position table");
  if (max_seqlen < 0 || max_seqlen > n_pos)
    return fail(CS_ERR_INVALID, nm + ": a text is longer than the position table");
  if (n_tok == 0) return CS_OK;
  if (n_text == 0) return fail(CS_ERR_INVALID, nm + ": tokens without a text");
  if (!ids || !cu_seqlens || !word_emb || !pos_emb || !type_emb || !weight || !bias || !y || !status)
    return fail(CS_ERR_INVALID, nm + ": NULL pointer");
  if (!(eps >= 0.0f)) return fail(CS_ERR_INVALID, nm + ": eps must be >= 0");
  if (ldy < d || ldy % 8) return fail(CS_ERR_INVALID, nm + ": ldy must be >= d and a multiple of 8");
  if (misaligned(word_emb, 16) || misaligned(pos_emb, 16) || misaligned(type_emb, 16) ||
      misaligned(weight, 16) || misaligned(bias, 16) || misaligned(y, 16))
    return fail(CS_ERR_INVALID, nm + ": tables and output must be 16-byte aligned");
  hipLaunchKernelGGL(embed_ln_kernel, dim3(static_cast<uint32_t>(n_tok)), dim3(kEncThreads), 0,
                     static_cast<hipStream_t>(stream), ids, cu_seqlens, n_text,
                     static_cast<const uint16_t*>(word_emb), vocab, static_cast<const uint16_t*>(pos_emb),
                     n_pos, static_cast<const uint16_t*>(type_emb), static_cast<const uint16_t*>(weight),
                     static_cast<const uint16_t*>(bias), d, eps, static_cast<uint16_t*>(y), ldy, status);
  return check_launch("cs_embed_layer_norm");
}

int cs_add_layer_norm(const void* x, int64_t ldx, const void* residual, int64_t ldr,
                      const void* weight, const void* bias, int64_t rows, int64_t d, float eps,
                      void* y, int64_t ldy, cs_stream_t stream) {
  const std::string nm = "cs_add_layer_norm";
  if (const int rc = check_ln_shape(nm, rows, d)) return rc;
  if (rows == 0) return CS_OK;
  if (!x || !weight || !bias || !y) return fail(CS_ERR_INVALID, nm + ": NULL pointer");
  if (!(eps >= 0.0f)) return fail(CS_ERR_INVALID, nm + ": eps must be >= 0");
  if (ldx < d || ldy < d || ldx % 8 || ldy % 8 || (residual && (ldr < d || ldr % 8)))
    return fail(CS_ERR_INVALID, nm + ": leading dimensions must be >= d and multiples of 8");
  if (misaligned(x, 16) || misaligned(residual, 16) || misaligned(weight, 16) ||
      misaligned(bias, 16) || misaligned(y, 16))
    return fail(CS_ERR_INVALID, nm + ": pointers must be 16-byte aligned");
  hipLaunchKernelGGL(add_ln_kernel, dim3(static_cast<uint32_t>(rows)), dim3(kEncThreads), 0,
                     static_cast<hipStream_t>(stream), static_cast<const uint16_t*>(x), ldx,
                     static_cast<const uint16_t*>(residual), ldr, static_cast<const uint16_t*>(weight),
                     static_cast<const uint16_t*>(bias), d, eps, static_cast<uint16_t*>(y), ldy);
  return check_launch("cs_add_layer_norm");
}

int cs_gelu(const void* x, int64_t ldx, int64_t rows, int64_t F, void* y, int64_t ldy,
            cs_stream_t stream) {
  if (rows < 0 || F <= 0) return fail(CS_ERR_INVALID, "cs_gelu: bad shape");
  if (rows == 0) return CS_OK;
  if (!x || !y) return fail(CS_ERR_INVALID, "cs_gelu: NULL pointer");
  if (F % 8 || ldx % 8 || ldy % 8 || ldx < F || ldy < F)
    return fail(CS_ERR_INVALID, "cs_gelu: F and leading dimensions must be multiples of 8, >= F");
  if (misaligned(x, 16) || misaligned(y, 16)) return fail(CS_ERR_INVALID, "cs_gelu: pointers must be 16-byte aligned");
  const int64_t nb = cdiv(F / 8, kEncThreads);
  if (rows * nb > 0x7fffffffLL) return fail(CS_ERR_INVALID, "cs_gelu: grid too large");
  hipLaunchKernelGGL(gelu_kernel, dim3(static_cast<uint32_t>(rows * nb)), dim3(kEncThreads), 0,
                     static_cast<hipStream_t>(stream), static_cast<const uint16_t*>(x), ldx, F,
                     static_cast<int>(nb), static_cast<uint16_t*>(y), ldy);
  return check_launch("cs_gelu");
}

int cs_cosine_welfare(const float* E_s, int64_t ld_s, const float* E_a, int64_t ld_a,
                      const uint8_t* valid_s, const uint8_t* valid_a, int32_t S, int32_t A, int64_t d,
                      double eps, double* out_cos, double* out_welfare, cs_stream_t stream) {
  if (S < 0 || A < 0 || d <= 0) return fail(CS_ERR_INVALID, "cs_cosine_welfare: bad shape");
  if (S == 0) return CS_OK;
  if (!E_s || (A > 0 && !E_a) || !out_welfare || (A > 0 && !out_cos))
    return fail(CS_ERR_INVALID, "cs_cosine_welfare: NULL pointer");
  if (ld_s < d || (A > 0 && ld_a < d)) return fail(CS_ERR_INVALID, "cs_cosine_welfare: leading dimension < d");
  if (!(eps > 0.0)) return fail(CS_ERR_INVALID, "cs_cosine_welfare: eps must be > 0");
  if (misaligned(E_s, 4) || misaligned(E_a, 4) || misaligned(out_cos, 8) || misaligned(out_welfare, 8))
    return fail(CS_ERR_INVALID, "cs_cosine_welfare: misaligned pointer");
  hipLaunchKernelGGL(cosine_welfare_kernel, dim3(static_cast<uint32_t>(S)), dim3(kEncThreads), 0,
                     static_cast<hipStream_t>(stream), E_s, ld_s, E_a, ld_a, valid_s, valid_a, S, A, d,
                     eps, out_cos, out_welfare);
  return check_launch("cs_cosine_welfare");
}

}  // extern "C"
