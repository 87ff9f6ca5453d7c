// gemm_w8.hip — the decode-step projection GEMM on a 1-byte copy of the weight:
// Y[M, N] = bf16(2^e[n] * sum_k X[m][k] * value(code[n][k])), X bf16, code OCP e4m3fn (bias 7,
// largest finite 448, no infinities; not MI300's fnuz), one power-of-two scale 2^e[n] per
// output row.  At the row counts of a decode step (M <= 80) a projection is a weight stream,
// so its time follows the bytes: this kernel streams half of what cs_gemm_bf16 does.
//
// The format (w8_row_exponent, w8_quantise; restated in tests/w8_ref.py):
//   e[n]       = the smallest integer with amax_n * 2^-e[n] <= 448 (an all-zero row: 0), int8
//   code[n][k] = e4m3_rne(w[n][k] * 2^-e[n])  (subnormal codes kept; NaN codes never produced)
//   twin[n][k] = value(code[n][k]) * 2^e[n]   (every finite code is exact in bf16 and the scale
//                moves only the exponent, so the twin is a bf16 number: the bf16 routes run
//                on exactly the values this kernel sees)
// A row is refused (status) when an input is not finite, when e[n] leaves int8, or when a
// twin value is not a bf16 number (it overflows, or falls below bf16's subnormal grid).
//
// The packed layout (cs_gemm_w8_pack, cs_gemm_w8_pack_codes): the 16-row tile T's 64-deep K
// step s is 1 KB at byte (T * K / 64 + s) * 1024, lane-linear: lane l's 16 bytes hold row
// 16 T + l % 16, bytes [8 h, 8 h + 8) = k 64 s + 32 h + 8 (l / 16) .. + 7 (h = 0, 1: the two
// 32-deep MFMAs of the step), so ONE 16-byte load per lane feeds a whole K step of a tile:
//   Cp[(T * K / 64 + s) * 1024 + 16 l + 8 h + j] = code[16 T + l % 16][64 s + 32 h + 8 (l / 16) + j]
//
// w8_gemm_kernel<MT, GATED>: a workgroup of 4 waves owns 128 W rows (GATED: 64 gate features
// and their 64 up features) x all M <= 16 MT rows over a K range; each wave streams two 16-row
// tiles of codes from HBM straight into registers through a six-step ring (10 KB in flight per
// wave), converts them to bf16 A-fragments in registers (v_cvt_pk_f32_fp8, then the upper
// halves of the two floats: exact, every code is a bf16 number) and runs
// v_mfma_f32_16x16x32_bf16 against X, which is staged through LDS in three buffers (as
// ws_gemm_kernel of gemm.hip stages it: 128-B rows, 16-B chunk XOR swizzle).  The fp32 sum (or
// each K split's partial) is scaled by 2^e[n] (ldexpf: exact) before anything is rounded.
// Split-K writes fp32 partials [split][M][N] folded in split order: deterministic, no atomics.
#include "cs_kernels.cuh"

#include <utility>

namespace {

typedef __bf16 wbf16x8 __attribute__((ext_vector_type(8)));
typedef float wf32x2 __attribute__((ext_vector_type(2)));
typedef float wf32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t wu32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t wu32x4 __attribute__((ext_vector_type(4)));
typedef uint16_t wu16x4 __attribute__((ext_vector_type(4)));
typedef uint16_t wu16x8 __attribute__((ext_vector_type(8)));

constexpr int kW8Threads = 256;     // 4 waves, each two 16-row tiles of W
constexpr int kW8BN = 128;          // W rows per workgroup
constexpr int kW8BK = 64;           // K per step
constexpr int kW8Ring = 6;          // register ring: K steps of W and of X loaded ahead (a multiple of 3)
constexpr int kW8MaxTiles = 5;      // 16-row tiles of X: M <= 80
constexpr int kW8MaxSplits = 16;    // (cs_add_rms_norm_splitk's limit)

enum : int { kW8NonFinite = 1, kW8RowRange = 2 };   // the status bits of cs_gemm_w8_pack

__device__ __forceinline__ float w_silu(float x) { return x / (1.0f + expf(-x)); }
__device__ __forceinline__ float w_gelu_tanh(float x) {
  const float k0 = 0.7978845608028654f, k1 = 0.044715f;
  return 0.5f * x * (1.0f + tanhf(k0 * (x + k1 * x * x * x)));
}

// byte offset of 16-B chunk c (0..7) of X-tile row r in one LDS stage
__device__ __forceinline__ int w_swz(int r, int c) { return r * 128 + ((c ^ ((r >> 1) & 7)) << 4); }

template <typename F, int... Is>
__device__ __forceinline__ void w_static_for_impl(F&& f, std::integer_sequence<int, Is...>) {
  (f(std::integral_constant<int, Is>{}), ...);
}
template <int N, typename F>
__device__ __forceinline__ void w_static_for(F&& f) {
  w_static_for_impl(f, std::make_integer_sequence<int, N>{});
}

// 8 codes (two dwords, k ascending) -> one bf16 A-fragment
__device__ __forceinline__ wbf16x8 w8_fragment(uint32_t c0, uint32_t c1) {
  const wf32x2 a = __builtin_amdgcn_cvt_pk_f32_fp8(static_cast<int>(c0), false);
  const wf32x2 b = __builtin_amdgcn_cvt_pk_f32_fp8(static_cast<int>(c0), true);
  const wf32x2 c = __builtin_amdgcn_cvt_pk_f32_fp8(static_cast<int>(c1), false);
  const wf32x2 d = __builtin_amdgcn_cvt_pk_f32_fp8(static_cast<int>(c1), true);
  const auto pair = [](wf32x2 v) {
    return (__float_as_uint(v[1]) & 0xffff0000u) | (__float_as_uint(v[0]) >> 16);
  };
  const wu32x4 r{pair(a), pair(b), pair(c), pair(d)};
  return __builtin_bit_cast(wbf16x8, r);
}

// grid: n_tiles x splits (column tile fastest).  nk = K steps per split, ns = K / 64.
template <int MT, int GATED>
__global__ __launch_bounds__(kW8Threads, 2) void w8_gemm_kernel(
    const uint16_t* __restrict__ X, int64_t ldx, const unsigned char* __restrict__ C,
    const int8_t* __restrict__ E, uint16_t* Y, int64_t ldy, float* __restrict__ P,
    int64_t M, int64_t n_out, int64_t gate_off, int nk, int64_t ns, int n_tiles, int act, int add) {
  constexpr int kRows = 16 * MT;
  constexpr int kStage = kRows * 128;
  constexpr int kChunks = kRows * 8;
  constexpr int kCPT = (kChunks + kW8Threads - 1) / kW8Threads;
  __shared__ __align__(16) unsigned char lds[3 * kStage];

  const int bid = blockIdx.x;
  const int nt = bid % n_tiles;
  const int sp = bid / n_tiles;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wv = tid >> 6;
  const int64_t step0 = static_cast<int64_t>(sp) * nk;

  // this wave's two W row tiles (first rows) and their code streams
  int64_t wrow[2];
  if (GATED) {
    wrow[0] = static_cast<int64_t>(nt) * 64 + wv * 16;
    wrow[1] = gate_off + wrow[0];
  } else {
    wrow[0] = static_cast<int64_t>(nt) * kW8BN + wv * 32;
    wrow[1] = wrow[0] + 16;
  }
  const unsigned char* cp[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) cp[j] = C + ((wrow[j] >> 4) * ns + step0) * 1024 + 16 * lane;

  // X staging as in ws_gemm_kernel: chunk q = tid + u * 256 -> tile row q >> 3, chunk q & 7;
  // chunks past the tile repeat its last one, rows past M a real row, K steps past the end
  // the last one: every load and store is unconditional
  const uint16_t* xp[kCPT];
  int xoff[kCPT];
#pragma unroll
  for (int u = 0; u < kCPT; ++u) {
    int q = tid + u * kW8Threads;
    if (q > kChunks - 1) q = kChunks - 1;
    const int r = q >> 3;
    const int c = q & 7;
    int64_t gr = r;
    if (gr > M - 1) gr = M - 1;
    xp[u] = X + gr * ldx + step0 * kW8BK + c * 8;
    xoff[u] = w_swz(r, c);
  }

  wf32x4 acc[MT][2];
#pragma unroll
  for (int i = 0; i < MT; ++i) {
    acc[i][0] = wf32x4{0.f, 0.f, 0.f, 0.f};
    acc[i][1] = wf32x4{0.f, 0.f, 0.f, 0.f};
  }

  auto load_x = [&](wu32x4 (&xs)[kCPT], int kt) {
    kt = kt < nk ? kt : nk - 1;
#pragma unroll
    for (int u = 0; u < kCPT; ++u) xs[u] = *reinterpret_cast<const wu32x4*>(xp[u] + kt * kW8BK);
  };
  auto store_x = [&](const wu32x4 (&xs)[kCPT], int buf) {
#pragma unroll
    for (int u = 0; u < kCPT; ++u) *reinterpret_cast<wu32x4*>(lds + buf * kStage + xoff[u]) = xs[u];
  };
  auto load_w = [&](wu32x4 (&w)[2], int kt) {
    kt = kt < nk ? kt : nk - 1;
    const int64_t o = static_cast<int64_t>(kt) * 1024;
    w[0] = __builtin_nontemporal_load(reinterpret_cast<const wu32x4*>(cp[0] + o));
    w[1] = __builtin_nontemporal_load(reinterpret_cast<const wu32x4*>(cp[1] + o));
  };
  const int xr = lane & 15;
  auto compute = [&](int buf, const wu32x4 (&w)[2]) {
    const unsigned char* base = lds + buf * kStage;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const wbf16x8 a0 = w8_fragment(w[0][2 * s], w[0][2 * s + 1]);
      const wbf16x8 a1 = w8_fragment(w[1][2 * s], w[1][2 * s + 1]);
#pragma unroll
      for (int i = 0; i < MT; ++i) {
        const wbf16x8 xf =
            *reinterpret_cast<const wbf16x8*>(base + w_swz(xr + 16 * i, s * 4 + (lane >> 4)));
        acc[i][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, xf, acc[i][0], 0, 0, 0);
        acc[i][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, xf, acc[i][1], 0, 0, 0);
      }
    }
  };

  // Step t computes X(t) (LDS buffer t % 3) against W(t) (ring slot t % 6) and stores X(t + 1)
  // (ring slot (t + 1) % 6) into buffer (t + 1) % 3 -- last read in step t - 2, two barriers
  // ago -- then issues X(t + 7) and W(t + 6) into the two slots it freed; one barrier per
  // step.  X rides as far ahead as W: the vmcnt counter retires loads in issue order, so the
  // wait for W(t) and X(t + 1) (both issued in step t - 6) leaves the loads of the five steps
  // after them in flight, 10 KB of codes per wave.
  wu32x4 wr[kW8Ring][2];
  wu32x4 xs[kW8Ring][kCPT];
  load_x(xs[0], 0);
  w_static_for<kW8Ring - 1>([&](auto rc) {
    constexpr int r = decltype(rc)::value;
    load_x(xs[r + 1], r + 1);
    load_w(wr[r], r);
  });
  store_x(xs[0], 0);
  load_x(xs[0], kW8Ring);
  load_w(wr[kW8Ring - 1], kW8Ring - 1);
  __syncthreads();
  int t = 0;
  for (; t + kW8Ring <= nk; t += kW8Ring) {
    w_static_for<kW8Ring>([&](auto rc) {
      constexpr int r = decltype(rc)::value;
      compute(r % 3, wr[r]);
      store_x(xs[(r + 1) % kW8Ring], (r + 1) % 3);
      load_x(xs[(r + 1) % kW8Ring], t + r + 1 + kW8Ring);
      load_w(wr[r], t + r + kW8Ring);
      __syncthreads();
    });
  }
  w_static_for<kW8Ring - 1>([&](auto rc) {      // the tail: up to 5 steps, all of them loaded
    constexpr int r = decltype(rc)::value;
    if (t + r < nk) {                            // (uniform: every thread takes the same way)
      compute(r % 3, wr[r]);
      store_x(xs[(r + 1) % kW8Ring], (r + 1) % 3);
      __syncthreads();
    }
  });

  // epilogue: D[n][m] -> the lane holds rows n = 4 * (lane >> 4) + e (e = 0..3) of column m
  int ex[2][4];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const uint32_t v = *reinterpret_cast<const uint32_t*>(E + wrow[j] + 4 * (lane >> 4));
#pragma unroll
    for (int e = 0; e < 4; ++e) ex[j][e] = static_cast<int8_t>((v >> (8 * e)) & 0xffu);
  }
#pragma unroll
  for (int i = 0; i < MT; ++i) {
    const int64_t m = 16 * i + (lane & 15);
    if (m >= M) continue;
    if (GATED) {
      wu16x4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float g = bf(bf16_bits(ldexpf(acc[i][0][e], ex[0][e])));
        const float u = bf(bf16_bits(ldexpf(acc[i][1][e], ex[1][e])));
        const uint16_t a = bf16_bits(act ? w_gelu_tanh(g) : w_silu(g));
        o[e] = bf16_bits(bf(a) * u);
      }
      *reinterpret_cast<wu16x4*>(Y + m * ldy + wrow[0] + 4 * (lane >> 4)) = o;
    } else {
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int64_t n = wrow[j] + 4 * (lane >> 4);
        wf32x4 v;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = ldexpf(acc[i][j][e], ex[j][e]);
        if (P) {
          *reinterpret_cast<wf32x4*>(P + (static_cast<int64_t>(sp) * M + m) * n_out + n) = v;
        } else {
          wu16x4 o;
          if (add) {     // Y holds the residual rows: the fp32 sum is added before the one rounding
            const wu16x4 r = *reinterpret_cast<const wu16x4*>(Y + m * ldy + n);
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = bf16_bits(v[e] + bf(r[e]));
          } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = bf16_bits(v[e]);
          }
          *reinterpret_cast<wu16x4*>(Y + m * ldy + n) = o;
        }
      }
    }
  }
}

// Y[m][n] = bf16(sum_s P[s][m][n]) in split order; 8 outputs per thread (the fold of
// cs_gemm_bf16, so cs_rope_place_splitk and cs_add_rms_norm_splitk fold these partials alike);
// add: Y[m][n] = bf16(Y[m][n] + sum_s P[s][m][n])
__global__ __launch_bounds__(256) void w8_reduce_kernel(const float* __restrict__ P, int splits,
                                                        int64_t M, int64_t N,
                                                        uint16_t* Y, int64_t ldy, int add) {
  const int64_t v = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  const int64_t nv = N / 8;
  if (v >= M * nv) return;
  const int64_t m = v / nv;
  const int64_t n = (v - m * nv) * 8;
  wf32x4 a = *reinterpret_cast<const wf32x4*>(P + m * N + n);
  wf32x4 b = *reinterpret_cast<const wf32x4*>(P + m * N + n + 4);
  for (int s = 1; s < splits; ++s) {
    const float* q = P + (static_cast<int64_t>(s) * M + m) * N + n;
    a += *reinterpret_cast<const wf32x4*>(q);
    b += *reinterpret_cast<const wf32x4*>(q + 4);
  }
  wu16x8 o;
  if (add) {     // Y holds the residual rows (cs_gemm_bf16_w8_add): added in fp32, one rounding
    const wu16x8 r = *reinterpret_cast<const wu16x8*>(Y + m * ldy + n);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      o[e] = bf16_bits(a[e] + bf(r[e]));
      o[4 + e] = bf16_bits(b[e] + bf(r[4 + e]));
    }
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      o[e] = bf16_bits(a[e]);
      o[4 + e] = bf16_bits(b[e]);
    }
  }
  *reinterpret_cast<wu16x8*>(Y + m * ldy + n) = o;
}

// ---- the quantiser ----

// the smallest e with |v| * 2^-e <= 448 for the bf16 magnitude bits mag (finite, non-zero):
// |v| = f * 2^x with f in [0.5, 1) and 448 = 0.875 * 2^9, so e = x - 9 when f <= 0.875, else x - 8
__device__ __forceinline__ int w8_row_exponent(uint32_t mag) {
  if (mag == 0) return 0;
  const int ef = static_cast<int>(mag >> 7);
  const uint32_t m = mag & 0x7fu;
  if (ef > 0) return (ef - 126) - (m <= 96 ? 9 : 8);            // f = (128 + m) / 256
  const int p = 31 - __clz(m);                                   // subnormal: m * 2^-133
  return (p - 132) - (m * 8 <= (7u << (p + 1)) ? 9 : 8);         // f = m / 2^(p + 1)
}

// e4m3_rne(q) for |q| <= 448: the code byte
__device__ __forceinline__ uint32_t w8_encode(float q) {
  const uint32_t u = __float_as_uint(q);
  const uint32_t sign = (u >> 24) & 0x80u;
  const float a = fabsf(q);
  uint32_t c;
  if (a < 0.015625f) {                       // below 2^-6: the subnormal grid, spacing 2^-9
    c = static_cast<uint32_t>(rintf(a * 512.0f));          // 8 = the smallest normal code
  } else {
    const uint32_t v = u & 0x7fffffffu;
    c = ((v + 0x7ffffu + ((v >> 20) & 1u)) >> 20) - (120u << 3);
  }
  return sign | c;
}

__device__ __forceinline__ float w8_value(uint32_t code) {
  const int m = code & 7, ef = (code >> 3) & 15;
  const float v = ldexpf(static_cast<float>(ef ? 8 + m : m), (ef ? ef : 1) - 10);
  return code & 0x80u ? -v : v;
}

// the largest magnitude bits of the row over the workgroup; `bad` if one is Inf or NaN
__device__ __forceinline__ uint32_t w8_row_amax(const uint16_t* w, int64_t K, bool* bad) {
  __shared__ uint32_t red[256 / 64];
  uint32_t mx = 0;
  for (int64_t c = threadIdx.x; c < K / 8; c += 256) {
    const wu16x8 v = *reinterpret_cast<const wu16x8*>(w + 8 * c);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const uint32_t mag = v[j] & 0x7fffu;
      mx = mag > mx ? mag : mx;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t other = __shfl_xor(mx, o);
    mx = other > mx ? other : mx;
  }
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mx;
  __syncthreads();
  mx = red[0];
#pragma unroll
  for (int i = 1; i < 256 / 64; ++i) mx = red[i] > mx ? red[i] : mx;
  *bad = mx >= 0x7f80u;
  return mx;
}

// code and twin bits of one element under the row exponent e; false when the twin is no bf16 number
__device__ __forceinline__ bool w8_quantise(uint16_t wbits, int e, uint32_t* code, uint16_t* twin) {
  const uint32_t c = w8_encode(ldexpf(bf(wbits), -e));
  const float val = w8_value(c);
  const float t = ldexpf(val, e);
  const uint16_t tb = bf16_bits(t);
  *code = c;
  *twin = tb;
  return (tb & 0x7fffu) < 0x7f80u && ldexpf(bf(tb), -e) == val;
}

// one workgroup per row: sets the status bits of a row cs_gemm_w8_pack refuses
__global__ __launch_bounds__(256) void w8_check_kernel(const uint16_t* __restrict__ W, int64_t ldw,
                                                       int64_t K, int* __restrict__ status) {
  const uint16_t* w = W + static_cast<int64_t>(blockIdx.x) * ldw;
  bool bad;
  const uint32_t mx = w8_row_amax(w, K, &bad);
  int flags = 0;
  if (bad) {
    flags = kW8NonFinite;
  } else {
    const int e = w8_row_exponent(mx);
    if (e < -128 || e > 127) {
      flags = kW8RowRange;
    } else {
      for (int64_t c = threadIdx.x; c < K / 8; c += 256) {
        const wu16x8 v = *reinterpret_cast<const wu16x8*>(w + 8 * c);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          uint32_t code;
          uint16_t tb;
          if (!w8_quantise(v[j], e, &code, &tb)) flags = kW8RowRange;
        }
      }
    }
  }
  if (flags) atomicOr(status, flags);
}

// one workgroup per row, after w8_check_kernel on the same stream: nothing is written once a
// row was refused.  twin may be W itself (each thread rewrites the elements it read, after the
// row's amax is known).
__global__ __launch_bounds__(256) void w8_write_kernel(const uint16_t* W, int64_t ldw,
                                                       int64_t K, const int* __restrict__ status,
                                                       unsigned char* __restrict__ Cp,
                                                       int8_t* __restrict__ E, uint16_t* twin,
                                                       int64_t ldt) {
  if (*status) return;
  const int64_t row = blockIdx.x;
  const uint16_t* w = W + row * ldw;
  bool bad;
  const int e = w8_row_exponent(w8_row_amax(w, K, &bad));
  if (threadIdx.x == 0) E[row] = static_cast<int8_t>(e);
  const int64_t ns = K / kW8BK;
  for (int64_t c = threadIdx.x; c < K / 8; c += 256) {
    const wu16x8 v = *reinterpret_cast<const wu16x8*>(w + 8 * c);
    wu16x8 tw;
    uint32_t lo = 0, hi = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      uint32_t code;
      uint16_t tb;
      w8_quantise(v[j], e, &code, &tb);
      tw[j] = tb;
      if (j < 4) lo |= code << (8 * j); else hi |= code << (8 * (j - 4));
    }
    const int64_t s = c >> 3;                  // K step; chunk c & 7 = 4 h + l / 16
    const int h = static_cast<int>(c & 7) >> 2, g = static_cast<int>(c & 3);
    const int l = 16 * g + static_cast<int>(row & 15);
    *reinterpret_cast<wu32x2*>(Cp + ((row >> 4) * ns + s) * 1024 + 16 * l + 8 * h) = wu32x2{lo, hi};
    if (twin) *reinterpret_cast<wu16x8*>(twin + row * ldt + 8 * c) = tw;
  }
}

// the permutation alone: codes [N, K] row-major -> Cp; one 8-byte piece per thread
__global__ __launch_bounds__(256) void w8_pack_codes_kernel(const unsigned char* __restrict__ Cin,
                                                            int64_t n_pieces, int64_t K,
                                                            unsigned char* __restrict__ Cp) {
  const int64_t v = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (v >= n_pieces) return;
  const int64_t per_row = K / 8, ns = K / kW8BK;
  const int64_t row = v / per_row, c = v - row * per_row;
  const int64_t s = c >> 3;
  const int h = static_cast<int>(c & 7) >> 2, g = static_cast<int>(c & 3);
  const int l = 16 * g + static_cast<int>(row & 15);
  *reinterpret_cast<wu32x2*>(Cp + ((row >> 4) * ns + s) * 1024 + 16 * l + 8 * h) =
      *reinterpret_cast<const wu32x2*>(Cin + row * K + 8 * c);
}

// ---- the host half ----

constexpr int64_t w8_splits(int64_t N, int64_t K, bool gated) {
  if (gated) return 1;
  const int64_t tiles = N / kW8BN;
  int64_t s = 1;
  // fill the 256 CUs while keeping >= 8 K steps per split
  while (tiles * s < 256 && s * 2 <= kW8MaxSplits && K % (kW8BK * s * 2) == 0 &&
         K / (kW8BK * s * 2) >= 8)
    s *= 2;
  return s;
}

template <int GATED, int... MTs>
bool w8_launch(int mt, std::integer_sequence<int, MTs...>, dim3 grid, hipStream_t st,
               const uint16_t* x, int64_t ldx, const unsigned char* c, const int8_t* e, uint16_t* y,
               int64_t ldy, float* p, int64_t M, int64_t n_out, int64_t gate_off, int nk, int64_t ns,
               int n_tiles, int act, int add) {
  const auto run = [&](auto tiles) {
    hipLaunchKernelGGL((w8_gemm_kernel<decltype(tiles)::value, GATED>), grid, dim3(kW8Threads), 0, st,
                       x, ldx, c, e, y, ldy, p, M, n_out, gate_off, nk, ns, n_tiles, act, add);
    return true;
  };
  return ((mt == MTs + 1 && run(std::integral_constant<int, MTs + 1>{})) || ...);
}

// cs_gemm_bf16_w8 (add = false) and cs_gemm_bf16_w8_add (y holds the residual rows); fn is the
// entry point's name
int w8_impl(const char* fn, const void* x, int64_t ldx, const void* codes_packed, const int8_t* row_exp,
            void* y, int64_t ldy, int64_t M, int64_t N, int64_t K, int splits, int gated, int act,
            float* workspace, cs_stream_t stream, bool add) {
  const auto bad = [fn](const char* why) { return fail(CS_ERR_INVALID, std::string(fn) + ": " + why); };
  if (M < 0 || N <= 0 || K <= 0) return bad("bad shape");
  if (N % kW8BN) return bad("N must be a multiple of 128");
  if (K % kW8BK) return bad("K must be a multiple of 64");
  if (M > 16 * kW8MaxTiles) return bad("M exceeds cs_gemm_w8_max_rows()");
  if (gated && splits > 1) return bad("the gated form takes no K split");
  if (M == 0) return CS_OK;
  int64_t s = splits <= 0 ? w8_splits(N, K, gated != 0) : splits;
  if (s > kW8MaxSplits) return bad("at most 16 splits");
  if (K % (kW8BK * s)) return bad("K must be a multiple of 64 * splits");
  const int64_t n_out = gated ? N / 2 : N;
  if (!x || !codes_packed || !row_exp) return bad("NULL pointer");
  if (!y && s <= 1) return bad("y may be NULL only with a K split (partials kept)");
  if (ldx % 8 || ldx < K || (y && (ldy % 4 || ldy < n_out)))
    return bad("leading dimensions too small or misaligned");
  if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(codes_packed)) & 15 ||
      reinterpret_cast<uintptr_t>(row_exp) & 3 || reinterpret_cast<uintptr_t>(y) & 7)
    return bad("x and the codes must be 16-byte aligned (y 8-byte, row_exp 4-byte)");
  if (s > 1 && (!workspace || reinterpret_cast<uintptr_t>(workspace) & 15))
    return bad("split K needs a 16-byte aligned workspace of splits * M * N floats");
  if (s > 1 && y && (ldy % 8 || reinterpret_cast<uintptr_t>(y) & 15))
    return bad("a K split needs y 16-byte aligned and ldy % 8 == 0");
  const int64_t n_tiles = N / kW8BN;
  if (n_tiles * s > 0x7fffffffLL) return bad("grid too large");
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int mt = static_cast<int>((M + 15) / 16);
  const dim3 grid(static_cast<uint32_t>(n_tiles * s));
  float* part = s > 1 ? workspace : nullptr;
  const auto launch = [&](auto g) {
    return w8_launch<decltype(g)::value>(
        mt, std::make_integer_sequence<int, kW8MaxTiles>{}, grid, st, static_cast<const uint16_t*>(x),
        ldx, static_cast<const unsigned char*>(codes_packed), row_exp, static_cast<uint16_t*>(y), ldy,
        part, M, n_out, gated ? N / 2 : 0, static_cast<int>(K / (kW8BK * s)), K / kW8BK,
        static_cast<int>(n_tiles), gated ? act : 0, add ? 1 : 0);
  };
  const bool ok = gated ? launch(std::integral_constant<int, 1>{}) : launch(std::integral_constant<int, 0>{});
  if (!ok) return bad("no kernel is compiled for this row count");
  if (s > 1 && y) {   // y == NULL: the caller folds the partials itself
    const int64_t nv = M * (N / 8);
    hipLaunchKernelGGL(w8_reduce_kernel, dim3(static_cast<uint32_t>((nv + 255) / 256)), dim3(256), 0, st,
                       workspace, static_cast<int>(s), M, N, static_cast<uint16_t*>(y), ldy, add ? 1 : 0);
  }
  return check_launch(fn);
}

}  // namespace

extern "C" {

int64_t cs_gemm_w8_max_rows(void) { return 16 * kW8MaxTiles; }

int64_t cs_gemm_w8_splits(int64_t M, int64_t N, int64_t K, int gated) {
  if (M <= 0 || N <= 0 || K <= 0 || N % kW8BN || K % kW8BK) return 0;
  return w8_splits(N, K, gated != 0);
}

int cs_gemm_bf16_w8(const void* x, int64_t ldx, const void* codes_packed, const int8_t* row_exp,
                    void* y, int64_t ldy, int64_t M, int64_t N, int64_t K, int splits, int gated,
                    int act, float* workspace, cs_stream_t stream) {
  return w8_impl("cs_gemm_bf16_w8", x, ldx, codes_packed, row_exp, y, ldy, M, N, K, splits, gated, act,
                 workspace, stream, false);
}

int cs_gemm_bf16_w8_add(const void* x, int64_t ldx, const void* codes_packed, const int8_t* row_exp,
                        void* h, int64_t ldh, int64_t M, int64_t N, int64_t K, int splits,
                        float* workspace, cs_stream_t stream) {
  if (!h && M > 0) return fail(CS_ERR_INVALID, "cs_gemm_bf16_w8_add: NULL pointer");
  return w8_impl("cs_gemm_bf16_w8_add", x, ldx, codes_packed, row_exp, h, ldh, M, N, K, splits, 0, 0,
                 workspace, stream, true);
}

int cs_gemm_w8_pack(const void* w, int64_t ldw, int64_t N, int64_t K, void* codes_packed,
                    int8_t* row_exp, void* twin, int64_t ldt, int32_t* status, cs_stream_t stream) {
  const auto bad = [](const char* why) { return fail(CS_ERR_INVALID, std::string("cs_gemm_w8_pack: ") + why); };
  if (!w || !codes_packed || !row_exp || !status) return bad("NULL pointer");
  if (N <= 0 || K <= 0 || N % 16 || K % kW8BK || ldw < K || ldw % 8 || N > 0x7fffffffLL)
    return bad("need N % 16 == 0, K % 64 == 0, ldw >= K, ldw % 8 == 0");
  if (twin && (ldt < K || ldt % 8)) return bad("need ldt >= K, ldt % 8 == 0");
  if ((reinterpret_cast<uintptr_t>(w) | reinterpret_cast<uintptr_t>(codes_packed) |
       reinterpret_cast<uintptr_t>(twin)) & 15 || reinterpret_cast<uintptr_t>(status) & 3)
    return bad("operands must be 16-byte aligned (status 4-byte)");
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (hipMemsetAsync(status, 0, sizeof(int32_t), st) != hipSuccess) return check_launch("cs_gemm_w8_pack");
  const dim3 grid(static_cast<uint32_t>(N));
  hipLaunchKernelGGL(w8_check_kernel, grid, dim3(256), 0, st, static_cast<const uint16_t*>(w), ldw, K,
                     status);
  hipLaunchKernelGGL(w8_write_kernel, grid, dim3(256), 0, st, static_cast<const uint16_t*>(w), ldw, K,
                     status, static_cast<unsigned char*>(codes_packed), row_exp,
                     static_cast<uint16_t*>(twin), ldt);
  return check_launch("cs_gemm_w8_pack");
}

int cs_gemm_w8_pack_codes(const void* codes, int64_t N, int64_t K, void* codes_packed,
                          cs_stream_t stream) {
  const auto bad = [](const char* why) { return fail(CS_ERR_INVALID, std::string("cs_gemm_w8_pack_codes: ") + why); };
  if (!codes || !codes_packed) return bad("NULL pointer");
  if (N <= 0 || K <= 0 || N % 16 || K % kW8BK) return bad("need N % 16 == 0, K % 64 == 0");
  if ((reinterpret_cast<uintptr_t>(codes) | reinterpret_cast<uintptr_t>(codes_packed)) & 15)
    return bad("operands must be 16-byte aligned");
  const int64_t n_pieces = N * K / 8;
  if ((n_pieces + 255) / 256 > 0x7fffffffLL) return bad("grid too large");
  hipLaunchKernelGGL(w8_pack_codes_kernel, dim3(static_cast<uint32_t>((n_pieces + 255) / 256)), dim3(256),
                     0, static_cast<hipStream_t>(stream), static_cast<const unsigned char*>(codes), n_pieces,
                     K, static_cast<unsigned char*>(codes_packed));
  return check_launch("cs_gemm_w8_pack_codes");
}

}  // extern "C"
