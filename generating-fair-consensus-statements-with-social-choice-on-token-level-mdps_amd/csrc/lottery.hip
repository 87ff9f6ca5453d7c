// lottery.hip — the Nash-welfare lottery over complete statements and the token policy it
// induces (the reference's core.py:116-168 and 297-328), the maximin lottery / coalition
// improvement LPs (core.py:171-279), whole solves in one launch, and the rollout of a token
// policy with numpy's own PCG64 draws (core.py:313-332).
#include "cs_kernels.cuh"

namespace {

// ---------------------------------------------------------------------------
// cs_nash_lottery: Frank-Wolfe with a golden-section line search, one workgroup per problem
// ---------------------------------------------------------------------------
// Per iteration (core.py:125-166), fp64 throughout:
//   1. every thread takes the columns j = tid, tid + BLOCK, ...: g_j = sum_i U[i,j] / a_i over
//      the agents in index order, and keeps its best (g, j), the lowest j on ties;
//   2. the block's best (wave butterfly, then the waves' bests through LDS) is j*: the pair
//      order (g desc, j asc) is total, so the result does not depend on how it is reduced;
//   3. wave 0, one lane per agent, runs the line search on F(gamma) = sum_i log((1 - gamma) a_i
//      + gamma U[i,j*]): each evaluation is one log per lane and a butterfly sum whose value
//      lane 0 broadcasts, so the bracket updates are wave-uniform; it then carries
//      a <- (1 - gamma*) a + gamma* U[:,j*] and F_new = sum_i log a_i;
//   4. every thread rescales its own columns of p (held in out_p, nobody else touches them).
// The STAGED variant keeps the problem's U in LDS ([A][m], the global layout with ld = m) and
// differs from the global one only in where a U value is loaded from: the arithmetic and its
// order are the same, so the outputs are bitwise equal.  No atomics, no host sync.
// After the last iteration a = U p is recomputed from the returned p (one wave per agent row, a
// fixed lane-strided order), so a, F and gap = max_j g_j - A are the certificate of exactly the
// p written.
constexpr int kLotMaxA = 64;
constexpr int kLotMaxM = 16384;
constexpr int kLotMaxRounds = 80;             // core.py:142
constexpr double kLotBracket = 1e-9;          // core.py:155
constexpr double kGolden = 0x1.3c6ef372fe95p-1;  // (sqrt(5) - 1) / 2 in fp64, core.py:137
// LDS the staged variant may take for U: the CU's 160 KiB less the kernel's own few hundred
// bytes, rounded down to leave room
constexpr size_t kLotLdsBytes = 144 * 1024;
constexpr int kLotWideM = 4096;               // above this many columns: 1024-thread workgroups

// wave_sum_f64 over `width` lanes, broadcast from lane 0: the same bits in every lane
__device__ __forceinline__ double wave_sum_bcast(double v, int width) {
  return __shfl(wave_sum_f64(v, width), 0, 64);
}

// (g, j) ordered by g descending, then j ascending: np.argmax's first maximum
__device__ __forceinline__ bool lot_better(double g, int32_t j, double g0, int32_t j0) {
  return g > g0 || (g == g0 && j < j0);
}

struct LotSmem {
  double a[kLotMaxA];
  double wg[16];       // one best per wave
  int32_t wj[16];
  double gamma, f_new;
  int32_t jstar;
};

// a_i = sum_j U[i,j] p_j for every agent into S.a: wave w takes the rows w, w + nwaves, ...;
// lane l adds the columns l, l + 64, ... in order, then a butterfly over the 64 lanes
template <int BLOCK, bool STAGED>
__device__ __forceinline__ void lot_row_dots(LotSmem& S, const double* __restrict__ Ug,
                                             const double* smU, int32_t A, int32_t m, int64_t ldu,
                                             const double* p) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int32_t i = wave; i < A; i += BLOCK / 64) {
    double acc = 0.0;
    for (int32_t j = lane; j < m; j += 64) {
      const double u = STAGED ? smU[static_cast<int64_t>(i) * m + j] : Ug[i * ldu + j];
      acc += u * p[j];
    }
    acc = wave_sum_f64(acc);
    if (lane == 0) S.a[i] = acc;
  }
}

// The block's argmax_j of g_j = sum_i U[i,j] / a_i (lowest j on ties), returned to every thread
template <int BLOCK, bool STAGED>
__device__ __forceinline__ ArgBest lot_gradient_argmax(LotSmem& S, const double* __restrict__ Ug,
                                                       const double* smU, int32_t A, int32_t m,
                                                       int64_t ldu) {
  double bg = -INFINITY;
  int32_t bj = 0x7fffffff;
  for (int32_t j = threadIdx.x; j < m; j += BLOCK) {
    double g = 0.0;
    for (int32_t i = 0; i < A; ++i) {
      const double u = STAGED ? smU[static_cast<int64_t>(i) * m + j] : Ug[i * ldu + j];
      g += u / S.a[i];
    }
    if (lot_better(g, j, bg, bj)) {
      bg = g;
      bj = j;
    }
  }
  const ArgBest best = block_argbest<BLOCK, lot_better>(bg, bj, S.wg, S.wj);
  return ArgBest{best.v, best.j < m ? best.j : 0};   // no column won (every g NaN): column 0
}

template <int BLOCK, bool STAGED>
__global__ __launch_bounds__(BLOCK) void nash_lottery_kernel(
    const double* __restrict__ U, int32_t A, int32_t m, int64_t ldu, int64_t ldp,
    int32_t max_iters, double tol, double* out_p, double* __restrict__ out_a,
    double* __restrict__ out_F, double* __restrict__ out_gap, int32_t* __restrict__ out_iters) {
  extern __shared__ __attribute__((aligned(16))) double smU[];
  __shared__ LotSmem S;
  const int tid = threadIdx.x, lane = tid & 63;
  const int64_t prob = blockIdx.x;
  const double* Ug = U + prob * ldp;
  double* p = out_p + prob * m;

  // the problem's entries: checked, staged, and p = 1/m
  int bad = 0;
  const double p0 = 1.0 / static_cast<double>(m);
  for (int32_t j = tid; j < m; j += BLOCK) {
    for (int32_t i = 0; i < A; ++i) {
      const double u = Ug[i * ldu + j];
      if (!(u >= 0.0) || u == INFINITY) bad = 1;
      if (STAGED) smU[static_cast<int64_t>(i) * m + j] = u;
    }
    p[j] = p0;
  }
  bad = __syncthreads_or(bad);
  lot_row_dots<BLOCK, STAGED>(S, Ug, smU, A, m, ldu, p);
  __syncthreads();
  // an agent without any utility (or a row sum that overflowed) has no log-welfare
  if (tid < A && !(S.a[tid] > 0.0 && S.a[tid] < INFINITY)) bad = 1;
  bad = __syncthreads_or(bad);
  if (bad) {  // block-uniform
    const double nan = __builtin_nan("");
    for (int32_t j = tid; j < m; j += BLOCK) p[j] = nan;
    if (out_a && tid < A) out_a[prob * A + tid] = nan;
    if (tid == 0) {
      if (out_F) out_F[prob] = nan;
      if (out_gap) out_gap[prob] = nan;
      if (out_iters) out_iters[prob] = -1;
    }
    return;
  }

  int width = 1;  // butterfly width of the per-agent sums
  while (width < A) width <<= 1;
  // F_prev = F(p): sum_i log a_i (every wave computes it, all get the same bits)
  double f_prev = wave_sum_bcast(lane < A ? log(S.a[lane]) : 0.0, width);
  int32_t iters = 0;
  for (int32_t it = 0; it < max_iters; ++it) {
    const int32_t jstar = lot_gradient_argmax<BLOCK, STAGED>(S, Ug, smU, A, m, ldu).j;
    if (tid < 64) {
      const bool on = lane < A;
      const double a = on ? S.a[lane] : 1.0;
      const double b = on ? (STAGED ? smU[static_cast<int64_t>(lane) * m + jstar]
                                    : Ug[lane * ldu + jstar])
                          : 1.0;
      auto f_gamma = [&](double gamma) {
        const double x = (1.0 - gamma) * a + gamma * b;
        return wave_sum_bcast(on ? log(x) : 0.0, width);
      };
      double lo = 0.0, hi = 1.0;
      double c = hi - kGolden * (hi - lo);
      double d = lo + kGolden * (hi - lo);
      double fc = f_gamma(c);
      double fd = f_gamma(d);
      for (int r = 0; r < kLotMaxRounds; ++r) {
        if (fc < fd) {
          lo = c;
          c = d;
          fc = fd;
          d = lo + kGolden * (hi - lo);
          fd = f_gamma(d);
        } else {
          hi = d;
          d = c;
          fd = fc;
          c = hi - kGolden * (hi - lo);
          fc = f_gamma(c);
        }
        if (hi - lo < kLotBracket) break;
      }
      const double gamma = 0.5 * (lo + hi);
      const double a_new = (1.0 - gamma) * a + gamma * b;
      const double f_new = wave_sum_bcast(on ? log(a_new) : 0.0, width);
      if (on) S.a[lane] = a_new;
      if (lane == 0) {
        S.gamma = gamma;
        S.f_new = f_new;
      }
    }
    __syncthreads();
    const double gamma = S.gamma;
    const double f_new = S.f_new;
    for (int32_t j = tid; j < m; j += BLOCK) {
      double pj = (1.0 - gamma) * p[j];
      if (j == jstar) pj += gamma;
      p[j] = pj;
    }
    iters = it + 1;
    if (f_new - f_prev < tol) break;  // block-uniform; the new p is adopted first (core.py:162-164)
    f_prev = f_new;
  }

  // the certificate of the p written: a = U p, F = sum log a, gap = max_j g_j - A
  __syncthreads();
  lot_row_dots<BLOCK, STAGED>(S, Ug, smU, A, m, ldu, p);
  __syncthreads();
  if (out_a && tid < A) out_a[prob * A + tid] = S.a[tid];
  if (out_F) {
    const double f = wave_sum_bcast(lane < A ? log(S.a[lane]) : 0.0, width);
    if (tid == 0) out_F[prob] = f;
  }
  if (out_gap) {
    const double g_best = lot_gradient_argmax<BLOCK, STAGED>(S, Ug, smU, A, m, ldu).v;
    if (tid == 0) out_gap[prob] = g_best - static_cast<double>(A);
  }
  if (out_iters && tid == 0) out_iters[prob] = iters;
}

// ---------------------------------------------------------------------------
// cs_lottery_policy: prefix masses bottom-up, then pi(b | s) = mass(s + b) / mass(s)
// ---------------------------------------------------------------------------
// The output's level-t block (B^t entries, t = 1..L) is indexed by the length-t prefix s + b, so
// it first holds that prefix's mass: level L is p itself, level t the sum of its B children in
// level t + 1, in action order (one thread per parent).  The levels are then divided by their
// parents' masses from the deepest up, each level reading the still undivided level above it;
// level 1 divides by the root mass.  A parent of mass <= 0 gives its B actions 1/B
// (core.py:316-320).  Every value is written by one thread in a fixed order: deterministic.
constexpr int kPolicyBlock = 256;
constexpr int kPolicyMaxL = 64;   // binds only at B = 1: B >= 2 has L <= 14 at the leaf limit

__global__ __launch_bounds__(kPolicyBlock) void lottery_policy_kernel(
    const double* __restrict__ p, int32_t B, int32_t L, int32_t m, int32_t total,
    double* __restrict__ out) {
  __shared__ int32_t off[kPolicyMaxL + 2];   // off[t]: start of level t (t = 1..L), off[L+1] = total
  __shared__ double root;
  const int tid = threadIdx.x;
  const double* pp = p + static_cast<int64_t>(blockIdx.x) * m;
  double* o = out + static_cast<int64_t>(blockIdx.x) * total;
  if (tid == 0) {
    int32_t at = 0, n = 1;
    for (int32_t t = 1; t <= L; ++t) {
      n *= B;
      off[t] = at;
      at += n;
    }
    off[L + 1] = at;
  }
  __syncthreads();
  for (int32_t j = tid; j < m; j += kPolicyBlock) o[off[L] + j] = pp[j];
  for (int32_t t = L - 1; t >= 0; --t) {
    __syncthreads();
    const int32_t n = t == 0 ? 1 : off[t + 1] - off[t];   // prefixes of length t
    const double* child = o + off[t + 1];
    for (int32_t s = tid; s < n; s += kPolicyBlock) {
      double acc = 0.0;
      for (int32_t b = 0; b < B; ++b) acc += child[static_cast<int64_t>(s) * B + b];
      if (t == 0) root = acc;
      else o[off[t] + s] = acc;
    }
  }
  const double uniform = 1.0 / static_cast<double>(B);
  for (int32_t t = L; t >= 1; --t) {
    __syncthreads();
    const int32_t n = off[t + 1] - off[t];
    for (int32_t i = tid; i < n; i += kPolicyBlock) {
      const double pm = t == 1 ? root : o[off[t - 1] + i / B];
      o[off[t] + i] = pm > 0.0 ? o[off[t] + i] / pm : uniform;
    }
  }
}

// ---------------------------------------------------------------------------
// cs_maximin_lottery: a revised dual simplex, one workgroup per (problem, coalition)
// ---------------------------------------------------------------------------
// The game value(M) = max_q min_{i in S} (M q)_i, M[l][j] = U[S_l][j] / base[S_l], is solved as
// min 1.x s.t. M x >= 1, x >= 0 (x = q / value).  With slacks, -M x + s = -1 and the cost row
// (1..1, 0..0) is dual-feasible from the all-slack basis, so there is no phase I.  The state is
// the r x r basis inverse Binv (r = |S|), the basic values xB, the dual weights w (the slack
// columns' reduced costs) and which column is basic in which row; the pivot row and the reduced
// costs of the m lottery columns are formed from M on the fly, so nothing grows with m but M.
// A pivot:
//   1. leaving row k: the most negative xB, lowest row on ties (every thread scans the r values
//      and gets the same k); none negative: optimal;
//   2. every thread takes the nonbasic columns j = tid, tid + BLOCK, ... of the m lottery
//      columns and then the r slacks: a_j = -sum_l Binv[k][l] M[l][j], d_j = max(1 - sum_l w[l]
//      M[l][j], 0) (slack l: Binv[k][l] and w[l]), rows in index order, and keeps its best ratio
//      d_j / -a_j over a_j < 0; the block's best (lowest j on ties: a total order, so the result
//      does not depend on how it is reduced) is the entering column e;
//   3. thread i < r forms t[i] = (Binv A_e)[i], and with it the new pivot row Binv[k][i] / t[k],
//      the step xB[k] / t[k] and d_e (each recomputed per thread: the same bits);
//   4. Binv (entries over the threads), xB and w are eliminated; thread 0 moves the basis.
// The STAGED variant keeps M in LDS ([r][m]); the other divides U by base at every read: the
// same operations in the same order, so the outputs are bitwise equal.  A one-column problem has
// one lottery and is answered without a pivot.  No atomics, no host sync.
constexpr int kMmxBasicWords = (kLotMaxM + kLotMaxA + 31) / 32;
constexpr int kMmxNarrowM = 128;              // up to this many columns: one wave per workgroup

struct MmxSmem {
  double xB[kLotMaxA], w[kLotMaxA], t[kLotMaxA], row[kLotMaxA], bs[kLotMaxA];
  double wg[16];                  // one best ratio per wave
  int32_t wj[16];
  unsigned long long wpos[16];    // per wave: the rows of M that hold a positive entry
  int32_t basis[kLotMaxA], agent[kLotMaxA];
  uint32_t basic[kMmxBasicWords];
  double sx, sw;
};

// (ratio, j) ordered by ratio ascending, then j ascending
__device__ __forceinline__ bool mmx_better(double g, int32_t j, double g0, int32_t j0) {
  return g < g0 || (g == g0 && j < j0);
}

// M[l][j] of the coalition in S: read from LDS when STAGED, else U divided by base at the read
template <bool STAGED>
struct MmxM {
  const MmxSmem& S;
  const double *smM, *Ug;
  int64_t ldu;
  int32_t m;
  __device__ __forceinline__ double operator()(int32_t l, int32_t j) const {
    return STAGED ? smM[static_cast<int64_t>(l) * m + j] : Ug[S.agent[l] * ldu + j] / S.bs[l];
  }
};

__device__ __forceinline__ bool mmx_is_basic(const MmxSmem& S, int32_t j) {
  return (S.basic[j >> 5] >> (j & 31)) & 1u;
}

// Setup: the coalition's agents and bases into S, the problem's entries checked (all A rows),
// the coalition's rows of M checked and staged into smM.  Returns (block-uniform) whether the
// problem has no answer: an empty coalition, a bad base or entry, a member's row of M all zero.
template <int BLOCK, bool STAGED>
__device__ __forceinline__ int mmx_setup(MmxSmem& S, const double* Ug, int32_t A, int32_t m,
                                         int64_t ldu, const double* base, unsigned long long mask,
                                         int32_t r, double* smM) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int bad = r == 0;
  if (tid < 64 && ((mask >> tid) & 1ull)) {
    const int32_t l = __popcll(mask & ((1ull << tid) - 1ull));
    const double b = base ? base[tid] : 1.0;
    S.agent[l] = tid;
    S.bs[l] = b;
    if (!(b > 0.0 && b < INFINITY)) bad = 1;
  }
  __syncthreads();
  unsigned long long pos = 0;
  for (int32_t j = tid; j < m; j += BLOCK) {
    for (int32_t i = 0; i < A; ++i) {
      const double u = Ug[i * ldu + j];
      if (!(u >= 0.0) || u == INFINITY) bad = 1;
    }
    for (int32_t l = 0; l < r; ++l) {
      const double v = Ug[S.agent[l] * ldu + j] / S.bs[l];
      if (v > 0.0) pos |= 1ull << l;
      if (v == INFINITY) bad = 1;          // U / base overflowed
      if (STAGED) smM[static_cast<int64_t>(l) * m + j] = v;
    }
  }
  for (int k = 1; k < 64; k <<= 1) pos |= __shfl_xor(pos, k, 64);
  if (lane == 0) S.wpos[wave] = pos;
  bad = __syncthreads_or(bad);
  for (int w = 0; w < BLOCK / 64; ++w) pos |= S.wpos[w];
  const unsigned long long rows = r == 64 ? ~0ull : (1ull << r) - 1ull;
  if (pos != rows) bad = 1;                // a member whose row of M is all zero
  return bad;
}

// Step 1: the most negative xB and its row (the lowest row on ties) as (v, j)
__device__ __forceinline__ ArgBest mmx_leaving_row(const MmxSmem& S, int32_t r) {
  int32_t k = 0;
  double xk = S.xB[0];
  for (int32_t i = 1; i < r; ++i) {
    const double x = S.xB[i];
    if (x < xk) {
      xk = x;
      k = i;
    }
  }
  return ArgBest{xk, k};
}

// Step 2: the entering column, the block's best ratio d_j / -a_j over the nonbasic columns with
// a_j < 0 against the pivot row rho = Binv[k]; >= m + r when no column can enter
template <int BLOCK, bool STAGED>
__device__ __forceinline__ int32_t mmx_ratio_test(MmxSmem& S, const MmxM<STAGED>& M,
                                                  const double* rho, int32_t r, int32_t m) {
  double bg = INFINITY;
  int32_t bj = 0x7fffffff;
  for (int32_t j = threadIdx.x; j < m + r; j += BLOCK) {
    if (mmx_is_basic(S, j)) continue;
    double a, d;
    if (j < m) {
      double acc_a = 0.0, acc_d = 0.0;
      for (int32_t l = 0; l < r; ++l) {
        const double v = M(l, j);
        acc_a += rho[l] * v;
        acc_d += S.w[l] * v;
      }
      a = -acc_a;
      d = fmax(1.0 - acc_d, 0.0);
    } else {
      a = rho[j - m];
      d = S.w[j - m];
    }
    if (a < 0.0) {
      const double g = d / -a;
      if (mmx_better(g, j, bg, bj)) {
        bg = g;
        bj = j;
      }
    }
  }
  return block_argbest<BLOCK, mmx_better>(bg, bj, S.wg, S.wj).j;
}

// Steps 3 and 4: thread i < r forms t[i], the new pivot row and the step for the entering column
// e, then Binv, xB and w are eliminated and thread 0 moves the basis
template <int BLOCK, bool STAGED>
__device__ __forceinline__ void mmx_pivot(MmxSmem& S, const MmxM<STAGED>& M, double* Binv,
                                          int32_t ldb, int32_t k, double xk, int32_t e, int32_t r,
                                          int32_t m) {
  const int tid = threadIdx.x;
  const double* rho = Binv + k * ldb;
  double theta = 0.0, de = 0.0;
  if (tid < r) {
    double ti, piv;
    if (e < m) {
      double acc_t = 0.0, acc_p = 0.0, acc_d = 0.0;
      for (int32_t l = 0; l < r; ++l) {
        const double v = M(l, e);
        acc_t += Binv[tid * ldb + l] * -v;
        acc_p += rho[l] * -v;
        acc_d += S.w[l] * v;
      }
      ti = acc_t;
      piv = acc_p;
      de = fmax(1.0 - acc_d, 0.0);
    } else {
      ti = Binv[tid * ldb + (e - m)];
      piv = rho[e - m];
      de = S.w[e - m];
    }
    theta = xk / piv;
    S.t[tid] = ti;
    S.row[tid] = rho[tid] / piv;
  }
  __syncthreads();
  for (int32_t idx = tid; idx < r * r; idx += BLOCK) {
    const int32_t i = idx / r, l = idx - i * r;
    Binv[i * ldb + l] = i == k ? S.row[l] : Binv[i * ldb + l] - S.t[i] * S.row[l];
  }
  if (tid < r) {
    S.xB[tid] = tid == k ? theta : S.xB[tid] - S.t[tid] * theta;
    S.w[tid] = fmax(S.w[tid] - de * S.row[tid], 0.0);
  }
  if (tid == 0) {
    const int32_t out = S.basis[k];
    S.basic[out >> 5] &= ~(1u << (out & 31));
    S.basic[e >> 5] |= 1u << (e & 31);
    S.basis[k] = e;
  }
}

// A one-column problem: q = (1), value = min_l M[l][0], the weight on the lowest such row
template <bool STAGED>
__device__ __forceinline__ void mmx_write_one_column(const MmxSmem& S, const MmxM<STAGED>& M,
                                                     int32_t A, int32_t r, int64_t slot,
                                                     double* out_alpha, double* out_q,
                                                     double* out_lambda, int32_t* out_pivots) {
  if (threadIdx.x != 0) return;
  int32_t kmin = 0;
  double vmin = M(0, 0);
  for (int32_t l = 1; l < r; ++l) {
    const double v = M(l, 0);
    if (v < vmin) {
      vmin = v;
      kmin = l;
    }
  }
  out_alpha[slot] = (static_cast<double>(r) / static_cast<double>(A)) * vmin;
  if (out_q) out_q[slot] = 1.0;
  if (out_lambda)
    for (int32_t i = 0; i < A; ++i) out_lambda[slot * A + i] = i == S.agent[kmin] ? 1.0 : 0.0;
  out_pivots[slot] = 0;
}

// The answer of a solve that ended with `status` (block-uniform): q = x / 1.x, lambda = w / 1.w
// and alpha from the optimal basis, or NaN and the negative status
template <int BLOCK>
__device__ __forceinline__ void mmx_write_out(MmxSmem& S, int32_t status, unsigned long long mask,
                                              int32_t A, int32_t r, int32_t m, int64_t slot,
                                              double* out_alpha, double* out_q, double* out_lambda,
                                              int32_t* out_pivots) {
  const int tid = threadIdx.x;
  if (status >= 0) {
    if (tid == 0) {
      double sx = 0.0, sw = 0.0;
      for (int32_t i = 0; i < r; ++i)
        if (S.basis[i] < m) sx += S.xB[i];
      for (int32_t i = 0; i < r; ++i) sw += S.w[i];
      S.sx = sx;
      S.sw = sw;
    }
    __syncthreads();
    if (!(S.sx > 0.0 && S.sx < INFINITY && S.sw > 0.0 && S.sw < INFINITY)) status = -2;
  }
  if (status < 0) {
    const double nan = __builtin_nan("");
    if (out_q)
      for (int32_t j = tid; j < m; j += BLOCK) out_q[slot * m + j] = nan;
    if (out_lambda && tid < A) out_lambda[slot * A + tid] = nan;
    if (tid == 0) {
      out_alpha[slot] = nan;
      out_pivots[slot] = status;
    }
    return;
  }
  const double sx = S.sx, sw = S.sw;
  if (out_q) {
    for (int32_t j = tid; j < m; j += BLOCK) {
      double q = 0.0;
      if (mmx_is_basic(S, j))
        for (int32_t i = 0; i < r; ++i)
          if (S.basis[i] == j) q = S.xB[i] / sx;
      out_q[slot * m + j] = q;
    }
  }
  if (out_lambda && tid < A) {
    double lam = 0.0;
    if ((mask >> tid) & 1ull) lam = S.w[__popcll(mask & ((1ull << tid) - 1ull))] / sw;
    out_lambda[slot * A + tid] = lam;
  }
  if (tid == 0) {
    out_alpha[slot] = (static_cast<double>(r) / static_cast<double>(A)) * (1.0 / sx);
    out_pivots[slot] = status;
  }
}

template <int BLOCK, bool STAGED>
__global__ __launch_bounds__(BLOCK) void maximin_lottery_kernel(
    const double* __restrict__ U, int32_t A, int32_t m, int64_t ldu, int64_t ldp,
    const double* __restrict__ base, const unsigned long long* __restrict__ masks, int32_t C,
    int32_t max_pivots, double* __restrict__ out_alpha, double* __restrict__ out_q,
    double* __restrict__ out_lambda, int32_t* __restrict__ out_pivots) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  __shared__ MmxSmem S;
  const int tid = threadIdx.x;
  const int64_t prob = blockIdx.x / C;
  const int32_t coal = blockIdx.x % C;
  const double* Ug = U + prob * ldp;
  const int64_t slot = prob * C + coal;

  const unsigned long long all = A == 64 ? ~0ull : (1ull << A) - 1ull;
  const unsigned long long mask = (masks ? masks[coal] : all) & all;
  const int32_t r = __popcll(mask);
  const int32_t ldb = r | 1;      // odd row stride: a column of Binv spreads over the banks
  double* Binv = sm;
  double* smM = sm + static_cast<int64_t>(A) * (A | 1);   // where the host put M's share
  const MmxM<STAGED> M{S, smM, Ug, ldu, m};

  const int bad =
      mmx_setup<BLOCK, STAGED>(S, Ug, A, m, ldu, base ? base + prob * A : nullptr, mask, r, smM);
  int32_t status = bad ? -1 : 0;           // block-uniform from here on
  if (!bad && m == 1) {
    mmx_write_one_column(S, M, A, r, slot, out_alpha, out_q, out_lambda, out_pivots);
    return;
  }
  if (!bad) {
    // the all-slack basis: Binv = I, xB = -1, w = 0, the slacks m .. m + r - 1 basic (inline:
    // as a function of its own it costs the one-wave kernel six VGPRs and a wave of occupancy)
    for (int32_t idx = tid; idx < r * r; idx += BLOCK) {
      const int32_t i = idx / r, l = idx - i * r;
      Binv[i * ldb + l] = i == l ? 1.0 : 0.0;
    }
    if (tid < r) {
      S.xB[tid] = -1.0;
      S.w[tid] = 0.0;
      S.basis[tid] = m + tid;
    }
    for (int32_t wi = tid; wi < (m + r + 31) / 32; wi += BLOCK) {
      uint32_t v = 0;
      for (int b = 0; b < 32; ++b) {
        const int32_t j = wi * 32 + b;
        if (j >= m && j < m + r) v |= 1u << b;
      }
      S.basic[wi] = v;
    }
    int32_t pivots = 0;
    for (;;) {
      __syncthreads();
      const ArgBest out = mmx_leaving_row(S, r);
      const int32_t k = out.j;
      const double xk = out.v;
      if (!(xk < 0.0)) {
        status = pivots;
        break;
      }
      if (pivots >= max_pivots) {
        status = -2;
        break;
      }
      const int32_t e = mmx_ratio_test<BLOCK, STAGED>(S, M, Binv + k * ldb, r, m);
      if (e >= m + r) {                    // no column can enter: rounding only, the LP is feasible
        status = -2;
        break;
      }
      mmx_pivot<BLOCK, STAGED>(S, M, Binv, ldb, k, xk, e, r, m);
      ++pivots;
    }
  }
  mmx_write_out<BLOCK>(S, status, mask, A, r, m, slot, out_alpha, out_q, out_lambda, out_pivots);
}

// ---------------------------------------------------------------------------
// cs_policy_rollout: leaves sampled step by step from a token policy, with numpy's own draws
// ---------------------------------------------------------------------------
// Generator.choice(B, p=probs) is cdf = cumsum(probs); cdf /= cdf[-1]; u = random(); a = the
// number of cdf entries <= u: one double of the PCG64 stream per draw.  Two kernels on the stream:
//   rollout_cdf_kernel   one workgroup per problem, one thread per row of B probabilities: the
//                        row is checked, summed left to right and divided by its last running
//                        sum into cdf_work; the problem's status is written (0 / -1);
//   rollout_walk_kernel  one workgroup per (problem, kRollPerGroup samples), each thread a
//                        contiguous run of kRollPerThread samples: one O(log) jump of the LCG to
//                        the run's first draw, then L sequential draws per sample.  The leaves
//                        are counted in an int32 LDS histogram whose nonzero bins are added to
//                        out_counts with integer atomics (the sums do not depend on the order).
// A row's cdf is nondecreasing (running sums of entries >= 0, then a monotone division), so the
// count of entries <= u is found by bisection.  A problem of status -1 is skipped by every
// workgroup of the walk.
constexpr int kRollBlock = 256;
constexpr int kRollPerThread = 16;
constexpr int kRollPerGroup = kRollBlock * kRollPerThread;   // 4096 samples
constexpr double kRollSumTol = 0x1p-26;       // sqrt(DBL_EPSILON): numpy's check of sum(p)

typedef unsigned __int128 u128;

__host__ __device__ __forceinline__ u128 make_u128(uint64_t hi, uint64_t lo) {
  return (static_cast<u128>(hi) << 64) | lo;
}

// PCG64's 128-bit LCG multiplier (0x2360ED051FC65DA4'4385DF649FCCF645)
__device__ __forceinline__ u128 pcg_mult() {
  return make_u128(0x2360ED051FC65DA4ull, 0x4385DF649FCCF645ull);
}

// the state after `delta` steps state <- state * mult + inc: square-and-multiply on (mult, inc)
__device__ __forceinline__ u128 pcg_advance(u128 state, u128 inc, uint64_t delta) {
  u128 acc_mult = 1, acc_plus = 0, cur_mult = pcg_mult(), cur_plus = inc;
  while (delta > 0) {
    if (delta & 1) {
      acc_mult *= cur_mult;
      acc_plus = acc_plus * cur_mult + cur_plus;
    }
    cur_plus = (cur_mult + 1) * cur_plus;
    cur_mult *= cur_mult;
    delta >>= 1;
  }
  return acc_mult * state + acc_plus;
}

// one step, then the XSL-RR output of the new state as numpy's double in [0, 1)
__device__ __forceinline__ double pcg_next_double(u128& state, u128 inc) {
  state = state * pcg_mult() + inc;
  const uint64_t hi = static_cast<uint64_t>(state >> 64), lo = static_cast<uint64_t>(state);
  const uint64_t x = hi ^ lo;
  const unsigned rot = static_cast<unsigned>(hi >> 58);
  const uint64_t out = (x >> rot) | (x << ((64u - rot) & 63u));
  return static_cast<double>(out >> 11) * (1.0 / 9007199254740992.0);
}

__global__ __launch_bounds__(kRollBlock) void rollout_cdf_kernel(
    const double* __restrict__ policy, int32_t B, int32_t rows, double* __restrict__ cdf,
    int32_t* __restrict__ out_status) {
  const int64_t base = static_cast<int64_t>(blockIdx.x) * rows * B;
  int bad = 0;
  for (int32_t r = threadIdx.x; r < rows; r += kRollBlock) {
    const double* row = policy + base + static_cast<int64_t>(r) * B;
    double* out = cdf + base + static_cast<int64_t>(r) * B;
    double acc = 0.0;
    for (int32_t b = 0; b < B; ++b) {
      const double v = row[b];
      if (!(v >= 0.0) || v == INFINITY) bad = 1;
      acc += v;
      out[b] = acc;
    }
    if (!(fabs(acc - 1.0) <= kRollSumTol)) bad = 1;
    for (int32_t b = 0; b < B; ++b) out[b] = out[b] / acc;
  }
  bad = __syncthreads_or(bad);
  if (threadIdx.x == 0) out_status[blockIdx.x] = bad ? -1 : 0;
}

__global__ __launch_bounds__(kRollBlock) void rollout_walk_kernel(
    const double* __restrict__ cdf, int32_t B, int32_t L, int32_t m, int32_t rows,
    const uint64_t* __restrict__ rng, int64_t first_sample, int64_t num_samples, int64_t chunks,
    const int32_t* __restrict__ status, unsigned long long* __restrict__ out_counts,
    int32_t* __restrict__ out_leaf) {
  extern __shared__ __attribute__((aligned(16))) int32_t hist[];   // [m]
  const int tid = threadIdx.x;
  const int64_t prob = blockIdx.x / chunks;
  const int64_t chunk = blockIdx.x % chunks;
  if (status[prob] != 0) return;               // block-uniform
  for (int32_t j = tid; j < m; j += kRollBlock) hist[j] = 0;
  __syncthreads();

  const int64_t first = chunk * kRollPerGroup + static_cast<int64_t>(tid) * kRollPerThread;
  if (first < num_samples) {
    const int64_t left = num_samples - first;
    const int32_t n = left < kRollPerThread ? static_cast<int32_t>(left) : kRollPerThread;
    const uint64_t* g = rng + prob * 4;
    const u128 inc = make_u128(g[2], g[3]);
    // sample i of the rollout owns the draws i * L .. i * L + L - 1 (< 2^62, checked on the host)
    u128 state = pcg_advance(make_u128(g[0], g[1]), inc,
                             static_cast<uint64_t>(first_sample + first) * static_cast<uint64_t>(L));
    const double* pc = cdf + prob * rows * B;
    for (int32_t i = 0; i < n; ++i) {
      int32_t s = 0, row0 = 0, width = 1;      // row0: the level's first row, width = B^t rows
      for (int32_t t = 0; t < L; ++t) {
        const double u = pcg_next_double(state, inc);
        const double* row = pc + static_cast<int64_t>(row0 + s) * B;
        int32_t lo = 0, hi = B - 1;            // the last entry is 1.0 > u: a <= B - 1
        while (lo < hi) {
          const int32_t mid = (lo + hi) >> 1;
          if (row[mid] <= u) lo = mid + 1;
          else hi = mid;
        }
        s = s * B + lo;
        row0 += width;
        width *= B;
      }
      atomicAdd(&hist[s], 1);
      if (out_leaf) out_leaf[prob * num_samples + first + i] = s;
    }
  }
  __syncthreads();
  for (int32_t j = tid; j < m; j += kRollBlock) {
    const int32_t c = hist[j];
    if (c) atomicAdd(out_counts + prob * m + j, static_cast<unsigned long long>(c));
  }
}

// B^L if it is <= limit, else -1 (no overflow: stops at the first product past the limit)
int64_t pow_limited(int32_t B, int32_t L, int64_t limit) {
  int64_t n = 1;
  for (int32_t t = 0; t < L; ++t) {
    n *= B;
    if (n > limit) return -1;
  }
  return n;
}

// Argument checks (w: the entry point's name as the messages' prefix): the P problems [A, m] of
// the two solvers
int check_problems(const std::string& w, int32_t P, int32_t A, int32_t m, int64_t ldu, int64_t ldp) {
  if (P < 0) return fail(CS_ERR_INVALID, w + "need P >= 0");
  if (A < 1 || A > kLotMaxA) return fail(CS_ERR_INVALID, w + "need 1 <= A <= 64");
  if (m < 1 || m > kLotMaxM) return fail(CS_ERR_INVALID, w + "need 1 <= m <= 16384");
  if (ldu < m) return fail(CS_ERR_INVALID, w + "need ldu >= m");
  if (ldp < static_cast<int64_t>(A - 1) * ldu + m)
    return fail(CS_ERR_INVALID, w + "problems overlap (need ldp_problem >= (A - 1) * ldu + m)");
  return CS_OK;
}

// the P token trees of B actions and depth L; m = B^L leaves, total = sum_t B^t entries (t = 1..L)
int check_trees(const std::string& w, int32_t P, int32_t B, int32_t L, int64_t& m, int64_t& total) {
  if (P < 0) return fail(CS_ERR_INVALID, w + "need P >= 0");
  if (B < 1 || L < 1) return fail(CS_ERR_INVALID, w + "need B >= 1 and L >= 1");
  if (L > kPolicyMaxL) return fail(CS_ERR_INVALID, w + "need L <= 64");
  m = pow_limited(B, L, kLotMaxM);
  if (m < 0) return fail(CS_ERR_INVALID, w + "need B^L <= 16384");
  total = 0;
  for (int64_t t = 1, n = B; t <= L; ++t, n *= B) total += n;
  return CS_OK;
}

// f(block, staged): BLOCK (1024 when wide, else 256) and STAGED as integral_constant values
template <typename F>
void dispatch_block_staged(bool wide, bool staged, F&& f) {
  auto go = [&](auto block) {
    if (staged) f(block, std::true_type{});
    else f(block, std::false_type{});
  };
  if (wide) go(std::integral_constant<int, 1024>{});
  else go(std::integral_constant<int, 256>{});
}

}  // namespace

extern "C" {

int cs_nash_lottery(const double* U, int32_t P, int32_t A, int32_t m, int64_t ldu,
                    int64_t ldp_problem, int32_t max_iters, double tol, int variant, double* out_p,
                    double* out_a, double* out_F, double* out_gap, int32_t* out_iters,
                    cs_stream_t stream) {
  const std::string w = "cs_nash_lottery: ";
  if (int rc = check_problems(w, P, A, m, ldu, ldp_problem)) return rc;
  if (max_iters < 0) return fail(CS_ERR_INVALID, w + "need max_iters >= 0");
  if (!std::isfinite(tol)) return fail(CS_ERR_INVALID, w + "tol must be finite");
  if (variant < 0 || variant > 2) return fail(CS_ERR_INVALID, w + "unknown variant");
  const size_t u_bytes = static_cast<size_t>(A) * m * sizeof(double);
  if (variant == 1 && u_bytes > kLotLdsBytes)
    return fail(CS_ERR_INVALID, w + "variant 1 needs A * m * 8 bytes of LDS, at most 147456");
  if (P == 0) return CS_OK;
  if (!U || !out_p) return fail(CS_ERR_INVALID, w + "NULL pointer");
  if (misaligned(U, 8) || misaligned(out_p, 8) || misaligned(out_a, 8) || misaligned(out_F, 8) ||
      misaligned(out_gap, 8) || misaligned(out_iters, 4))
    return fail(CS_ERR_INVALID, w + "U and the fp64 outputs must be 8-byte aligned");
  // variant 0: staged whenever U fits ("The Nash-welfare lottery")
  const bool staged = variant == 1 || (variant == 0 && u_bytes <= kLotLdsBytes);
  dispatch_block_staged(m > kLotWideM, staged, [&](auto block, auto stg) {
    constexpr int BLOCK = decltype(block)::value;
    constexpr bool STAGED = decltype(stg)::value;
    launch_big_lds<&nash_lottery_kernel<BLOCK, STAGED>>(
        kLotLdsBytes, dim3(P), dim3(BLOCK), STAGED ? u_bytes : 0, static_cast<hipStream_t>(stream),
        U, A, m, ldu, ldp_problem, max_iters, tol, out_p, out_a, out_F, out_gap, out_iters);
  });
  return check_launch("cs_nash_lottery");
}

int cs_maximin_lottery(const double* U, int32_t P, int32_t A, int32_t m, int64_t ldu,
                       int64_t ldp_problem, const double* base, const uint64_t* masks_host,
                       const uint64_t* masks, int32_t C, int32_t max_pivots, double* out_alpha,
                       double* out_q, double* out_lambda, int32_t* out_pivots, cs_stream_t stream) {
  const std::string w = "cs_maximin_lottery: ";
  if (int rc = check_problems(w, P, A, m, ldu, ldp_problem)) return rc;
  if (max_pivots < 0) return fail(CS_ERR_INVALID, w + "need max_pivots >= 0");
  if (C < 1) return fail(CS_ERR_INVALID, w + "need C >= 1");
  if ((masks_host == nullptr) != (masks == nullptr))
    return fail(CS_ERR_INVALID, w + "masks_host and masks come together (or both NULL)");
  if (!masks && C != 1) return fail(CS_ERR_INVALID, w + "NULL masks mean one coalition (C = 1)");
  if (masks_host) {
    const uint64_t all = A == 64 ? ~uint64_t{0} : (uint64_t{1} << A) - 1;
    for (int32_t c = 0; c < C; ++c) {
      if (masks_host[c] == 0) return fail(CS_ERR_INVALID, w + "empty coalition mask");
      if (masks_host[c] & ~all) return fail(CS_ERR_INVALID, w + "coalition mask names an agent >= A");
    }
  }
  const int64_t grid = static_cast<int64_t>(P) * C;
  if (int rc = check_grid("cs_maximin_lottery", grid)) return rc;
  if (P == 0) return CS_OK;
  if (!U || !out_alpha || !out_pivots) return fail(CS_ERR_INVALID, w + "NULL pointer");
  if (misaligned(U, 8) || misaligned(base, 8) || misaligned(masks, 8) || misaligned(out_alpha, 8) ||
      misaligned(out_q, 8) || misaligned(out_lambda, 8) || misaligned(out_pivots, 4))
    return fail(CS_ERR_INVALID, w + "U, base, masks and the fp64 outputs must be 8-byte aligned");
  // Binv's share is sized by A (a coalition has at most A rows); M is staged whenever it fits too
  const size_t binv_bytes = static_cast<size_t>(A) * (A | 1) * sizeof(double);
  const size_t m_bytes = static_cast<size_t>(A) * m * sizeof(double);
  const bool staged = binv_bytes + m_bytes <= kLotLdsBytes;
  auto go = [&](auto block, auto stg) {
    constexpr int BLOCK = decltype(block)::value;
    constexpr bool STAGED = decltype(stg)::value;
    launch_big_lds<&maximin_lottery_kernel<BLOCK, STAGED>>(
        kLotLdsBytes, dim3(static_cast<uint32_t>(grid)), dim3(BLOCK),
        binv_bytes + (STAGED ? m_bytes : 0), static_cast<hipStream_t>(stream), U, A, m, ldu,
        ldp_problem, base, reinterpret_cast<const unsigned long long*>(masks), C, max_pivots,
        out_alpha, out_q, out_lambda, out_pivots);
  };
  // one wave per workgroup up to kMmxNarrowM columns: 64 x 65 + 64 x 128 doubles always fit
  if (m <= kMmxNarrowM) go(std::integral_constant<int, 64>{}, std::true_type{});
  else dispatch_block_staged(m > kLotWideM, staged, go);
  return check_launch("cs_maximin_lottery");
}

int cs_lottery_policy(const double* p, int32_t P, int32_t B, int32_t L, double* out_policy,
                      cs_stream_t stream) {
  const std::string w = "cs_lottery_policy: ";
  int64_t m, total;
  if (int rc = check_trees(w, P, B, L, m, total)) return rc;
  if (P == 0) return CS_OK;
  if (!p || !out_policy) return fail(CS_ERR_INVALID, w + "NULL pointer");
  if (misaligned(p, 8) || misaligned(out_policy, 8))
    return fail(CS_ERR_INVALID, w + "p and out_policy must be 8-byte aligned");
  hipLaunchKernelGGL(lottery_policy_kernel, dim3(P), dim3(kPolicyBlock), 0,
                     static_cast<hipStream_t>(stream), p, B, L, static_cast<int32_t>(m),
                     static_cast<int32_t>(total), out_policy);
  return check_launch("cs_lottery_policy");
}

int cs_policy_rollout(const double* policy, int32_t P, int32_t B, int32_t L, const uint64_t* rng,
                      int64_t first_sample, int64_t num_samples, double* cdf_work,
                      int64_t* out_counts, int32_t* out_leaf, int32_t* out_status,
                      cs_stream_t stream) {
  const std::string w = "cs_policy_rollout: ";
  int64_t m, total;
  if (int rc = check_trees(w, P, B, L, m, total)) return rc;
  if (first_sample < 0 || num_samples < 0)
    return fail(CS_ERR_INVALID, w + "need first_sample >= 0 and num_samples >= 0");
  const u128 draws = (static_cast<u128>(first_sample) + static_cast<u128>(num_samples)) * L;
  if (draws >= (static_cast<u128>(1) << 62))
    return fail(CS_ERR_INVALID, w + "need (first_sample + num_samples) * L < 2^62");
  if (out_leaf && static_cast<u128>(P) * static_cast<u128>(num_samples) > 0x7fffffffu)
    return fail(CS_ERR_INVALID, w + "out_leaf needs P * num_samples <= 2^31 - 1");
  const int64_t chunks = cdiv(num_samples, kRollPerGroup);
  if (chunks > 0x7fffffffLL) return fail(CS_ERR_INVALID, w + "grid too large");
  if (int rc = check_grid("cs_policy_rollout", static_cast<int64_t>(P) * chunks)) return rc;
  if (P == 0 || num_samples == 0) return CS_OK;
  if (!policy || !rng || !cdf_work || !out_counts || !out_status)
    return fail(CS_ERR_INVALID, w + "NULL pointer");
  if (misaligned(policy, 8) || misaligned(rng, 8) || misaligned(cdf_work, 8) ||
      misaligned(out_counts, 8) || misaligned(out_leaf, 4) || misaligned(out_status, 4))
    return fail(CS_ERR_INVALID, w + "policy, rng, cdf_work and out_counts must be 8-byte aligned");
  const int32_t rows = static_cast<int32_t>(total / B);
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(rollout_cdf_kernel, dim3(P), dim3(kRollBlock), 0, st, policy, B, rows, cdf_work,
                     out_status);
  hipLaunchKernelGGL(rollout_walk_kernel, dim3(static_cast<uint32_t>(P * chunks)), dim3(kRollBlock),
                     static_cast<size_t>(m) * sizeof(int32_t), st, cdf_work, B, L,
                     static_cast<int32_t>(m), rows, rng, first_sample, num_samples, chunks, out_status,
                     reinterpret_cast<unsigned long long*>(out_counts), out_leaf);
  return check_launch("cs_policy_rollout");
}

}  // extern "C"
