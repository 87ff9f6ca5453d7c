// schulze.hip — Schulze rank aggregation, the Habermas Machine's choice among candidate
// statements (the reference's src/methods/habermas_machine.py:1030-1261): pairwise defeats,
// strongest-path strengths, the tied social ranking, the ballot tie-break and the winner of a
// whole batch of elections in one launch, one workgroup per election.
#include "cs_kernels.cuh"

namespace {

// ---------------------------------------------------------------------------
// cs_schulze: one workgroup per election, the whole aggregation in LDS
// ---------------------------------------------------------------------------
// LDS: the C x C int32 matrix (row stride C | 1, odd) that holds the defeats d and then, in
// place, the path strengths p; one tile of kSchTile voters ([kSchTile][C], int32 ranks or float
// scores); five int32 vectors of length C.
//   stage 1  the voters pass through the tile kSchTile at a time.  The unordered pairs (i, j),
//            i < j, are numbered q = j (j - 1) / 2 + i and thread tid owns q = tid, tid + BLOCK,
//            ...: per tile it counts both directions over the tile's rows and adds them to
//            d[i][j] and d[j][i], which no other thread touches.  Consecutive q share j (a
//            broadcast) and read consecutive i.  A voter that `valid` leaves out is staged as a
//            row of equal entries, which prefers nothing.  Integer sums: any order gives the
//            same result.
//   stage 2  p[i][j] = d[i][j] > d[j][i] ? d[i][j] : 0 (by the pair's owner), then for every
//            pivot k in ascending order p[j][l] = max(p[j][l], min(p[j][k], p[k][l])) over all
//            (j, l) with j != k, l != k, j != l.  A pivot reads row k and column k and writes
//            neither, so its updates are independent and one barrier per pivot orders them
//            against the next pivot's reads: the sequential loop's result exactly.  Lanes map to
//            consecutive l of one row j: p[j][k] is a broadcast, p[k][l] and p[j][l] contiguous.
//   stage 3  count[i] = #{j : p[i][j] >= p[j][i]} (the transposed read walks a column, which the
//            odd stride spreads over the banks); the ranking is the dense rank of -count, the
//            ballot's tie-break two more dense ranks.  A dense rank of C values is two O(C)
//            scans per thread: first occurrences, then the first occurrences below the own value.
// No atomics, no global scratch, no host sync.  Two workgroup sizes: one wave up to
// kSchNarrowC candidates (the Habermas Machine's own sizes: thousands of small elections fill
// the chip), four waves above.
constexpr int kSchMaxC = 128;
constexpr int kSchMaxR = 65536;
constexpr int kSchTile = 32;                  // voters staged per pass (tests sit on its edges)
constexpr int kSchNarrowC = 16;               // up to this many candidates: one wave per workgroup
constexpr int kSchVecs = 5;
constexpr int kSchRows = 8;                   // four waves: rows of a pivot update loaded together

constexpr size_t sch_lds_bytes(int C) {
  return (static_cast<size_t>(C) * (C | 1) + static_cast<size_t>(kSchTile) * C +
          static_cast<size_t>(kSchVecs) * C) * sizeof(int32_t);
}
constexpr size_t kSchLdsMax = sch_lds_bytes(kSchMaxC);   // 84,992 bytes at C = 128

// ranks: lower is better; scores: higher is better, a NaN prefers nothing
__device__ __forceinline__ bool sch_prefers(int32_t a, int32_t b) { return a < b; }
__device__ __forceinline__ bool sch_prefers(float a, float b) { return a > b; }

// q = j (j - 1) / 2 + i, i < j  ->  (i, j)
__device__ __forceinline__ void sch_pair(int32_t q, int32_t& i, int32_t& j) {
  int32_t jj = static_cast<int32_t>((1.0f + sqrtf(static_cast<float>(8 * q + 1))) * 0.5f);
  while (jj * (jj - 1) / 2 > q) --jj;
  while ((jj + 1) * jj / 2 <= q) ++jj;
  j = jj;
  i = q - jj * (jj - 1) / 2;
}

// out[i] = the number of distinct values of v below v[i] (np.unique's inverse); first is scratch
template <int BLOCK>
__device__ __forceinline__ void sch_dense_rank(const int32_t* v, int32_t* first, int32_t* out,
                                               int32_t C) {
  const int tid = threadIdx.x;
  __syncthreads();
  for (int32_t i = tid; i < C; i += BLOCK) {
    const int32_t x = v[i];
    int32_t f = 1;
    for (int32_t j = 0; j < i; ++j)
      if (v[j] == x) f = 0;
    first[i] = f;
  }
  __syncthreads();
  for (int32_t i = tid; i < C; i += BLOCK) {
    const int32_t x = v[i];
    int32_t n = 0;
    for (int32_t j = 0; j < C; ++j) n += (first[j] != 0 && v[j] < x) ? 1 : 0;
    out[i] = n;
  }
  __syncthreads();
}

// stage 1 for one element type; returns (to every thread) whether a counted rank was out of range
template <int BLOCK, typename T>
__device__ __forceinline__ int sch_defeats(const T* __restrict__ in, const uint8_t* __restrict__ valid,
                                           int32_t R, int32_t C, int32_t ld, int32_t* mat,
                                           int32_t* tile_words) {
  const int tid = threadIdx.x;
  T* tile = reinterpret_cast<T*>(tile_words);
  const int32_t npairs = C * (C - 1) / 2;
  int bad = 0;
  for (int32_t idx = tid; idx < C * ld; idx += BLOCK) mat[idx] = 0;
  for (int32_t r0 = 0; r0 < R; r0 += kSchTile) {
    const int32_t rows = R - r0 < kSchTile ? R - r0 : kSchTile;
    __syncthreads();   // the matrix is zeroed / the previous tile has been counted
    for (int32_t idx = tid; idx < rows * C; idx += BLOCK) {
      const int32_t t = idx / C;
      T x = in[static_cast<int64_t>(r0) * C + idx];
      if (valid && valid[r0 + t] == 0) {
        x = T(0);
      } else if (std::is_same<T, int32_t>::value) {
        if (x < T(0) || x >= T(C)) bad = 1;
      }
      tile[idx] = x;
    }
    __syncthreads();
    for (int32_t q = tid; q < npairs; q += BLOCK) {
      int32_t i, j;
      sch_pair(q, i, j);
      int32_t nij = 0, nji = 0;
      for (int32_t t = 0; t < rows; ++t) {
        const T a = tile[t * C + i], b = tile[t * C + j];
        nij += sch_prefers(a, b) ? 1 : 0;
        nji += sch_prefers(b, a) ? 1 : 0;
      }
      mat[i * ld + j] += nij;
      mat[j * ld + i] += nji;
    }
  }
  return __syncthreads_or(bad);
}

template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void schulze_kernel(
    const void* __restrict__ in, int kind, int32_t R, int32_t C, const uint8_t* __restrict__ valid,
    const int32_t* __restrict__ ballot, int32_t* __restrict__ out_defeats,
    int32_t* __restrict__ out_strengths, int32_t* __restrict__ out_ranking,
    int32_t* __restrict__ out_untied, int32_t* __restrict__ out_winner,
    int32_t* __restrict__ out_status) {
  extern __shared__ __attribute__((aligned(16))) int32_t sch_sm[];
  const int tid = threadIdx.x;
  const int64_t e = blockIdx.x;
  const int32_t ld = C | 1;
  int32_t* mat = sch_sm;                       // [C][ld]
  int32_t* tile = mat + C * ld;                // [kSchTile][C]
  int32_t* vec = tile + kSchTile * C;          // kSchVecs x [C]
  int32_t* v_key = vec;                        // the values being ranked
  int32_t* v_first = vec + C;
  int32_t* v_rank = vec + 2 * C;               // the tied social ranking
  int32_t* v_nb = vec + 3 * C;                 // the ballot's dense rank
  int32_t* v_untied = vec + 4 * C;
  const int64_t cc = static_cast<int64_t>(C) * C;
  const int32_t npairs = C * (C - 1) / 2;

  int32_t status = 0;                          // block-uniform
  if (kind <= 1) {
    const uint8_t* val = valid ? valid + e * R : nullptr;
    if (val) {
      int any = 0;
      for (int32_t r = tid; r < R; r += BLOCK) any |= val[r] != 0;
      if (!__syncthreads_or(any)) status = -2;
    }
    if (status == 0) {
      const int64_t off = e * R * C;
      const int bad = kind == 0
          ? sch_defeats<BLOCK, int32_t>(static_cast<const int32_t*>(in) + off, val, R, C, ld, mat, tile)
          : sch_defeats<BLOCK, float>(static_cast<const float*>(in) + off, val, R, C, ld, mat, tile);
      if (bad) status = -1;
    }
  } else {
    // a defeat or strength matrix from the caller: staged, its diagonal checked
    const int32_t* src = static_cast<const int32_t*>(in) + e * cc;
    int bad = 0;
    for (int32_t idx = tid; idx < C * C; idx += BLOCK) {
      const int32_t i = idx / C, j = idx - i * C;
      const int32_t x = src[idx];
      if (i == j && x != 0) bad = 1;
      mat[i * ld + j] = x;
    }
    if (__syncthreads_or(bad)) status = -1;
  }

  if (status != 0) {
    if (out_defeats && kind <= 1)
      for (int32_t idx = tid; idx < C * C; idx += BLOCK) out_defeats[e * cc + idx] = -1;
    if (out_strengths && kind <= 2)
      for (int32_t idx = tid; idx < C * C; idx += BLOCK) out_strengths[e * cc + idx] = -1;
    for (int32_t i = tid; i < C; i += BLOCK) {
      out_ranking[e * C + i] = -1;
      if (out_untied) out_untied[e * C + i] = -1;
    }
    if (tid == 0) {
      if (out_winner) out_winner[e] = -1;
      out_status[e] = status;
    }
    return;
  }

  if (kind <= 1 && out_defeats) {
    for (int32_t idx = tid; idx < C * C; idx += BLOCK) {
      const int32_t i = idx / C, j = idx - i * C;
      out_defeats[e * cc + idx] = mat[i * ld + j];
    }
    __syncthreads();                           // d is read out before stage 2 overwrites it
  }

  if (kind <= 2) {
    // p = where(d > d^T, d, 0), diagonal 0: by the owner of each pair
    for (int32_t q = tid; q < npairs; q += BLOCK) {
      int32_t i, j;
      sch_pair(q, i, j);
      const int32_t a = mat[i * ld + j], b = mat[j * ld + i];
      mat[i * ld + j] = a > b ? a : 0;
      mat[j * ld + i] = b > a ? b : 0;
    }
    for (int32_t i = tid; i < C; i += BLOCK) mat[i * ld + i] = 0;
    // lanes over W >= C consecutive l (a power of two), BLOCK / W rows j at a time
    int32_t shift = 0;
    while ((1 << shift) < C) ++shift;          // W <= 16 in one wave, <= 128 in four: W <= BLOCK
    const int32_t l = tid & ((1 << shift) - 1);
    const int32_t j0 = tid >> shift, jstep = BLOCK >> shift;
    for (int32_t k = 0; k < C; ++k) {
      __syncthreads();                         // the previous pivot's writes (or the init above)
      if (l < C && l != k) {
        const int32_t pkl = mat[k * ld + l];
        // ROWS rows at a time: their loads are issued together, ahead of the stores (one wave
        // has at most four rows per thread and takes them one by one)
        constexpr int ROWS = BLOCK == 64 ? 1 : kSchRows;
        for (int32_t jb = j0; jb < C; jb += jstep * ROWS) {
          int32_t pjk[ROWS], pjl[ROWS];
#pragma unroll
          for (int u = 0; u < ROWS; ++u) {
            const int32_t j = jb + u * jstep;
            const bool on = j < C;
            pjk[u] = on ? mat[j * ld + k] : 0;
            pjl[u] = on ? mat[j * ld + l] : 0;
          }
#pragma unroll
          for (int u = 0; u < ROWS; ++u) {
            const int32_t j = jb + u * jstep;
            const int32_t via = pjk[u] < pkl ? pjk[u] : pkl;
            if (j < C && j != k && j != l && via > pjl[u]) mat[j * ld + l] = via;
          }
        }
      }
    }
    __syncthreads();
    if (out_strengths) {
      for (int32_t idx = tid; idx < C * C; idx += BLOCK) {
        const int32_t i = idx / C, j = idx - i * C;
        out_strengths[e * cc + idx] = mat[i * ld + j];
      }
    }
  }

  // stage 3: -count, so that its dense rank is np.unique(-count, return_inverse=True)
  for (int32_t i = tid; i < C; i += BLOCK) {
    int32_t n = 0;
    for (int32_t j = 0; j < C; ++j) n += mat[i * ld + j] >= mat[j * ld + i] ? 1 : 0;
    v_key[i] = -n;
  }
  sch_dense_rank<BLOCK>(v_key, v_first, v_rank, C);
  for (int32_t i = tid; i < C; i += BLOCK) out_ranking[e * C + i] = v_rank[i];
  const int32_t* final_rank = v_rank;
  if (ballot) {
    // _hm_untie_ranking_with_ballot: normalise the ballot, key = rank * C + it, normalise
    for (int32_t i = tid; i < C; i += BLOCK) v_key[i] = ballot[e * C + i];
    sch_dense_rank<BLOCK>(v_key, v_first, v_nb, C);
    for (int32_t i = tid; i < C; i += BLOCK) v_key[i] = v_rank[i] * C + v_nb[i];
    sch_dense_rank<BLOCK>(v_key, v_first, v_untied, C);
    if (out_untied)
      for (int32_t i = tid; i < C; i += BLOCK) out_untied[e * C + i] = v_untied[i];
    final_rank = v_untied;
  }
  if (tid == 0) {
    if (out_winner) {
      int32_t w = 0;                           // a dense rank always holds a 0
      while (w < C - 1 && final_rank[w] != 0) ++w;
      out_winner[e] = w;
    }
    out_status[e] = 0;
  }
}

}  // namespace

extern "C" {

int cs_schulze(const void* in, int in_kind, int32_t E, int32_t R, int32_t C, const uint8_t* valid,
               const int32_t* ballot, int32_t* out_defeats, int32_t* out_strengths,
               int32_t* out_ranking, int32_t* out_untied, int32_t* out_winner, int32_t* out_status,
               cs_stream_t stream) {
  const std::string w = "cs_schulze: ";
  if (E < 0) return fail(CS_ERR_INVALID, w + "need E >= 0");
  if (in_kind < CS_SCHULZE_RANKINGS || in_kind > CS_SCHULZE_STRENGTHS)
    return fail(CS_ERR_INVALID, w + "unknown in_kind (0 rankings, 1 scores, 2 defeats, 3 strengths)");
  if (C < 1 || C > kSchMaxC) return fail(CS_ERR_INVALID, w + "need 1 <= C <= 128");
  const bool voters = in_kind <= CS_SCHULZE_SCORES;
  if (voters && (R < 1 || R > kSchMaxR)) return fail(CS_ERR_INVALID, w + "need 1 <= R <= 65536");
  if (out_untied && !ballot) return fail(CS_ERR_INVALID, w + "out_untied needs a ballot");
  if (int rc = check_grid("cs_schulze", E)) return rc;
  if (E == 0) return CS_OK;
  if (!in || !out_ranking || !out_status) return fail(CS_ERR_INVALID, w + "NULL pointer");
  if (misaligned(in, 4) || misaligned(ballot, 4) || misaligned(out_defeats, 4) ||
      misaligned(out_strengths, 4) || misaligned(out_ranking, 4) || misaligned(out_untied, 4) ||
      misaligned(out_winner, 4) || misaligned(out_status, 4))
    return fail(CS_ERR_INVALID, w + "in, ballot and the outputs must be 4-byte aligned");
  hipStream_t st = static_cast<hipStream_t>(stream);
  const size_t lds = sch_lds_bytes(C);
  if (!voters) {
    R = 0;
    valid = nullptr;
  }
  auto go = [&](auto block) {
    constexpr int BLOCK = decltype(block)::value;
    launch_big_lds<&schulze_kernel<BLOCK>>(kSchLdsMax, dim3(static_cast<uint32_t>(E)), dim3(BLOCK),
                                           lds, st, in, in_kind, R, C, valid, ballot, out_defeats,
                                           out_strengths, out_ranking, out_untied, out_winner,
                                           out_status);
  };
  if (C <= kSchNarrowC) go(std::integral_constant<int, 64>{});
  else go(std::integral_constant<int, 256>{});
  return check_launch("cs_schulze");
}

}  // extern "C"
