// cluster.hip — the data-preparation pipeline's clustering step (the reference's
// data/cluster_habermas_issues.py): StandardScaler, KMeans(n_init restarts of k-means++ and
// Lloyd's iteration, scikit-learn's decisions restated) and the nearest row to each centre, all
// arithmetic fp64.
//
// Kernel boundaries are the only grid-wide synchronisation.  Every sum over points is folded in a
// fixed order (a tile's or a segment's partial by one thread in index order, the partials in
// tile order), there is no floating-point atomic: two runs are bitwise equal.  The only atomics
// are integer: the count of changed labels, the count of live restarts, and the LDS index minimum
// of the same-partition test.
//
// One distance routine serves every stage: a workgroup holds kKmTile points, streams them and up
// to 64 "centre" rows through LDS kKmChunk features at a time, and each thread accumulates the
// squared distances of one point to every fourth centre, features in ascending order.
#include "cs_kernels.cuh"

#include <cfloat>

namespace {

constexpr int kKmMaxK = CS_KMEANS_MAX_K;
constexpr int kKmMaxD = CS_KMEANS_MAX_D;
constexpr int kKmMaxN = CS_KMEANS_MAX_N;
constexpr int kKmMaxR = CS_KMEANS_MAX_R;
constexpr int kKmMaxT = 8;                    // k-means++ trials per centre: 2 + int(log k) <= 6
constexpr int kKmTile = 64;                   // points per workgroup (tests sit on its edges)
constexpr int kKmChunk = 32;                  // features staged per pass
constexpr int kKmSeg = 128;                   // points per segment of the cluster sums
constexpr int kKmRegK = 8;                    // up to this many clusters: segment sums in registers
constexpr int kKmBlock = 256;
constexpr int kKmColParts = 256;              // at most this many row partials per column sum
constexpr int kKmDistLds = kKmTile * (kKmChunk + 1) + 64 * kKmChunk;   // doubles; = 64 * 65

static_assert(kKmDistLds == kKmTile * 65, "the distance matrix reuses the staging buffers");

inline size_t up16(size_t x) { return (x + 15) & ~static_cast<size_t>(15); }

// ---------------------------------------------------------------------------------------------
// distances of a tile of points to nc <= 64 centre rows
// ---------------------------------------------------------------------------------------------
// buf: kKmDistLds doubles.  On return buf[p * 65 + c] = |Z[i0 + p] - C[row(c)]|^2 for p < 64,
// c < nc (rows at or above n count as zero rows: their entries are never used), behind a barrier.
// row(c) = cidx ? cidx[c] : c.  Thread tid owns point p = tid & 63 and centres (tid >> 6) + 4 j,
// j < NJ >= ceil(nc / 4): the centre rows at and above nc are staged as zeros and accumulated
// like the others (no branch in the inner loop, so its NJ LDS reads are issued together) but
// never written out.
template <int NJ>
__device__ __forceinline__ void km_tile_dists_n(const double* __restrict__ Z, int64_t ldz, int32_t n,
                                                int32_t d, int32_t i0, const double* __restrict__ C,
                                                int64_t ldc, const int32_t* __restrict__ cidx,
                                                int32_t nc, double* buf) {
  const int tid = threadIdx.x, p = tid & 63, cg = tid >> 6;
  double* zs = buf;                               // [64][kKmChunk + 1]
  double* cs = buf + kKmTile * (kKmChunk + 1);    // [64][kKmChunk]
  double acc[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) acc[j] = 0.0;
  for (int32_t j0 = 0; j0 < d; j0 += kKmChunk) {
    const int32_t w = d - j0 < kKmChunk ? d - j0 : kKmChunk;
    __syncthreads();                              // the previous chunk has been consumed
    for (int idx = tid; idx < kKmTile * kKmChunk; idx += kKmBlock) {
      const int row = idx / kKmChunk, col = idx % kKmChunk;
      const int32_t i = i0 + row;
      zs[row * (kKmChunk + 1) + col] =
          (i < n && col < w) ? Z[static_cast<int64_t>(i) * ldz + j0 + col] : 0.0;
      double cv = 0.0;
      if (row < nc && col < w) {
        const int64_t cr = cidx ? cidx[row] : row;
        cv = C[cr * ldc + j0 + col];
      }
      cs[row * kKmChunk + col] = cv;
    }
    __syncthreads();
    for (int32_t jj = 0; jj < w; ++jj) {
      const double z = zs[p * (kKmChunk + 1) + jj];
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const double df = z - cs[(cg + 4 * j) * kKmChunk + jj];   // wave-uniform address
        acc[j] = fma(df, df, acc[j]);
      }
    }
  }
  __syncthreads();                                // the staging buffers become the matrix
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int c = cg + 4 * j;
    if (c < nc) buf[p * 65 + c] = acc[j];
  }
  __syncthreads();
}

__device__ __forceinline__ void km_tile_dists(const double* __restrict__ Z, int64_t ldz, int32_t n,
                                              int32_t d, int32_t i0, const double* __restrict__ C,
                                              int64_t ldc, const int32_t* __restrict__ cidx,
                                              int32_t nc, double* buf) {
  const int32_t nj = (nc + 3) >> 2;               // block-uniform
  if (nj <= 1) km_tile_dists_n<1>(Z, ldz, n, d, i0, C, ldc, cidx, nc, buf);
  else if (nj <= 2) km_tile_dists_n<2>(Z, ldz, n, d, i0, C, ldc, cidx, nc, buf);
  else if (nj <= 4) km_tile_dists_n<4>(Z, ldz, n, d, i0, C, ldc, cidx, nc, buf);
  else if (nj <= 8) km_tile_dists_n<8>(Z, ldz, n, d, i0, C, ldc, cidx, nc, buf);
  else km_tile_dists_n<16>(Z, ldz, n, d, i0, C, ldc, cidx, nc, buf);
}

// restarts stacked per labelling workgroup: as many as fit 64 centre rows, fewer while the grid
// would leave compute units idle (the grouping changes no result: a restart's labels depend on
// its own centres only)
inline int32_t km_group(int32_t n, int32_t k, int32_t R) {
  const int64_t tiles = (n + kKmTile - 1) / kKmTile;
  int32_t G = 64 / k;
  while (G > 1 && tiles * ((R + G - 1) / G) < 512) --G;
  return G;
}

// ---------------------------------------------------------------------------------------------
// column statistics (the scaler, and the tolerance's mean variance)
// ---------------------------------------------------------------------------------------------
// grid (ceil(d / 64), parts): p1[part][col] = sum over the part's rows of (x - shift[col]),
// p2 the sum of its square; four row lanes per column, each in row order, folded lane 0..3.
__global__ __launch_bounds__(kKmBlock) void km_col_partial_kernel(
    const double* __restrict__ X, int64_t ld, int32_t n, int32_t d, int32_t rows_per_part,
    const double* __restrict__ shift, double* __restrict__ p1, double* __restrict__ p2) {
  __shared__ double s1[4][64], s2[4][64];
  const int tid = threadIdx.x, lane = tid & 63, rl = tid >> 6;
  const int32_t col = blockIdx.x * 64 + lane;
  const int64_t r0 = static_cast<int64_t>(blockIdx.y) * rows_per_part;
  const int64_t r1 = r0 + rows_per_part < n ? r0 + rows_per_part : n;
  double a = 0.0, b = 0.0;
  if (col < d) {
    const double sh = shift ? shift[col] : 0.0;
    for (int64_t r = r0 + rl; r < r1; r += 4) {
      const double x = X[r * ld + col] - sh;
      a += x;
      b += x * x;
    }
  }
  s1[rl][lane] = a;
  s2[rl][lane] = b;
  __syncthreads();
  if (rl == 0 && col < d) {
    const int64_t o = static_cast<int64_t>(blockIdx.y) * d + col;
    p1[o] = ((s1[0][lane] + s1[1][lane]) + s1[2][lane]) + s1[3][lane];
    p2[o] = ((s2[0][lane] + s2[1][lane]) + s2[2][lane]) + s2[3][lane];
  }
}

// mode 0: out[col] = fold(p1) / n (the mean).  mode 1: np.var about the mean the partials were
// shifted by, fold(p2) / n.  mode 2: StandardScaler's scale: var = (fold(p2) - fold(p1)^2 / n) / n,
// 1 for a constant feature (var <= n eps var + (n mean eps)^2), else sqrt(var).
__global__ void km_col_fold_kernel(const double* __restrict__ p1, const double* __restrict__ p2,
                                   int32_t parts, int32_t n, int32_t d, int mode,
                                   const double* __restrict__ mean, double* __restrict__ out) {
  const int32_t col = blockIdx.x * blockDim.x + threadIdx.x;
  if (col >= d) return;
  double a = 0.0, b = 0.0;
  for (int32_t p = 0; p < parts; ++p) {
    a += p1[static_cast<int64_t>(p) * d + col];
    b += p2[static_cast<int64_t>(p) * d + col];
  }
  const double dn = static_cast<double>(n);
  if (mode == 0) {
    out[col] = a / dn;
  } else if (mode == 1) {
    out[col] = b / dn;
  } else {
    const double var = (b - a * a / dn) / dn;
    const double m = mean[col], eps = DBL_EPSILON;
    const double nme = dn * m * eps;
    const double bound = dn * eps * var + nme * nme;
    out[col] = var <= bound ? 1.0 : sqrt(var);
  }
}

__global__ void km_standardize_kernel(const double* __restrict__ X, int64_t ldx, int32_t n,
                                      int32_t d, const double* __restrict__ mean,
                                      const double* __restrict__ scale, double* __restrict__ Z,
                                      int64_t ldz) {
  const int64_t idx = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (idx >= static_cast<int64_t>(n) * d) return;
  const int64_t r = idx / d;
  const int32_t c = static_cast<int32_t>(idx - r * d);
  Z[r * ldz + c] = (X[r * ldx + c] - mean[c]) / scale[c];
}

// tol_abs = mean(var) * tol, the columns in order
__global__ void km_tol_kernel(const double* __restrict__ var, int32_t d, double tol,
                              double* __restrict__ out) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double s = 0.0;
  for (int32_t j = 0; j < d; ++j) s += var[j];
  *out = s / static_cast<double>(d) * tol;
}

struct ColPlan {
  int32_t rows_per_part, parts;
};
inline ColPlan col_plan(int32_t n) {
  ColPlan p;
  const int64_t rp = cdiv(n, kKmColParts);
  p.rows_per_part = static_cast<int32_t>(rp < 256 ? 256 : rp);
  p.parts = static_cast<int32_t>(cdiv(n, p.rows_per_part));
  return p;
}
inline size_t col_ws_doubles(int32_t n, int32_t d) {
  return 2 * static_cast<size_t>(col_plan(n).parts) * d;
}

// mean (mode 0) then the statistic `mode` about it into out2; p1 / p2 are the partials
void launch_col_stats(hipStream_t st, const double* X, int64_t ld, int32_t n, int32_t d, double* p1,
                      double* p2, double* mean, int mode, double* out2) {
  const ColPlan cp = col_plan(n);
  const dim3 grid(static_cast<uint32_t>(cdiv(d, 64)), static_cast<uint32_t>(cp.parts));
  const uint32_t fold_blocks = static_cast<uint32_t>(cdiv(d, 256));
  hipLaunchKernelGGL(km_col_partial_kernel, grid, dim3(kKmBlock), 0, st, X, ld, n, d,
                     cp.rows_per_part, static_cast<const double*>(nullptr), p1, p2);
  hipLaunchKernelGGL(km_col_fold_kernel, dim3(fold_blocks), dim3(256), 0, st, p1, p2, cp.parts, n, d,
                     0, static_cast<const double*>(nullptr), mean);
  hipLaunchKernelGGL(km_col_partial_kernel, grid, dim3(kKmBlock), 0, st, X, ld, n, d,
                     cp.rows_per_part, static_cast<const double*>(mean), p1, p2);
  hipLaunchKernelGGL(km_col_fold_kernel, dim3(fold_blocks), dim3(256), 0, st, p1, p2, cp.parts, n, d,
                     mode, static_cast<const double*>(mean), out2);
}

// ---------------------------------------------------------------------------------------------
// k-means workspace
// ---------------------------------------------------------------------------------------------
struct KmWs {
  double* closest;    // [R][n]   seeding: distance to the nearest chosen centre; Lloyd: to the
                      //          assigned old centre
  double* tilecum;    // [R][tiles]  tile sums of closest, then their inclusive prefix
  double* part;       // [R][kKmMaxT][tiles]  candidate potentials per tile; finish: inertia per tile
  double* pot;        // [R]
  double* sumpart;    // [R][segs][k][d]
  double* sq;         // [R][k][d]  squared centre moves
  double* colp;       // 2 x [parts][d]
  double* colmean;    // [d]
  double* colvar;     // [d]
  double* tol_abs;    // [1]
  int32_t* labels;    // [R][n]
  int32_t* cntpart;   // [R][segs][k]
  int32_t* count;     // [R][k]
  int32_t* reloc;     // [R][k][3]  (empty cluster, point, its label)
  int32_t* nreloc;    // [R]
  int32_t* amax;      // [R]  the first largest cluster after relocation
  int32_t* nchanged;  // [R]
  int32_t* cand;      // [R][kKmMaxT]
  int32_t* chosen;    // [R]
  size_t bytes;
};

KmWs km_layout(void* base, int32_t n, int32_t d, int32_t k, int32_t R) {
  KmWs w;
  char* p = static_cast<char*>(base);
  size_t off = 0;
  const size_t tiles = cdiv(n, kKmTile), segs = cdiv(n, kKmSeg);
  auto take = [&](size_t bytes) {
    char* q = p + off;
    off += up16(bytes);
    return q;
  };
  const size_t sR = R, sn = n, sd = d, sk = k;
  w.closest = reinterpret_cast<double*>(take(sR * sn * 8));
  w.tilecum = reinterpret_cast<double*>(take(sR * tiles * 8));
  w.part = reinterpret_cast<double*>(take(sR * kKmMaxT * tiles * 8));
  w.pot = reinterpret_cast<double*>(take(sR * 8));
  w.sumpart = reinterpret_cast<double*>(take(sR * segs * sk * sd * 8));
  w.sq = reinterpret_cast<double*>(take(sR * sk * sd * 8));
  w.colp = reinterpret_cast<double*>(take(col_ws_doubles(n, d) * 8));
  w.colmean = reinterpret_cast<double*>(take(sd * 8));
  w.colvar = reinterpret_cast<double*>(take(sd * 8));
  w.tol_abs = reinterpret_cast<double*>(take(8));
  w.labels = reinterpret_cast<int32_t*>(take(sR * sn * 4));
  w.cntpart = reinterpret_cast<int32_t*>(take(sR * segs * sk * 4));
  w.count = reinterpret_cast<int32_t*>(take(sR * sk * 4));
  w.reloc = reinterpret_cast<int32_t*>(take(sR * sk * 3 * 4));
  w.nreloc = reinterpret_cast<int32_t*>(take(sR * 4));
  w.amax = reinterpret_cast<int32_t*>(take(sR * 4));
  w.nchanged = reinterpret_cast<int32_t*>(take(sR * 4));
  w.cand = reinterpret_cast<int32_t*>(take(sR * kKmMaxT * 4));
  w.chosen = reinterpret_cast<int32_t*>(take(sR * 4));
  w.bytes = off;
  return w;
}

// ---------------------------------------------------------------------------------------------
// k-means++ seeding
// ---------------------------------------------------------------------------------------------
// grid R: centre c of restart r.  c == 0: the given first row.  Else the candidate with the
// smallest potential (its tile partials folded in tile order; first on ties).  Records it, copies
// the row into centers[r][c] and leaves it in chosen[r] for km_seed_update_kernel.
__global__ __launch_bounds__(64) void km_seed_commit_kernel(
    const double* __restrict__ Z, int64_t ldz, int32_t n, int32_t d, int32_t k, int32_t T,
    int32_t c, const int32_t* __restrict__ first, KmWs w, double* __restrict__ centers,
    int32_t* __restrict__ indices) {
  __shared__ double pots[kKmMaxT];
  __shared__ int32_t pick;
  const int tid = threadIdx.x;
  const int32_t r = blockIdx.x;
  const int32_t tiles = (n + kKmTile - 1) / kKmTile;
  if (c == 0) {
    if (tid == 0) pick = first[r];
  } else {
    if (tid < T) {
      const double* pp = w.part + (static_cast<int64_t>(r) * kKmMaxT + tid) * tiles;
      double s = 0.0;
      for (int32_t t = 0; t < tiles; ++t) s += pp[t];
      pots[tid] = s;
    }
    __syncthreads();
    if (tid == 0) {
      int32_t b = 0;
      for (int32_t t = 1; t < T; ++t)
        if (pots[t] < pots[b]) b = t;
      pick = w.cand[r * kKmMaxT + b];
    }
  }
  __syncthreads();
  const int32_t row = pick;
  if (tid == 0) {
    w.chosen[r] = row;
    indices[static_cast<int64_t>(r) * k + c] = row;
  }
  double* out = centers + (static_cast<int64_t>(r) * k + c) * d;
  for (int32_t j = tid; j < d; j += 64) out[j] = Z[static_cast<int64_t>(row) * ldz + j];
}

// grid (tiles, R): closest = min(closest, |z - Z[chosen]|^2) (init: the distance itself), and
// the tile's sum of it, points in order
__global__ __launch_bounds__(kKmBlock) void km_seed_update_kernel(
    const double* __restrict__ Z, int64_t ldz, int32_t n, int32_t d, int init, KmWs w) {
  __shared__ double buf[kKmDistLds];
  const int tid = threadIdx.x;
  const int32_t tile = blockIdx.x, r = blockIdx.y, i0 = tile * kKmTile;
  km_tile_dists(Z, ldz, n, d, i0, Z, ldz, w.chosen + r, 1, buf);
  double* cl = w.closest + static_cast<int64_t>(r) * n;
  if (tid < kKmTile && i0 + tid < n) {
    double v = buf[tid * 65];
    if (!init) {
      const double o = cl[i0 + tid];
      v = o < v ? o : v;
    }
    cl[i0 + tid] = v;
    buf[tid * 65 + 1] = v;
  }
  __syncthreads();
  if (tid == 0) {
    const int32_t m = n - i0 < kKmTile ? n - i0 : kKmTile;
    double s = 0.0;
    for (int32_t p = 0; p < m; ++p) s += buf[p * 65 + 1];
    w.tilecum[static_cast<int64_t>(r) * gridDim.x + tile] = s;
  }
}

// grid R: the tile sums become their inclusive prefix, pot its last entry; trial t's candidate is
// min(searchsorted(cumsum(closest), u pot, side=left), n - 1)
__global__ __launch_bounds__(64) void km_seed_pick_kernel(int32_t n, int32_t k, int32_t T, int32_t c,
                                                          const double* __restrict__ u, KmWs w) {
  const int tid = threadIdx.x;
  const int32_t r = blockIdx.x;
  const int32_t tiles = (n + kKmTile - 1) / kKmTile;
  double* cum = w.tilecum + static_cast<int64_t>(r) * tiles;
  if (tid == 0) {
    double s = 0.0;
    for (int32_t t = 0; t < tiles; ++t) {
      s += cum[t];
      cum[t] = s;
    }
    w.pot[r] = s;
  }
  __syncthreads();
  if (tid < T) {
    const double pot = cum[tiles - 1];
    const double v = u[(static_cast<int64_t>(r) * (k - 1) + (c - 1)) * T + tid] * pot;
    int32_t lo = 0, hi = tiles;                   // the first tile with cum >= v
    while (lo < hi) {
      const int32_t mid = (lo + hi) >> 1;
      if (cum[mid] >= v) hi = mid; else lo = mid + 1;
    }
    int32_t pick = n - 1;
    if (lo < tiles) {
      const double* cl = w.closest + static_cast<int64_t>(r) * n;
      const int32_t i0 = lo * kKmTile;
      const int32_t i1 = i0 + kKmTile < n ? i0 + kKmTile : n;
      double run = lo ? cum[lo - 1] : 0.0;
      pick = i1 - 1;
      for (int32_t i = i0; i < i1; ++i) {
        run += cl[i];
        if (run >= v) {
          pick = i;
          break;
        }
      }
    }
    w.cand[r * kKmMaxT + tid] = pick;
  }
}

// grid (tiles, R): part[r][t][tile] = sum over the tile of min(closest, |z - Z[cand t]|^2)
__global__ __launch_bounds__(kKmBlock) void km_seed_dist_kernel(
    const double* __restrict__ Z, int64_t ldz, int32_t n, int32_t d, int32_t T, KmWs w) {
  __shared__ double buf[kKmDistLds];
  const int tid = threadIdx.x;
  const int32_t tile = blockIdx.x, r = blockIdx.y, i0 = tile * kKmTile;
  km_tile_dists(Z, ldz, n, d, i0, Z, ldz, w.cand + r * kKmMaxT, T, buf);
  if (tid < T) {
    const double* cl = w.closest + static_cast<int64_t>(r) * n;
    const int32_t m = n - i0 < kKmTile ? n - i0 : kKmTile;
    double s = 0.0;
    for (int32_t p = 0; p < m; ++p) {
      const double o = cl[i0 + p], v = buf[p * 65 + tid];
      s += o < v ? o : v;
    }
    w.part[(static_cast<int64_t>(r) * kKmMaxT + tid) * gridDim.x + tile] = s;
  }
}

// ---------------------------------------------------------------------------------------------
// Lloyd's iteration
// ---------------------------------------------------------------------------------------------
// state: done[R] (0 running, 1 labels repeated, 2 tolerance or max_iter), n_iter[R], live
__global__ void km_init_kernel(int32_t n, int32_t R, KmWs w, int32_t* __restrict__ state) {
  const int64_t idx = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (idx < static_cast<int64_t>(R) * n) w.labels[idx] = -1;
  if (idx < R) {
    state[idx] = 0;
    state[R + idx] = 0;
    w.nchanged[idx] = 0;
  }
  if (idx == 0) state[2 * R] = R;
}

// grid (tiles, ceil(R / G)), G <= 64 / k restarts per workgroup (km_group): the centres of the group's
// restarts that take part are stacked into one list of at most 64 rows, so the tile of points is
// read once for all of them and a finished restart costs nothing.  relabel == 0: an iteration's
// labelling (running restarts).  relabel == 1: the labelling against the final centres of every
// restart whose labels did not repeat.  The label is the first lowest distance; closest keeps it.
__global__ __launch_bounds__(kKmBlock) void km_assign_kernel(
    const double* __restrict__ Z, int64_t ldz, int32_t n, int32_t d, int32_t k, int32_t R, int32_t G,
    const double* __restrict__ centers, int relabel, KmWs w, const int32_t* __restrict__ state) {
  __shared__ double buf[kKmDistLds];
  __shared__ int32_t rows[64];                    // stacked row -> row of centers [R * k][d]
  __shared__ int32_t live[64], nch[64];
  __shared__ int32_t nl_s;
  const int tid = threadIdx.x;
  const int32_t tile = blockIdx.x, r0 = blockIdx.y * G, i0 = tile * kKmTile;
  const int32_t nr = R - r0 < G ? R - r0 : G;
  if (tid == 0) {
    int32_t nl = 0;
    for (int32_t rr = 0; rr < nr; ++rr) {
      const int32_t dn = state[r0 + rr];
      if (relabel ? dn != 1 : dn == 0) {
        for (int32_t c = 0; c < k; ++c) rows[nl * k + c] = (r0 + rr) * k + c;
        nch[nl] = 0;
        live[nl++] = r0 + rr;
      }
    }
    nl_s = nl;
  }
  __syncthreads();
  const int32_t nl = nl_s;
  if (nl == 0) return;
  km_tile_dists(Z, ldz, n, d, i0, centers, d, rows, nl * k, buf);
  const int p = tid & 63;
  if (i0 + p < n) {
    for (int32_t j = tid >> 6; j < nl; j += kKmBlock / 64) {
      const double* row = buf + p * 65 + j * k;
      int32_t b = 0;
      double bd = row[0];
      for (int32_t c = 1; c < k; ++c) {
        const double v = row[c];
        if (v < bd) {
          bd = v;
          b = c;
        }
      }
      const int64_t o = static_cast<int64_t>(live[j]) * n + i0 + p;
      if (w.labels[o] != b) atomicAdd(&nch[j], 1);
      w.labels[o] = b;
      w.closest[o] = bd;
    }
  }
  __syncthreads();
  if (!relabel && tid < nl && nch[tid]) atomicAdd(w.nchanged + live[tid], nch[tid]);
}

// grid (ceil(d / 64), segs, R), one wave: the segment's per-cluster sums of 64 columns, points in
// order, each thread its own column: in registers up to kKmRegK clusters, above that in its own
// LDS column (no conflict, no atomic); both add the same values in the same order.  The first
// column block counts.
__global__ __launch_bounds__(64) void km_accumulate_kernel(
    const double* __restrict__ Z, int64_t ldz, int32_t n, int32_t d, int32_t k, KmWs w,
    const int32_t* __restrict__ state) {
  __shared__ double acc[kKmMaxK][64];
  const int tid = threadIdx.x;
  const int32_t seg = blockIdx.y, r = blockIdx.z, segs = gridDim.y;
  if (state[r] != 0) return;
  const int32_t col = blockIdx.x * 64 + tid;
  const int32_t i0 = seg * kKmSeg, i1 = i0 + kKmSeg < n ? i0 + kKmSeg : n;
  const int32_t* lab = w.labels + static_cast<int64_t>(r) * n;
  double* out = w.sumpart + (static_cast<int64_t>(r) * segs + seg) * k * d;
  if (k <= kKmRegK) {
    // few clusters: their sums live in registers, one select per cluster and point
    if (col < d) {
      double a[kKmRegK];
#pragma unroll
      for (int c = 0; c < kKmRegK; ++c) a[c] = 0.0;
      int32_t i = i0;
      for (; i + 8 <= i1; i += 8) {               // eight rows' loads in flight, added in order
        double z[8];
        int32_t l[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          z[q] = Z[static_cast<int64_t>(i + q) * ldz + col];
          l[q] = lab[i + q];
        }
#pragma unroll
        for (int q = 0; q < 8; ++q) {
#pragma unroll
          for (int c = 0; c < kKmRegK; ++c) a[c] = l[q] == c ? a[c] + z[q] : a[c];
        }
      }
      for (; i < i1; ++i) {
        const double z = Z[static_cast<int64_t>(i) * ldz + col];
        const int32_t l = lab[i];
#pragma unroll
        for (int c = 0; c < kKmRegK; ++c) a[c] = l == c ? a[c] + z : a[c];
      }
#pragma unroll
      for (int c = 0; c < kKmRegK; ++c)
        if (c < k) out[static_cast<int64_t>(c) * d + col] = a[c];
    }
  } else {
    for (int32_t c = 0; c < k; ++c) acc[c][tid] = 0.0;
    if (col < d) {
      int32_t i = i0;
      for (; i + 4 <= i1; i += 4) {
        double z[4];
        int32_t l[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          z[q] = Z[static_cast<int64_t>(i + q) * ldz + col];
          l[q] = lab[i + q];
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[l[q]][tid] += z[q];
      }
      for (; i < i1; ++i) acc[lab[i]][tid] += Z[static_cast<int64_t>(i) * ldz + col];
      for (int32_t c = 0; c < k; ++c) out[static_cast<int64_t>(c) * d + col] = acc[c][tid];
    }
  }
  if (blockIdx.x == 0 && tid < k) {
    int32_t cnt = 0;
    for (int32_t i = i0; i < i1; ++i) cnt += lab[i] == tid;
    w.cntpart[(static_cast<int64_t>(r) * segs + seg) * k + tid] = cnt;
  }
}

// grid R: cluster counts, and scikit-learn's relocation of empty clusters: the empty clusters in
// increasing id take the points farthest from their assigned old centre, farthest first (the
// lower index among equal distances); nothing moves when that largest distance is 0.
__global__ __launch_bounds__(kKmBlock) void km_plan_kernel(int32_t n, int32_t k, int32_t segs, KmWs w,
                                                            const int32_t* __restrict__ state) {
  __shared__ int32_t cnt[kKmMaxK], empty[kKmMaxK], picked[kKmMaxK];
  __shared__ double rv[kKmBlock];
  __shared__ int32_t ri[kKmBlock];
  __shared__ int32_t ne_s;
  const int tid = threadIdx.x;
  const int32_t r = blockIdx.x;
  if (state[r] != 0) return;
  if (tid < k) {
    int32_t c = 0;
    for (int32_t s = 0; s < segs; ++s) c += w.cntpart[(static_cast<int64_t>(r) * segs + s) * k + tid];
    cnt[tid] = c;
  }
  __syncthreads();
  if (tid == 0) {
    int32_t ne = 0;
    for (int32_t c = 0; c < k; ++c)
      if (cnt[c] == 0) empty[ne++] = c;
    ne_s = ne;
  }
  __syncthreads();
  const int32_t ne = ne_s;
  int32_t nrel = 0;
  const double* dist = w.closest + static_cast<int64_t>(r) * n;
  const int32_t* lab = w.labels + static_cast<int64_t>(r) * n;
  for (int32_t j = 0; j < ne; ++j) {
    double bv = -1.0;
    int32_t bi = -1;
    for (int32_t i = tid; i < n; i += kKmBlock) {
      bool taken = false;
      for (int32_t q = 0; q < j; ++q) taken |= picked[q] == i;
      const double v = dist[i];
      if (!taken && v > bv) {
        bv = v;
        bi = i;
      }
    }
    rv[tid] = bv;
    ri[tid] = bi;
    __syncthreads();
    for (int s = kKmBlock / 2; s > 0; s >>= 1) {
      if (tid < s) {
        const double ov = rv[tid + s];
        const int32_t oi = ri[tid + s];
        const bool better = oi >= 0 && (ri[tid] < 0 || ov > rv[tid] || (ov == rv[tid] && oi < ri[tid]));
        if (better) {
          rv[tid] = ov;
          ri[tid] = oi;
        }
      }
      __syncthreads();
    }
    const int32_t f = ri[0];
    const double fv = rv[0];
    __syncthreads();                              // rv / ri are rewritten by the next round
    if (f < 0 || (j == 0 && !(fv > 0.0))) break;  // block-uniform
    if (tid == 0) {
      const int32_t o = lab[f], e = empty[j];
      picked[j] = f;
      int32_t* rel = w.reloc + (static_cast<int64_t>(r) * k + j) * 3;
      rel[0] = e;
      rel[1] = f;
      rel[2] = o;
      cnt[e] = 1;
      cnt[o] -= 1;
    }
    nrel = j + 1;
    __syncthreads();
  }
  __syncthreads();
  if (tid < k) w.count[r * k + tid] = cnt[tid];
  if (tid == 0) {
    int32_t a = 0;
    for (int32_t c = 1; c < k; ++c)
      if (cnt[c] > cnt[a]) a = c;
    w.amax[r] = a;
    w.nreloc[r] = nrel;
  }
}

// grid (ceil(d / 64), R), one wave: the new centres of 64 columns.  Sums folded in segment order,
// relocations applied in their order, then scikit-learn's averaging: sum * (1 / count), and a
// cluster still empty takes the first largest cluster's row as it stands at that point.
__global__ __launch_bounds__(64) void km_centres_kernel(
    const double* __restrict__ Z, int64_t ldz, int32_t d, int32_t k, int32_t segs, KmWs w,
    double* __restrict__ centers, const int32_t* __restrict__ state) {
  __shared__ double sums[kKmMaxK][64];
  const int tid = threadIdx.x;
  const int32_t r = blockIdx.y;
  if (state[r] != 0) return;
  const int32_t col = blockIdx.x * 64 + tid;
  if (col >= d) return;                           // no barrier below: each thread its own column
  for (int32_t c = 0; c < k; ++c) {
    double s = 0.0;
    for (int32_t g = 0; g < segs; ++g)
      s += w.sumpart[((static_cast<int64_t>(r) * segs + g) * k + c) * d + col];
    sums[c][tid] = s;
  }
  const int32_t nrel = w.nreloc[r];
  for (int32_t j = 0; j < nrel; ++j) {
    const int32_t* rel = w.reloc + (static_cast<int64_t>(r) * k + j) * 3;
    const double zf = Z[static_cast<int64_t>(rel[1]) * ldz + col];
    sums[rel[2]][tid] -= zf;
    sums[rel[0]][tid] = zf;
  }
  const int32_t amax = w.amax[r];
  for (int32_t c = 0; c < k; ++c) {
    const int32_t cn = w.count[r * k + c];
    if (cn > 0) {
      const double alpha = 1.0 / static_cast<double>(cn);
      sums[c][tid] *= alpha;
    } else {
      sums[c][tid] = sums[amax][tid];
    }
  }
  for (int32_t c = 0; c < k; ++c) {
    const int64_t o = (static_cast<int64_t>(r) * k + c) * d + col;
    const double nw = sums[c][tid], df = nw - centers[o];
    centers[o] = nw;
    w.sq[o] = df * df;
  }
}

// grid R: shift = sum_c sqrt(|new_c - old_c|^2)^2 and the restart's exit
__global__ __launch_bounds__(kKmBlock) void km_decide_kernel(int32_t d, int32_t k, int32_t R,
                                                              int32_t max_iter, KmWs w,
                                                              int32_t* __restrict__ state) {
  __shared__ double red[kKmBlock];
  const int tid = threadIdx.x;
  const int32_t r = blockIdx.x;
  if (state[r] != 0) return;
  double tot = 0.0;                               // thread 0's
  for (int32_t c = 0; c < k; ++c) {
    const double* q = w.sq + (static_cast<int64_t>(r) * k + c) * d;
    double s = 0.0;
    for (int32_t j = tid; j < d; j += kKmBlock) s += q[j];
    red[tid] = s;
    __syncthreads();
    for (int st = kKmBlock / 2; st > 0; st >>= 1) {
      if (tid < st) red[tid] += red[tid + st];
      __syncthreads();
    }
    if (tid == 0) {
      const double e = sqrt(red[0]);
      tot += e * e;
    }
    __syncthreads();
  }
  if (tid == 0) {
    const int32_t it = state[R + r] + 1;
    state[R + r] = it;
    const int32_t changed = w.nchanged[r];
    w.nchanged[r] = 0;
    int32_t dn = 0;
    if (changed == 0) dn = 1;
    else if (tot <= *w.tol_abs || it >= max_iter) dn = 2;
    if (dn) {
      state[r] = dn;
      atomicSub(state + 2 * R, 1);
    }
  }
}

// ---------------------------------------------------------------------------------------------
// finish
// ---------------------------------------------------------------------------------------------
// grid (tiles, R): the tile's sum of |z_i - c_label(i)|^2 against the final centres
__global__ __launch_bounds__(kKmBlock) void km_inertia_kernel(
    const double* __restrict__ Z, int64_t ldz, int32_t n, int32_t d, int32_t k,
    const double* __restrict__ centers, KmWs w) {
  __shared__ double buf[kKmDistLds];
  const int tid = threadIdx.x;
  const int32_t tile = blockIdx.x, r = blockIdx.y, i0 = tile * kKmTile;
  km_tile_dists(Z, ldz, n, d, i0, centers + static_cast<int64_t>(r) * k * d, d, nullptr, k, buf);
  if (tid == 0) {
    const int32_t* lab = w.labels + static_cast<int64_t>(r) * n;
    const int32_t m = n - i0 < kKmTile ? n - i0 : kKmTile;
    double s = 0.0;
    for (int32_t p = 0; p < m; ++p) s += buf[p * 65 + lab[i0 + p]];
    w.part[(static_cast<int64_t>(r) * kKmMaxT) * gridDim.x + tile] = s;
  }
}

// grid G (one workgroup per group of n_init restarts): inertia per restart, then scikit-learn's
// sequential choice: restart r replaces the incumbent if its inertia is lower and its labels are
// not the incumbent's partition renamed (its one-directional mapping test)
constexpr int kKmSelBlock = 1024;
__global__ __launch_bounds__(kKmSelBlock) void km_select_kernel(
    int32_t n, int32_t d, int32_t k, int32_t R, int32_t n_init, const double* __restrict__ centers,
    const double* __restrict__ mean, KmWs w, const int32_t* __restrict__ state,
    int32_t* __restrict__ out_best, int32_t* __restrict__ out_labels,
    double* __restrict__ out_centers, double* __restrict__ out_inertia,
    int32_t* __restrict__ out_n_iter) {
  __shared__ double inert[kKmMaxR];
  __shared__ int32_t map[kKmMaxK];
  const int tid = threadIdx.x;
  const int32_t g = blockIdx.x, r0 = g * n_init;
  const int32_t tiles = (n + kKmTile - 1) / kKmTile;
  if (tid < n_init) {
    const double* pp = w.part + (static_cast<int64_t>(r0 + tid) * kKmMaxT) * tiles;
    double s = 0.0;
    for (int32_t t = 0; t < tiles; ++t) s += pp[t];
    inert[tid] = s;
    out_inertia[r0 + tid] = s;
    out_n_iter[r0 + tid] = state[R + r0 + tid];
  }
  __syncthreads();
  int32_t best = 0;                               // block-uniform
  for (int32_t q = 1; q < n_init; ++q) {
    if (!(inert[q] < inert[best])) continue;
    const int32_t* l1 = w.labels + static_cast<int64_t>(r0 + q) * n;
    const int32_t* l2 = w.labels + static_cast<int64_t>(r0 + best) * n;
    if (tid < k) map[tid] = 0x7fffffff;
    __syncthreads();
    for (int32_t i = tid; i < n; i += kKmSelBlock) atomicMin(&map[l1[i]], i);
    __syncthreads();
    int differs = 0;
    for (int32_t i = tid; i < n; i += kKmSelBlock) differs |= l2[i] != l2[map[l1[i]]];
    if (__syncthreads_or(differs)) best = q;
  }
  if (tid == 0) out_best[g] = best;
  const int32_t* lb = w.labels + static_cast<int64_t>(r0 + best) * n;
  for (int32_t i = tid; i < n; i += kKmSelBlock) out_labels[static_cast<int64_t>(g) * n + i] = lb[i];
  const double* cb = centers + static_cast<int64_t>(r0 + best) * k * d;
  for (int32_t idx = tid; idx < k * d; idx += kKmSelBlock)
    out_centers[static_cast<int64_t>(g) * k * d + idx] = cb[idx] + (mean ? mean[idx % d] : 0.0);
}

// ---------------------------------------------------------------------------------------------
// nearest rows
// ---------------------------------------------------------------------------------------------
// grid (tiles of X, ceil(q / 64)): per query the tile's first lowest squared distance
__global__ __launch_bounds__(kKmBlock) void km_nearest_tile_kernel(
    const double* __restrict__ Q, int64_t ldq, int32_t q, const double* __restrict__ X, int64_t ldx,
    int32_t n, int32_t d, double* __restrict__ pd, int32_t* __restrict__ pi) {
  __shared__ double buf[kKmDistLds];
  const int tid = threadIdx.x;
  const int32_t tile = blockIdx.x, q0 = blockIdx.y * 64, i0 = tile * kKmTile;
  const int32_t nq = q - q0 < 64 ? q - q0 : 64;
  km_tile_dists(X, ldx, n, d, i0, Q + static_cast<int64_t>(q0) * ldq, ldq, nullptr, nq, buf);
  if (tid < nq) {
    const int32_t m = n - i0 < kKmTile ? n - i0 : kKmTile;
    double bd = buf[tid];
    int32_t b = 0;
    for (int32_t p = 1; p < m; ++p) {
      const double v = buf[p * 65 + tid];
      if (v < bd) {
        bd = v;
        b = p;
      }
    }
    const int64_t o = static_cast<int64_t>(q0 + tid) * gridDim.x + tile;
    pd[o] = bd;
    pi[o] = i0 + b;
  }
}

__global__ void km_nearest_fold_kernel(int32_t q, int32_t tiles, const double* __restrict__ pd,
                                       const int32_t* __restrict__ pi, int32_t* __restrict__ out_idx,
                                       double* __restrict__ out_dist) {
  const int32_t c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= q) return;
  double bd = pd[static_cast<int64_t>(c) * tiles];
  int32_t b = pi[static_cast<int64_t>(c) * tiles];
  for (int32_t t = 1; t < tiles; ++t) {
    const double v = pd[static_cast<int64_t>(c) * tiles + t];
    if (v < bd) {
      bd = v;
      b = pi[static_cast<int64_t>(c) * tiles + t];
    }
  }
  out_idx[c] = b;
  out_dist[c] = sqrt(bd);
}

// ---------------------------------------------------------------------------------------------
// argument checks
// ---------------------------------------------------------------------------------------------
int check_matrix(const std::string& w, const char* name, const void* p, int64_t ld, int32_t d) {
  if (!p) return fail(CS_ERR_INVALID, w + name + " is NULL");
  if (misaligned(p, 8)) return fail(CS_ERR_INVALID, w + name + " must be 8-byte aligned");
  if (ld < d) return fail(CS_ERR_INVALID, w + "leading dimension of " + name + " below d");
  return CS_OK;
}

int check_km_dims(const std::string& w, int32_t n, int32_t d, int32_t k, int32_t R) {
  if (n < 1 || n > kKmMaxN) return fail(CS_ERR_INVALID, w + "need 1 <= n <= 2^20");
  if (d < 1 || d > kKmMaxD) return fail(CS_ERR_INVALID, w + "need 1 <= d <= 4096");
  if (k < 1 || k > kKmMaxK) return fail(CS_ERR_INVALID, w + "need 1 <= k <= 64");
  if (k > n) return fail(CS_ERR_INVALID, w + "need k <= n");
  if (R < 1 || R > kKmMaxR) return fail(CS_ERR_INVALID, w + "need 1 <= R <= 1024");
  return CS_OK;
}

}  // namespace

extern "C" {

size_t cs_standardize_workspace_size(int32_t n, int32_t d) {
  if (n < 1 || d < 1 || n > kKmMaxN || d > kKmMaxD) return 0;
  return col_ws_doubles(n, d) * 8;
}

int cs_standardize(const double* X, int64_t ldx, int32_t n, int32_t d, double* Z, int64_t ldz,
                   double* mean, double* scale, void* workspace, size_t workspace_bytes,
                   cs_stream_t stream) {
  const std::string w = "cs_standardize: ";
  if (n < 1 || n > kKmMaxN) return fail(CS_ERR_INVALID, w + "need 1 <= n <= 2^20");
  if (d < 1 || d > kKmMaxD) return fail(CS_ERR_INVALID, w + "need 1 <= d <= 4096");
  if (int rc = check_matrix(w, "X", X, ldx, d)) return rc;
  if (int rc = check_matrix(w, "Z", Z, ldz, d)) return rc;
  if (!mean || !scale || misaligned(mean, 8) || misaligned(scale, 8))
    return fail(CS_ERR_INVALID, w + "mean and scale must be 8-byte aligned and not NULL");
  if (int rc = check_workspace("cs_standardize", workspace, workspace_bytes,
                               cs_standardize_workspace_size(n, d)))
    return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  double* p1 = static_cast<double*>(workspace);
  double* p2 = p1 + col_ws_doubles(n, d) / 2;
  launch_col_stats(st, X, ldx, n, d, p1, p2, mean, 2, scale);
  const int64_t total = static_cast<int64_t>(n) * d;
  hipLaunchKernelGGL(km_standardize_kernel, dim3(static_cast<uint32_t>(cdiv(total, 256))), dim3(256),
                     0, st, X, ldx, n, d, static_cast<const double*>(mean),
                     static_cast<const double*>(scale), Z, ldz);
  return check_launch("cs_standardize");
}

size_t cs_kmeans_workspace_size(int32_t n, int32_t d, int32_t k, int32_t R) {
  if (n < 1 || d < 1 || k < 1 || R < 1 || n > kKmMaxN || d > kKmMaxD || k > kKmMaxK || R > kKmMaxR)
    return 0;
  return km_layout(nullptr, n, d, k, R).bytes;
}

int cs_kmeans_seed(const double* Z, int64_t ldz, int32_t n, int32_t d, int32_t k, int32_t R,
                   int32_t T, const int32_t* first_host, const double* u_host, const int32_t* first,
                   const double* u, double* centers, int32_t* indices, void* workspace,
                   size_t workspace_bytes, cs_stream_t stream) {
  const std::string w = "cs_kmeans_seed: ";
  if (int rc = check_km_dims(w, n, d, k, R)) return rc;
  if (T < 1 || T > kKmMaxT) return fail(CS_ERR_INVALID, w + "need 1 <= T <= 8");
  if (int rc = check_matrix(w, "Z", Z, ldz, d)) return rc;
  if (!first_host || !first || !centers || !indices || (k > 1 && (!u_host || !u)))
    return fail(CS_ERR_INVALID, w + "NULL pointer");
  if (misaligned(first, 4) || misaligned(indices, 4) || misaligned(u, 8) || misaligned(centers, 8))
    return fail(CS_ERR_INVALID, w + "first, indices 4-byte and u, centers 8-byte aligned");
  for (int32_t r = 0; r < R; ++r)
    if (first_host[r] < 0 || first_host[r] >= n)
      return fail(CS_ERR_INVALID, w + "first outside [0, n)");
  const int64_t nu = static_cast<int64_t>(R) * (k - 1) * T;
  for (int64_t i = 0; i < nu; ++i)
    if (!(u_host[i] >= 0.0 && u_host[i] < 1.0)) return fail(CS_ERR_INVALID, w + "u outside [0, 1)");
  if (int rc = check_workspace("cs_kmeans_seed", workspace, workspace_bytes,
                               cs_kmeans_workspace_size(n, d, k, R), 16))
    return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const KmWs ws = km_layout(workspace, n, d, k, R);
  const uint32_t tiles = static_cast<uint32_t>(cdiv(n, kKmTile));
  const dim3 tgrid(tiles, static_cast<uint32_t>(R));
  for (int32_t c = 0; c < k; ++c) {
    if (c > 0) {
      hipLaunchKernelGGL(km_seed_pick_kernel, dim3(R), dim3(64), 0, st, n, k, T, c, u, ws);
      hipLaunchKernelGGL(km_seed_dist_kernel, tgrid, dim3(kKmBlock), 0, st, Z, ldz, n, d, T, ws);
    }
    hipLaunchKernelGGL(km_seed_commit_kernel, dim3(R), dim3(64), 0, st, Z, ldz, n, d, k, T, c, first,
                       ws, centers, indices);
    if (c + 1 < k)
      hipLaunchKernelGGL(km_seed_update_kernel, tgrid, dim3(kKmBlock), 0, st, Z, ldz, n, d,
                         c == 0 ? 1 : 0, ws);
  }
  return check_launch("cs_kmeans_seed");
}

int cs_kmeans_init(const double* Z, int64_t ldz, int32_t n, int32_t d, int32_t k, int32_t R,
                   double tol, int32_t* state, void* workspace, size_t workspace_bytes,
                   cs_stream_t stream) {
  const std::string w = "cs_kmeans_init: ";
  if (int rc = check_km_dims(w, n, d, k, R)) return rc;
  if (!(tol >= 0.0) || std::isinf(tol)) return fail(CS_ERR_INVALID, w + "tol must be finite and >= 0");
  if (int rc = check_matrix(w, "Z", Z, ldz, d)) return rc;
  if (!state || misaligned(state, 4)) return fail(CS_ERR_INVALID, w + "state NULL or misaligned");
  if (int rc = check_workspace("cs_kmeans_init", workspace, workspace_bytes,
                               cs_kmeans_workspace_size(n, d, k, R), 16))
    return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const KmWs ws = km_layout(workspace, n, d, k, R);
  const int64_t total = static_cast<int64_t>(R) * n;
  hipLaunchKernelGGL(km_init_kernel, dim3(static_cast<uint32_t>(cdiv(total, 256))), dim3(256), 0, st,
                     n, R, ws, state);
  launch_col_stats(st, Z, ldz, n, d, ws.colp, ws.colp + col_ws_doubles(n, d) / 2, ws.colmean, 1,
                   ws.colvar);
  hipLaunchKernelGGL(km_tol_kernel, dim3(1), dim3(64), 0, st, static_cast<const double*>(ws.colvar),
                     d, tol, ws.tol_abs);
  return check_launch("cs_kmeans_init");
}

int cs_kmeans_iterate(const double* Z, int64_t ldz, int32_t n, int32_t d, int32_t k, int32_t R,
                      double* centers, int32_t* state, int32_t n_steps, int32_t max_iter,
                      void* workspace, size_t workspace_bytes, cs_stream_t stream) {
  const std::string w = "cs_kmeans_iterate: ";
  if (int rc = check_km_dims(w, n, d, k, R)) return rc;
  if (n_steps < 0 || n_steps > 65536) return fail(CS_ERR_INVALID, w + "need 0 <= n_steps <= 65536");
  if (max_iter < 1) return fail(CS_ERR_INVALID, w + "need max_iter >= 1");
  if (int rc = check_matrix(w, "Z", Z, ldz, d)) return rc;
  if (!centers || misaligned(centers, 8)) return fail(CS_ERR_INVALID, w + "centers NULL or misaligned");
  if (!state || misaligned(state, 4)) return fail(CS_ERR_INVALID, w + "state NULL or misaligned");
  if (int rc = check_workspace("cs_kmeans_iterate", workspace, workspace_bytes,
                               cs_kmeans_workspace_size(n, d, k, R), 16))
    return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const KmWs ws = km_layout(workspace, n, d, k, R);
  const uint32_t tiles = static_cast<uint32_t>(cdiv(n, kKmTile));
  const uint32_t segs = static_cast<uint32_t>(cdiv(n, kKmSeg));
  const uint32_t dblocks = static_cast<uint32_t>(cdiv(d, 64));
  const uint32_t uR = static_cast<uint32_t>(R);
  const int32_t G = km_group(n, k, R);
  const uint32_t groups = static_cast<uint32_t>(cdiv(R, G));
  for (int32_t s = 0; s < n_steps; ++s) {
    hipLaunchKernelGGL(km_assign_kernel, dim3(tiles, groups), dim3(kKmBlock), 0, st, Z, ldz, n, d, k,
                       R, G, static_cast<const double*>(centers), 0, ws,
                       static_cast<const int32_t*>(state));
    hipLaunchKernelGGL(km_accumulate_kernel, dim3(dblocks, segs, uR), dim3(64), 0, st, Z, ldz, n, d,
                       k, ws, static_cast<const int32_t*>(state));
    hipLaunchKernelGGL(km_plan_kernel, dim3(uR), dim3(kKmBlock), 0, st, n, k,
                       static_cast<int32_t>(segs), ws, static_cast<const int32_t*>(state));
    hipLaunchKernelGGL(km_centres_kernel, dim3(dblocks, uR), dim3(64), 0, st, Z, ldz, d, k,
                       static_cast<int32_t>(segs), ws, centers, static_cast<const int32_t*>(state));
    hipLaunchKernelGGL(km_decide_kernel, dim3(uR), dim3(kKmBlock), 0, st, d, k, R, max_iter, ws,
                       state);
  }
  return check_launch("cs_kmeans_iterate");
}

int cs_kmeans_finish(const double* Z, int64_t ldz, int32_t n, int32_t d, int32_t k, int32_t R,
                     int32_t n_init, const double* centers, const double* mean, const int32_t* state,
                     int32_t* out_best, int32_t* out_labels, double* out_centers, double* out_inertia,
                     int32_t* out_n_iter, void* workspace, size_t workspace_bytes,
                     cs_stream_t stream) {
  const std::string w = "cs_kmeans_finish: ";
  if (int rc = check_km_dims(w, n, d, k, R)) return rc;
  if (n_init < 1 || R % n_init != 0)
    return fail(CS_ERR_INVALID, w + "R must be a multiple of n_init >= 1");
  if (int rc = check_matrix(w, "Z", Z, ldz, d)) return rc;
  if (!centers || !state || !out_best || !out_labels || !out_centers || !out_inertia || !out_n_iter)
    return fail(CS_ERR_INVALID, w + "NULL pointer");
  if (misaligned(centers, 8) || misaligned(mean, 8) || misaligned(out_centers, 8) ||
      misaligned(out_inertia, 8) || misaligned(state, 4) || misaligned(out_best, 4) ||
      misaligned(out_labels, 4) || misaligned(out_n_iter, 4))
    return fail(CS_ERR_INVALID, w + "doubles 8-byte, int32 4-byte aligned");
  if (int rc = check_workspace("cs_kmeans_finish", workspace, workspace_bytes,
                               cs_kmeans_workspace_size(n, d, k, R), 16))
    return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const KmWs ws = km_layout(workspace, n, d, k, R);
  const uint32_t tiles = static_cast<uint32_t>(cdiv(n, kKmTile));
  const dim3 tgrid(tiles, static_cast<uint32_t>(R));
  const int32_t G = km_group(n, k, R);
  hipLaunchKernelGGL(km_assign_kernel, dim3(tiles, static_cast<uint32_t>(cdiv(R, G))), dim3(kKmBlock),
                     0, st, Z, ldz, n, d, k, R, G, centers, 1, ws, state);
  hipLaunchKernelGGL(km_inertia_kernel, tgrid, dim3(kKmBlock), 0, st, Z, ldz, n, d, k, centers, ws);
  hipLaunchKernelGGL(km_select_kernel, dim3(static_cast<uint32_t>(R / n_init)), dim3(kKmSelBlock), 0,
                     st, n, d, k, R, n_init, centers, mean, ws, state, out_best, out_labels,
                     out_centers, out_inertia, out_n_iter);
  return check_launch("cs_kmeans_finish");
}

size_t cs_nearest_rows_workspace_size(int32_t q, int32_t n) {
  if (q < 1 || n < 1 || n > kKmMaxN) return 0;
  const size_t tiles = cdiv(n, kKmTile);
  return up16(static_cast<size_t>(q) * tiles * 8) + up16(static_cast<size_t>(q) * tiles * 4);
}

int cs_nearest_rows(const double* Q, int64_t ldq, int32_t q, const double* X, int64_t ldx, int32_t n,
                    int32_t d, int32_t* out_index, double* out_dist, void* workspace,
                    size_t workspace_bytes, cs_stream_t stream) {
  const std::string w = "cs_nearest_rows: ";
  if (q < 1 || q > kKmMaxN) return fail(CS_ERR_INVALID, w + "need 1 <= q <= 2^20");
  if (n < 1 || n > kKmMaxN) return fail(CS_ERR_INVALID, w + "need 1 <= n <= 2^20");
  if (d < 1 || d > kKmMaxD) return fail(CS_ERR_INVALID, w + "need 1 <= d <= 4096");
  if (int rc = check_matrix(w, "Q", Q, ldq, d)) return rc;
  if (int rc = check_matrix(w, "X", X, ldx, d)) return rc;
  if (!out_index || !out_dist || misaligned(out_index, 4) || misaligned(out_dist, 8))
    return fail(CS_ERR_INVALID, w + "out_index / out_dist NULL or misaligned");
  if (int rc = check_workspace("cs_nearest_rows", workspace, workspace_bytes,
                               cs_nearest_rows_workspace_size(q, n), 16))
    return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const uint32_t tiles = static_cast<uint32_t>(cdiv(n, kKmTile));
  double* pd = static_cast<double*>(workspace);
  int32_t* pi = reinterpret_cast<int32_t*>(static_cast<char*>(workspace) +
                                           up16(static_cast<size_t>(q) * tiles * 8));
  hipLaunchKernelGGL(km_nearest_tile_kernel, dim3(tiles, static_cast<uint32_t>(cdiv(q, 64))),
                     dim3(kKmBlock), 0, st, Q, ldq, q, X, ldx, n, d, pd, pi);
  hipLaunchKernelGGL(km_nearest_fold_kernel, dim3(static_cast<uint32_t>(cdiv(q, 256))), dim3(256), 0,
                     st, q, static_cast<int32_t>(tiles), static_cast<const double*>(pd),
                     static_cast<const int32_t*>(pi), out_index, out_dist);
  return check_launch("cs_nearest_rows");
}

}  // extern "C"
