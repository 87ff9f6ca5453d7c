// attn.hip — the transformer side of the batched agent x candidate decode:
//
//   prefix_attn_*_kernel cascade attention over SHARED per-agent prefix K/V.  Every
//                        candidate stream of an agent (a beam, a Best-of-N candidate) reads
//                        its agent's prefix keys through one workgroup that holds ALL of
//                        that agent's query rows of one K/V head, so a prefix key block is
//                        fetched from HBM once per (agent, head), not once per stream (the
//                        reference re-encodes the whole ~150-800-token prompt per call:
//                        src/utils.py:249-259, driven per candidate at
//                        src/methods/beam_search.py:495-538, best_of_n.py:266-321).  Each
//                        stream's own tokens (history + causal self) live in a per-stream
//                        buffer and are attended in the same pass.  bf16 MFMA
//                        (v_mfma_f32_16x16x32_bf16), fp32 online softmax.
//                        Two kernels, built from one set of pieces (each written once, below):
//                        tile_rows / hist_blocks (who a lane is, which history blocks its rows
//                        see), block_mask / prefix_block / hist_block (where a key block lives
//                        and what of it a row may see), load_q, attend_block (the arithmetic),
//                        fetch_chunks / stage_chunks / attend_staged under CS_ATTEND_STAGED
//                        (key blocks staged through LDS, double-buffered), combine_waves,
//                        store_out.  prefix_attn_lds_kernel stages every block of the
//                        workgroup's list; prefix_attn_plan_lds_kernel stages its split's
//                        prefix blocks and loads its tiles' history per wave.
//                        prefix_attn_wide_kernel (described where it stands) is the no-plan
//                        kernel's second form for scoring chunks and prefill at D = 128: 32
//                        query rows per wave over 64-key blocks (v_mfma_f32_32x32x16_bf16).
//   attn_merge_kernel    fixed-order merge of the key splits (no float atomics).
//   rope_place_kernel    RoPE on the fused q|k|v projection + placement of the new K (row
//                        layout) and V (transposed layout) into the per-stream buffers;
//                        positions come from device memory (prefix length + history base),
//                        so a captured decode step replays with no host input but ids.
//   encoder_attn_kernel  bidirectional attention of the text encoder over a ragged batch, from
//                        the same pieces (described where it stands, at the end of the file).
//
// Layouts (all bf16, D = head_dim in {64, 128, 256}):
//   q       [n_tok, H, D], token tok = s*T + t of stream s = grp*n_str + b
//   k_pfx   [Hkv, Lp, D]                vt_pfx [Hkv, Lp/32, D, 32] (ragged prefixes: prefix p's
//           keys are rows off[p] .. off[p] + len[p], off[p] % 32 == 0, padded to 32 keys)
//   k_hist  [S, Hkv, ldh, D]            vt_hist [S, Hkv, ldh/32, D, 32]  (ldh % 32 == 0)
// V is stored TRANSPOSED IN 32-KEY TILES: the tile of keys 32c .. 32c+31 is D rows of 32
// keys, contiguous (64 B per row): a key block's V^T is one 2-16 KB span, read as 16 rows
// of 64 B per load instruction (a plain [D][keys] transpose puts the rows a whole key axis
// apart — tens of KB — and the scattered 64-byte reads ran 10x below the HBM rate).
//   out     [n_tok, H, D]
// Query token t of stream s sees prefix keys [0, plen[pfx]) and history keys
// [0, hist_base + t] (its own key is history slot hist_base + t).
//
// Operand orientation (MI355X 16x16x32 bf16 maps, cdna_hip_programming.md §3): the score
// tile is computed transposed, S^T = K . Q^T (A = 16 keys x 32 d, B = Q^T), so lane l ends
// with query l&15's scores for keys 4(l>>4)+i of each 16-key tile.  Those scores become the
// B operand of O^T = V^T . P^T for a 32-key block without any lane movement, by ordering the
// k slots as key(h, j) = 16(j>>2) + 4h + (j&3): V^T rows are key-contiguous (hence the
// transposed V layout) and give the matching 2 x 8-byte A fragments.  Every lane keeps ONE
// query column throughout, so the softmax rescale needs no shuffle; the row max needs two
// xor-shuffles across the four lane groups.
#include "cs_kernels.cuh"

#include <algorithm>
#include <vector>

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kAttnThreads = 256;   // 4 waves
constexpr int kGroupRows = 64;      // query rows per workgroup (4 tiles of 16)
constexpr int kKeyBlock = 32;
constexpr int kMaxSplit = 32;       // key splits of one (group, head, query group)
constexpr int kPlanMinBase = 1024;  // from this many (group, head, query group) workgroups on,
                                    // the chip is full without key splits: no plan
constexpr int kMergeRows = 8;       // query rows per merge workgroup (2 per wave)
constexpr float kLazyRescale = 8.0f;   // attend_block's lazy-rescale threshold (log2 units)
constexpr int64_t kPlanImbalance = 4;   // ... or from a longest cell 4x the mean on (T = 1)
constexpr int kPlanTargetWgs = 512;     // plan: split cells until about this many workgroups
constexpr int kPlanMinItems = 3;        // ... but never below this many key blocks per wave

// Work plan entries (int32 x 4, device memory), attention entries first:
//   attention  {pg = group * Hkv + head, query group, split | n_used << 8, partial slot}
//   merge      {pg, query group, first partial slot, row chunk | n_used << 8}
struct AttnParams {
  const __bf16* q;
  const __bf16* kp;
  const __bf16* vtp;
  const int64_t* poff;
  const int32_t* plen;
  const int32_t* gpfx;      // group -> prefix index (nullable: identity)
  const __bf16* kh;
  const __bf16* vth;
  const int32_t* hist_base;
  const int32_t* hrow;      // row-layout history (cs_prefix_attention_rows): [S][ldh] stream
                            // row holding each slot; nullptr: V^T tiles, slot j of stream s in row s
  __bf16* out;
  float* part;              // [slot][kGroupRows][D + 2]: O (unnormalised), m, l
  const int4* plan;         // nullable: one workgroup per (group, head, query group), no split
  int64_t ldp, ldh;
  int32_t n_grp, n_str, T, H, Hkv, rep, n_qg, n_attn;
  float scale, softcap, inv_softcap;
  int32_t window;           // > 0: keys more than window - 1 positions back are masked
  int32_t swizzle;
};


// the workgroup's logical id: consecutive logical ids on one XCD (dispatch is round-robin
// over the 8 XCDs), so the query groups of one (prefix, head) share that XCD's L2
__device__ __forceinline__ int logical_block(int swz) {
  const int b = blockIdx.x;
  if (!swz) return b;
  const int per = gridDim.x >> 3;
  return (b & 7) * per + (b >> 3);
}

// ROWS history V image: the chunk swizzle of key k (even, so 32-byte pairs stay whole; the
// 8 keys of a half-wave's transposed read land in 8 different 8-bank groups)
template <int D>
__device__ __forceinline__ int vimg_swz(int k) {
  return D == 64 ? 2 * ((k >> 1) & 3) : 2 * (k & 7);
}

// One 32-key block's operands for this lane: K rows kb + col and kb + 16 + col (8 bf16 of
// each 32-wide d step), V^T rows (16-row d tiles) of the block's 32-key tile.
template <int D>
struct KeyBlock {
  bf16x8 k0[D / 32], k1[D / 32];
  bf16x4 vlo[D / 16], vhi[D / 16];
};

// This lane's place in a workgroup: the workgroup holds query rows r0 .. r0 + nrows - 1 of
// (group gi, K/V head g) -- row = ((stream b) * T + token t) * rep + head of the K/V head --
// as n_qt tiles of 16; wave w attends tile qt's key blocks ks, ks + kw, ... (kw waves share a
// tile when the workgroup has fewer than four), lane (col, h4) query column col of the tile.
struct TileRows {
  int gi, g;             // group, K/V head
  int M, r0, nrows;      // the (group, head)'s query rows; the workgroup's first row and count
  int n_qt, kw;          // 16-row tiles; waves per tile
  int w, lane, qt, ks;   // wave, lane, the wave's tile and key-block stripe
  bool active;           // ks < kw: the wave has a tile
  int col, h4;           // lane & 15, lane >> 4
  bool vrow;             // active and the lane's row exists
  int t, b;              // the row's token and stream (the last row's when !vrow)
  int64_t tok;           // its q / out token index
  int head;
  int hb, pl;            // *hist_base; the group's prefix length
  int64_t po;            // ... and its first key row in k_pfx / vt_pfx
  int hv;                // history keys the row sees: slots [0, hv)
  int kmin_pos;          // first position inside the row's window (INT32_MIN: no window)
};

// pg = group * Hkv + K/V head, qg = which 64 rows of it
__device__ __forceinline__ TileRows tile_rows(const AttnParams& a, int pg, int qg) {
  TileRows r;
  r.gi = pg / a.Hkv;
  r.g = pg % a.Hkv;
  const int p = a.gpfx ? a.gpfx[r.gi] : r.gi;
  r.M = a.n_str * a.T * a.rep;
  r.r0 = qg * kGroupRows;
  r.nrows = min(kGroupRows, r.M - r.r0);
  r.n_qt = (r.nrows + 15) >> 4;
  r.kw = r.n_qt == 1 ? 4 : (r.n_qt == 2 ? 2 : 1);
  const int tid = threadIdx.x;
  r.w = tid >> 6;
  r.lane = tid & 63;
  r.qt = r.w % r.n_qt;
  r.ks = r.w / r.n_qt;
  r.active = r.ks < r.kw;
  r.col = r.lane & 15;
  r.h4 = r.lane >> 4;

  const int row = r.r0 + r.qt * 16 + r.col;
  r.vrow = r.active && row < r.M;
  const int rr = row < r.M ? row : r.M - 1;
  const int jh = rr % a.rep, bt = rr / a.rep;
  r.t = bt % a.T;
  r.b = bt / a.T;
  r.tok = (static_cast<int64_t>(r.gi) * a.n_str + r.b) * a.T + r.t;
  r.head = r.g * a.rep + jh;
  r.hb = *a.hist_base;
  r.pl = a.plen[p];
  r.po = a.poff[p];
  r.hv = min(r.hb + r.t + 1, static_cast<int>(a.ldh));
  r.kmin_pos = a.window > 0 ? r.pl + r.hb + r.t - a.window + 1 : INT32_MIN;
  return r;
}

// The history key blocks that rows row0 .. row1 of a (group, head) can see (uniform over
// whoever shares the rows: the workgroup's 64, a wave's 16): nbh blocks -- up to the furthest
// query's causal limit hlim -- of each stream the rows touch, b_lo on; n blocks in all.
struct HistBlocks {
  int b_lo, nbh, n, hlim;
};

__device__ __forceinline__ HistBlocks hist_blocks(const AttnParams& a, int hb, int row0, int row1) {
  HistBlocks h;
  h.b_lo = (row0 / a.rep) / a.T;
  const int b_hi = (row1 / a.rep) / a.T;
  const int t_hi = h.b_lo == b_hi ? (row1 / a.rep) % a.T : a.T - 1;
  h.hlim = min(hb + t_hi + 1, static_cast<int>(a.ldh));
  h.nbh = (h.hlim + kKeyBlock - 1) / kKeyBlock;
  h.n = (b_hi - h.b_lo + 1) * h.nbh;
  return h;
}

// what attend_block masks a block's keys by: key kb + j is visible iff kb + j < lim and its
// position pos0 + kb + j >= the row's kmin_pos
struct BlockMask {
  int kb, lim, pos0;
};

// the lane's mask of key block kb of the prefix, or (hist) of stream bb's history: a row that
// does not exist sees nothing, a row of another stream nothing of bb's
__device__ __forceinline__ BlockMask block_mask(const TileRows& tr, int kb, bool hist, int bb) {
  BlockMask k;
  k.kb = kb;
  k.lim = hist ? ((tr.vrow && bb == tr.b) ? tr.hv : 0) : (tr.vrow ? tr.pl : 0);
  k.pos0 = hist ? tr.pl : 0;
  return k;
}

// The K rows and V^T tiles of the prefixes and of the history, read from the kernel arguments
// once per kernel: a block list that picks prefix or history per block would otherwise load
// the pointers it picks between inside its loop (a scalar load and a wait per staged block).
struct KvBase {
  const __bf16 *kp, *vtp, *kh, *vth;
};
__device__ __forceinline__ KvBase kv_base(const AttnParams& a) { return {a.kp, a.vtp, a.kh, a.vth}; }

// where a key block lives (its 32 K rows and its V^T tile, each contiguous) and its mask
struct BlockRef {
  const __bf16* k;
  const __bf16* vt;
  BlockMask mask;
};

// block blk of the group's prefix
template <int D>
__device__ __forceinline__ BlockRef prefix_block(const AttnParams& a, const KvBase& kv, const TileRows& tr,
                                                int blk) {
  BlockRef r;
  r.mask = block_mask(tr, blk * kKeyBlock, false, 0);
  const int64_t k0 = static_cast<int64_t>(tr.g) * a.ldp + tr.po + r.mask.kb;
  r.k = kv.kp + k0 * D;
  r.vt = kv.vtp + k0 * D;
  return r;
}

// history block ih of h's list: block ih % nbh of stream b_lo + ih / nbh (V^T-tile layout;
// the row layout takes the mask alone)
template <int D>
__device__ __forceinline__ BlockRef hist_block(const AttnParams& a, const KvBase& kv, const TileRows& tr,
                                               const HistBlocks& h, int ih) {
  BlockRef r;
  const int bb = h.b_lo + ih / h.nbh;
  r.mask = block_mask(tr, (ih % h.nbh) * kKeyBlock, true, bb);
  const int64_t sh = (static_cast<int64_t>(tr.gi) * a.n_str + bb) * a.Hkv + tr.g;
  const int64_t k0 = sh * a.ldh + r.mask.kb;
  r.k = kv.kh + k0 * D;
  r.vt = kv.vth + k0 * D;
  return r;
}

// a block straight from global memory (the plan kernel's per-wave V^T-tile history): all of
// its loads issued back to back (one memory round trip per block)
template <int D>
__device__ __forceinline__ void load_block(KeyBlock<D>& f, const BlockRef& r, int col, int h4) {
  const __bf16* k = r.k + col * D + 8 * h4;
  const __bf16* v = r.vt + col * kKeyBlock + 4 * h4;
#pragma unroll
  for (int ds = 0; ds < D / 32; ++ds) {
    f.k0[ds] = *reinterpret_cast<const bf16x8*>(k + ds * 32);
    f.k1[ds] = *reinterpret_cast<const bf16x8*>(k + 16 * D + ds * 32);
  }
#pragma unroll
  for (int dt = 0; dt < D / 16; ++dt) {
    f.vlo[dt] = *reinterpret_cast<const bf16x4*>(v + dt * 16 * kKeyBlock);
    f.vhi[dt] = *reinterpret_cast<const bf16x4*>(v + dt * 16 * kKeyBlock + 16);
  }
}

// S^T = K . Q^T for the block's 32 keys, online softmax update, O^T += V^T . P^T
template <int D>
__device__ __forceinline__ void attend_block(const AttnParams& a, const KeyBlock<D>& f,
                                             const BlockMask& r, const bf16x8 (&qf)[D / 32],
                                             int kmin_pos, int h4, f32x4 (&o)[D / 16], float& m,
                                             float& l) {
  f32x4 s0 = {0.f, 0.f, 0.f, 0.f}, s1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int ds = 0; ds < D / 32; ++ds) {
    s0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(f.k0[ds], qf[ds], s0, 0, 0, 0);
    s1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(f.k1[ds], qf[ds], s1, 0, 0, 0);
  }
  float y[8];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    y[i] = s0[i];
    y[4 + i] = s1[i];
  }
  float bm = -INFINITY;
  if constexpr (D <= 128) {
    // the scale into log2 units in one multiply without a soft-cap, and a key k0 + j of the
    // lane's 8 visible iff jlo <= j < jhi: fewer vector instructions per block (the online
    // softmax, not the MFMA, paces these kernels; D = 256 keeps the plain form, whose
    // registers are at the two-waves-per-SIMD limit)
    if (a.softcap > 0.0f) {
#pragma unroll
      for (int i = 0; i < 8; ++i) y[i] = softcap_fn(y[i] * a.scale, a.softcap, a.inv_softcap) * kLog2e;
    } else {
      const float sl2 = a.scale * kLog2e;
#pragma unroll
      for (int i = 0; i < 8; ++i) y[i] *= sl2;
    }
    const int k0 = r.kb + 4 * h4;
    const int jlo = kmin_pos == INT32_MIN ? INT32_MIN : kmin_pos - r.pos0 - k0, jhi = r.lim - k0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int j = (i >> 2) * 16 + (i & 3);
      y[i] = (j < jhi && j >= jlo) ? y[i] : -INFINITY;
      bm = fmaxf(bm, y[i]);
    }
  } else {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int key = r.kb + (i >> 2) * 16 + 4 * h4 + (i & 3);
      float x = y[i] * a.scale;
      if (a.softcap > 0.0f) x = softcap_fn(x, a.softcap, a.inv_softcap);
      x *= kLog2e;
      y[i] = (key < r.lim && r.pos0 + key >= kmin_pos) ? x : -INFINITY;
      bm = fmaxf(bm, y[i]);
    }
  }
  bm = fmaxf(bm, __shfl_xor(bm, 16, 64));
  bm = fmaxf(bm, __shfl_xor(bm, 32, 64));
  // lazy rescale: the running max moves (and l, O are rescaled) only when some query column
  // of the wave sees a block max more than kLazyRescale (log2 units) above its own — until
  // then the stale max stands and p = 2^(s - m) stays <= 2^kLazyRescale (exact in the final
  // O / l, which share it).  Most blocks after the first few skip the rescale's vector work.
  float mn = m;
  if (__ballot(bm > m + kLazyRescale) != 0) {   // wave-uniform
    mn = fmaxf(m, bm);
    const float alpha = mn == -INFINITY ? 1.0f : __builtin_amdgcn_exp2f(m - mn);
    l *= alpha;
#pragma unroll
    for (int dt = 0; dt < D / 16; ++dt) o[dt] *= alpha;
  }
  const bool none = mn == -INFINITY;
  float ps = 0.0f;
  bf16x8 pb;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const float pv = none ? 0.0f : __builtin_amdgcn_exp2f(y[i] - mn);
    ps += pv;
    pb[i] = static_cast<__bf16>(pv);
  }
  l += ps;
  m = mn;
#pragma unroll
  for (int dt = 0; dt < D / 16; ++dt) {
    const bf16x8 va = {f.vlo[dt][0], f.vlo[dt][1], f.vlo[dt][2], f.vlo[dt][3],
                       f.vhi[dt][0], f.vhi[dt][1], f.vhi[dt][2], f.vhi[dt][3]};
    o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(va, pb, o[dt], 0, 0, 0);
  }
}

// the lane's Q fragments (its row's 8 d of each 32-wide d step); zeros for a row that does
// not exist
template <int D>
__device__ __forceinline__ void load_q(const AttnParams& a, const TileRows& tr, bf16x8 (&qf)[D / 32]) {
  const __bf16* qrow = a.q + (tr.tok * a.H + tr.head) * D + 8 * tr.h4;
#pragma unroll
  for (int ds = 0; ds < D / 32; ++ds) {
    if (tr.vrow) {
      qf[ds] = *reinterpret_cast<const bf16x8*>(qrow + ds * 32);
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) qf[ds][e] = static_cast<__bf16>(0.0f);
    }
  }
}

// A key block staged through LDS once per workgroup: K rows padded to D + 8, V^T rows to 40
// keys (conflict-free fragment reads), two buffers.  The same LDS holds the wave combine
// (combine_waves: three waves' O, m, l of 16 rows) once the key blocks are done.
template <int D>
struct LdsTile {
  static constexpr int KROW = D + 8;                 // bf16 per staged K row
  static constexpr int VROW = 40;                    // bf16 per staged V^T row (32 keys + pad)
  static constexpr int KELEMS = kKeyBlock * KROW;
  static constexpr int VELEMS = D * VROW;
  static constexpr int ELEMS = KELEMS + VELEMS;      // one buffer
  static constexpr int NCH = D / 64;                 // 16-byte chunks per thread per operand
  static constexpr int LDSW = D + 2;                 // floats per combined row: O, m, l
  static constexpr int kBufBytes = 2 * ELEMS * 2;
  static constexpr int kCombBytes = 3 * 16 * LDSW * 4;
  static constexpr int kBytes = kBufBytes > kCombBytes ? kBufBytes : kCombBytes;
};

// staging: thread tid copies 16-byte chunks c = tid + 256 j of the block's K (row c / (D/8))
// and V^T (d row c / 4, keys 8 (c % 4) ..): global -> registers ...
template <int D>
__device__ __forceinline__ void fetch_chunks(const BlockRef& r, u32x4 (&rk)[LdsTile<D>::NCH],
                                             u32x4 (&rv)[LdsTile<D>::NCH]) {
#pragma unroll
  for (int j = 0; j < LdsTile<D>::NCH; ++j) {
    const int c = static_cast<int>(threadIdx.x) + kAttnThreads * j;
    rk[j] = *reinterpret_cast<const u32x4*>(r.k + c * 8);
    rv[j] = *reinterpret_cast<const u32x4*>(r.vt + c * 8);
  }
}

// ... registers -> block j's padded buffer, j & 1.  256 is a whole number of K and of V^T
// rows, so chunk c's place is chunk tid's plus a compile-time offset: one address per operand
template <int D>
__device__ __forceinline__ void stage_chunks(__bf16* buf, int j, const u32x4 (&rk)[LdsTile<D>::NCH],
                                             const u32x4 (&rv)[LdsTile<D>::NCH]) {
  using LT = LdsTile<D>;
  __bf16* kd = buf + (j & 1) * LT::ELEMS;
  __bf16* vd = kd + LT::KELEMS;
  const int tid = threadIdx.x;
  __bf16* kt = kd + (tid / (D / 8)) * LT::KROW + (tid % (D / 8)) * 8;
  __bf16* vt = vd + (tid >> 2) * LT::VROW + (tid & 3) * 8;
#pragma unroll
  for (int i = 0; i < LT::NCH; ++i) {
    *reinterpret_cast<u32x4*>(kt + i * (kAttnThreads / (D / 8)) * LT::KROW) = rk[i];
    *reinterpret_cast<u32x4*>(vt + i * (kAttnThreads / 4) * LT::VROW) = rv[i];
  }
}

// the staged block j (buffer j & 1) attended by this wave; mine_staged: is it this wave's --
// the tile's wave ks takes the blocks j % kw == ks
__device__ __forceinline__ bool mine_staged(const TileRows& tr, int j) {
  return tr.active && (j % tr.kw) == tr.ks;
}

template <int D, typename Ref>
__device__ __forceinline__ void attend_staged(const AttnParams& a, const TileRows& tr, const __bf16* buf,
                                              int j, Ref ref, const bf16x8 (&qf)[D / 32],
                                              f32x4 (&o)[D / 16], float& m, float& l) {
  using LT = LdsTile<D>;
  const int col = tr.col, h4 = tr.h4;
  const __bf16* kd = buf + (j & 1) * LT::ELEMS;
  const __bf16* vd = kd + LT::KELEMS;
  KeyBlock<D> f;
#pragma unroll
  for (int ds = 0; ds < D / 32; ++ds) {
    f.k0[ds] = *reinterpret_cast<const bf16x8*>(kd + col * LT::KROW + ds * 32 + 8 * h4);
    f.k1[ds] = *reinterpret_cast<const bf16x8*>(kd + (16 + col) * LT::KROW + ds * 32 + 8 * h4);
  }
#pragma unroll
  for (int dt = 0; dt < D / 16; ++dt) {
    f.vlo[dt] = *reinterpret_cast<const bf16x4*>(vd + (dt * 16 + col) * LT::VROW + 4 * h4);
    f.vhi[dt] = *reinterpret_cast<const bf16x4*>(vd + (dt * 16 + col) * LT::VROW + 16 + 4 * h4);
  }
  attend_block<D>(a, f, ref(j).mask, qf, tr.kmin_pos, h4, o, m, l);
}

// The staged pipeline: the workgroup's key blocks ref(0) .. ref(n - 1) (n uniform; ref(j): a
// BlockRef), each staged once and attended by every tile, double-buffered -- block j + 1's
// 16-byte global loads are in flight while block j is attended from LDS, staged after it
// (buffer (j + 1) & 1 was last read in iteration j - 1), one barrier per block.
// Expanded in the kernel body, not called: with this loop in a function of its own, however
// it is passed its operands, prefix_attn_plan_lds_kernel<128, true> needs 170-172 VGPRs for
// the same instructions (168, three waves per SIMD, when it is expanded in place).
#define CS_ATTEND_STAGED(D, a, tr, lds, n_blocks, ref, qf, o, m, l)                         \
  do {                                                                                      \
    using LT_ = LdsTile<D>;                                                                 \
    const int n_ = (n_blocks);                                                              \
    __bf16* buf_ = reinterpret_cast<__bf16*>(lds);                                          \
    u32x4 rk_[LT_::NCH], rv_[LT_::NCH];                                                     \
    if (n_ > 0) {                                                                           \
      fetch_chunks<D>(ref(0), rk_, rv_);                                                    \
      stage_chunks<D>(buf_, 0, rk_, rv_);                                                   \
    }                                                                                       \
    __syncthreads();                                                                        \
    for (int j_ = 0; j_ < n_; ++j_) {                                                       \
      const bool more_ = j_ + 1 < n_;                                                       \
      if (more_) fetch_chunks<D>(ref(j_ + 1), rk_, rv_);                                    \
      if (mine_staged(tr, j_)) attend_staged<D>(a, tr, buf_, j_, ref, qf, o, m, l);   \
      if (more_) stage_chunks<D>(buf_, j_ + 1, rk_, rv_);                                   \
      __syncthreads();                                                                      \
    }                                                                                       \
  } while (0)

// l summed over the lane groups, then the waves that share a query tile combine through LDS
// into the tile's wave ks = 0 (fixed order: ks = 0, 1, ...).  Every wave of the workgroup
// calls this, after a barrier that ends the last use of the LDS.
template <int D>
__device__ __forceinline__ void combine_waves(const TileRows& tr, char* lds, f32x4 (&o)[D / 16],
                                              float& m, float& l) {
  auto sm = reinterpret_cast<float (*)[16][LdsTile<D>::LDSW]>(lds);
  const int n_qt = tr.n_qt, kw = tr.kw, col = tr.col, h4 = tr.h4;
  l += __shfl_xor(l, 16, 64);
  l += __shfl_xor(l, 32, 64);
  if (kw > 1) {
    if (tr.active && tr.ks > 0) {
      const int sl = tr.w - n_qt;
#pragma unroll
      for (int dt = 0; dt < D / 16; ++dt)
#pragma unroll
        for (int i = 0; i < 4; ++i) sm[sl][col][dt * 16 + 4 * h4 + i] = o[dt][i];
      if (h4 == 0) {
        sm[sl][col][D] = m;
        sm[sl][col][D + 1] = l;
      }
    }
    __syncthreads();
    if (tr.active && tr.ks == 0) {
      float mt = m;
      for (int k = 1; k < kw; ++k) mt = fmaxf(mt, sm[tr.qt + n_qt * k - n_qt][col][D]);
      const float c0 = mt == -INFINITY ? 0.0f : __builtin_amdgcn_exp2f(m - mt);
      l *= c0;
#pragma unroll
      for (int dt = 0; dt < D / 16; ++dt) o[dt] *= c0;
      for (int k = 1; k < kw; ++k) {
        const int sl = tr.qt + n_qt * k - n_qt;
        const float mk = sm[sl][col][D];
        const float ck = mt == -INFINITY ? 0.0f : __builtin_amdgcn_exp2f(mk - mt);
        l = fmaf(sm[sl][col][D + 1], ck, l);
#pragma unroll
        for (int dt = 0; dt < D / 16; ++dt)
#pragma unroll
          for (int i = 0; i < 4; ++i) o[dt][i] = fmaf(sm[sl][col][dt * 16 + 4 * h4 + i], ck, o[dt][i]);
      }
      m = mt;
    }
  }
}

// the lane's row of out: O / l as bf16 (zeros for a row that saw no key)
template <int D>
__device__ __forceinline__ void store_out(const AttnParams& a, const TileRows& tr,
                                          const f32x4 (&o)[D / 16], float l) {
  const float inv = l > 0.0f ? 1.0f / l : 0.0f;
  __bf16* orow = a.out + (tr.tok * a.H + tr.head) * D + 4 * tr.h4;
#pragma unroll
  for (int dt = 0; dt < D / 16; ++dt) {
    bf16x4 v;
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = static_cast<__bf16>(o[dt][i] * inv);
    *reinterpret_cast<bf16x4*>(orow + dt * 16) = v;
  }
}

// Scoring chunks and prompt prefill (no plan, T > 1, >= 1024 cells): the workgroup's four
// 16-row query tiles walk ONE key-block list -- the agent's prefix blocks, then the history
// blocks of every stream the 64 rows touch, up to the furthest query's causal limit -- through
// CS_ATTEND_STAGED (loading every block once per tile instead is 4x the L2 traffic for 64
// rows of one stream).  Blocks outside a tile's own stream or causal range are masked per lane
// (block_mask); the arithmetic of a block is attend_block's.
// D = 256: one wave per SIMD (two: 208 B/lane of spills)
template <int D>
__global__ __launch_bounds__(kAttnThreads, D <= 128 ? 2 : 1)
void prefix_attn_lds_kernel(AttnParams a) {
  __shared__ __attribute__((aligned(16))) char lds[LdsTile<D>::kBytes];
  const int bid = logical_block(a.swizzle);
  const TileRows tr = tile_rows(a, bid / a.n_qg, bid % a.n_qg);
  const HistBlocks hs = hist_blocks(a, tr.hb, tr.r0, tr.r0 + tr.nrows - 1);
  const int nbp = (tr.pl + kKeyBlock - 1) / kKeyBlock;

  bf16x8 qf[D / 32];
  load_q<D>(a, tr, qf);
  f32x4 o[D / 16];
#pragma unroll
  for (int dt = 0; dt < D / 16; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m = -INFINITY, l = 0.0f;

  // the workgroup's key-block list
  const KvBase kv = kv_base(a);
  auto ref = [&](int it) {
    return it < nbp ? prefix_block<D>(a, kv, tr, it) : hist_block<D>(a, kv, tr, hs, it - nbp);
  };
  CS_ATTEND_STAGED(D, a, tr, lds, nbp + hs.n, ref, qf, o, m, l);
  combine_waves<D>(tr, lds, o, m, l);
  if (tr.vrow && tr.ks == 0) store_out<D>(a, tr, o, l);
}

// ---- the wide tile: 32 query rows per wave over 64-key blocks (v_mfma_f32_32x32x16_bf16) ----
//
// Scoring chunks and prompt prefill at D = 128 without soft-cap or window (the rule is in
// prefix_attention_impl).  A workgroup of kWideWaves waves holds 32 kWideWaves consecutive query
// rows of one (group, K/V head), one 32-row tile per wave, and walks ONE list of 64-key blocks:
// the prefix's, then those of every stream its rows touch up to the furthest query's causal
// limit.  Per barrier and per memory round trip a wave attends 32 rows x 64 keys where
// prefix_attn_lds_kernel's attends 16 x 32.
//
// Operands (32x32x16 bf16 maps: lane l, r = l & 31, h = l >> 5 holds A[r][8h + j], B[8h + j][r],
// C[(i & 3) + 8 (i >> 2) + 4h][r] in register i): S^T = K . Q^T per 32-key half-block, so the
// lane keeps query column r and, per half-block, the 16 keys (i & 3) + 8 (i >> 2) + 4h.
// Registers 8s .. 8s + 7 rounded to bf16 are the B fragment of k-step s of O^T = V^T . P^T with
// the k slots ordered key(h, j) = 16s + 8 (j >> 2) + 4h + (j & 3) -- the file header's ordering
// argument on the 32-wide map -- and the V^T fragment of d row r is keys 16s + 4h .. + 3 and
// 16s + 8 + 4h .. + 3 of that row.  m and l need one exchange between the two lane halves.
//
// LDS image of a block (32 KB, two buffers): K as 64 rows of 256 B with 16-byte chunk c of row k
// at chunk c ^ (k & 15) (a ds_read_b128 lane group reads 16 rows distinct mod 16 at one c:
// conflict-free); each 32-key V^T tile as D rows of 64 B in which the 8-byte key group
// 4s + 2u + h sits at 16-byte chunk (2s + h) ^ ((d >> 2) & 3), half u: the lane's two key groups
// of a k-step are ONE 16-byte read, and a lane group's 16 rows land in 16 different chunks of
// the 256-byte bank window.
//
// Staging is through registers (no LDS DMA): block j + 2's 16-byte loads are issued after block
// j's QK^T and written to buffer (j + 1) & 1 ... after the next barrier, which is also the one
// that ends block j - 1's reads of that buffer: one barrier per 64 keys.  A wave skips (between
// barriers) a staged history block that none of its own 32 rows can see.
//
// A 64-key block's second 32-key tile may not exist (prefixes are padded to 32 keys and ld_hist
// is a multiple of 32, not 64): when no row of the workgroup can see a key of it, the second
// half is staged from the block's FIRST tile again -- K / V that exist, that the first half
// reads anyway, and that the mask hides (index >= 32 in the block is >= the limit).  No address
// outside [0, ld_prefix) or the stream's [0, ld_hist) is ever formed.
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kWideWaves = 4;        // waves (32-row tiles) per workgroup
constexpr int kWideBlock = 64;       // keys per staged block

template <int D, int NW>
struct WideLds {
  static_assert(D == 128, "the chunk swizzles below are written for 256-byte K rows");
  static constexpr int NT = 64 * NW;
  static constexpr int KBYTES = kWideBlock * D * 2;
  static constexpr int VTILE = D * 64;                       // one 32-key V^T tile
  static constexpr int BUF = KBYTES + 2 * VTILE;
  static constexpr int NCH = kWideBlock * (D / 8) / NT;      // 16-byte chunks per thread per operand
  static constexpr int QIMG = 32 * D * 2;                    // a wave's 32 rows of out
  static_assert(NW * QIMG <= 2 * BUF, "every wave's row image fits the two key buffers");
  static_assert(NCH >= 2 && NCH % 2 == 0, "a thread's chunks split evenly over the two tiles");
};

// the workgroup's rows as a TileRows: wave w holds rows r0 + 32w .. + 31, lane (col = l & 31,
// h4 = l >> 5) query column col; no key striping (kw = 1) and no window
template <int NW>
__device__ __forceinline__ TileRows wide_rows(const AttnParams& a, int pg, int qg) {
  TileRows r;
  r.gi = pg / a.Hkv;
  r.g = pg % a.Hkv;
  const int p = a.gpfx ? a.gpfx[r.gi] : r.gi;
  r.M = a.n_str * a.T * a.rep;
  r.r0 = qg * 32 * NW;
  r.nrows = min(32 * NW, r.M - r.r0);
  r.n_qt = (r.nrows + 31) >> 5;
  r.kw = 1;
  const int tid = threadIdx.x;
  r.w = tid >> 6;
  r.lane = tid & 63;
  r.qt = r.w;
  r.ks = 0;
  r.active = r.w < r.n_qt;
  r.col = r.lane & 31;
  r.h4 = r.lane >> 5;
  const int row = r.r0 + r.w * 32 + r.col;
  r.vrow = row < r.M;
  const int rr = r.vrow ? row : r.M - 1;
  const int jh = rr % a.rep, bt = rr / a.rep;
  r.t = bt % a.T;
  r.b = bt / a.T;
  r.tok = (static_cast<int64_t>(r.gi) * a.n_str + r.b) * a.T + r.t;
  r.head = r.g * a.rep + jh;
  r.hb = *a.hist_base;
  r.pl = a.plen[p];
  r.po = a.poff[p];
  r.hv = min(r.hb + r.t + 1, static_cast<int>(a.ldh));
  r.kmin_pos = INT32_MIN;
  return r;
}

// a 64-key block: the K rows and V^T tile of its two 32-key tiles (the second the first again
// when it is not needed), its first key and the stream it belongs to (-1: the prefix)
struct WideRef {
  const __bf16 *k0, *vt0, *k1, *vt1;
  int kb, bb;
};

template <int D, int NW>
__device__ __forceinline__ void wide_fetch(const WideRef& r, u32x4 (&rk)[WideLds<D, NW>::NCH],
                                           u32x4 (&rv)[WideLds<D, NW>::NCH]) {
  using WL = WideLds<D, NW>;
  const int tid = threadIdx.x;
#pragma unroll
  for (int j = 0; j < WL::NCH; ++j) {
    // chunk c = tid + NT j of 1024: K row c / 16 of 64, V^T chunk c % 512 of tile c / 512
    const bool first = j < WL::NCH / 2;
    const int c = tid + WL::NT * (j % (WL::NCH / 2));        // the chunk inside its tile
    rk[j] = *reinterpret_cast<const u32x4*>((first ? r.k0 : r.k1) + c * 8);
    rv[j] = *reinterpret_cast<const u32x4*>((first ? r.vt0 : r.vt1) + c * 8);
  }
}

template <int D, int NW>
__device__ __forceinline__ void wide_stage(char* buf, const u32x4 (&rk)[WideLds<D, NW>::NCH],
                                           const u32x4 (&rv)[WideLds<D, NW>::NCH]) {
  using WL = WideLds<D, NW>;
  typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
  const int tid = threadIdx.x;
#pragma unroll
  for (int j = 0; j < WL::NCH; ++j) {
    const int half = j < WL::NCH / 2 ? 0 : 1;
    const int c = tid + WL::NT * (j % (WL::NCH / 2));
    const int krow = c >> 4, kch = c & 15;
    *reinterpret_cast<u32x4*>(buf + (half * 32 + krow) * 256 + ((kch ^ (krow & 15)) << 4)) = rk[j];
    // V^T chunk: d row c / 4, keys 8 (c % 4) .. + 7 = key groups 2 (c % 4) (h = 0), + 1 (h = 1)
    const int d = c >> 2, s = (c >> 1) & 1, u = c & 1, g = (d >> 2) & 3;
    char* vrow = buf + WL::KBYTES + half * WL::VTILE + d * 64 + u * 8;
    *reinterpret_cast<u32x2*>(vrow + (((2 * s) ^ g) << 4)) = u32x2{rv[j][0], rv[j][1]};
    *reinterpret_cast<u32x2*>(vrow + (((2 * s + 1) ^ g) << 4)) = u32x2{rv[j][2], rv[j][3]};
  }
}

template <int D, int NW>
__global__ __launch_bounds__(64 * NW, 2)
void prefix_attn_wide_kernel(AttnParams a) {
  using WL = WideLds<D, NW>;
  constexpr int NDS = D / 16;        // k-steps of QK^T
  constexpr int NDT = D / 32;        // 32-row d tiles of O^T
  __shared__ __attribute__((aligned(16))) char lds[2 * WL::BUF];
  const int bid = logical_block(a.swizzle);
  const TileRows tr = wide_rows<NW>(a, bid / a.n_qg, bid % a.n_qg);
  const int row1 = tr.r0 + tr.nrows - 1;
  const HistBlocks hs = hist_blocks(a, tr.hb, tr.r0, row1);
  // the list: the prefix's 64-key blocks, then per stream b_lo .. b_hi those up to the
  // stream's furthest query's causal limit -- hs.hlim (every token) for all but the last
  // stream, whose last row of the workgroup sets its own
  const int nbp = (tr.pl + kWideBlock - 1) / kWideBlock;
  const int n_st = hs.n / hs.nbh;                                   // streams (hs.nbh >= 1)
  const int hlim_last = min(tr.hb + (row1 / a.rep) % a.T + 1, static_cast<int>(a.ldh));
  const int nbh_full = (hs.hlim + kWideBlock - 1) / kWideBlock;
  const int nbh_last = (hlim_last + kWideBlock - 1) / kWideBlock;
  const int n = nbp + (n_st - 1) * nbh_full + nbh_last;
  const int r = tr.col, h = tr.h4;

  // the wave's own rows (uniform): which staged history blocks any of them can see
  const int w = __builtin_amdgcn_readfirstlane(tr.w);
  const int wr0 = tr.r0 + 32 * w, wr1 = min(wr0 + 31, tr.M - 1);
  const bool wact = wr0 < tr.M;
  const int wb_lo = (wr0 / a.rep) / a.T, wb_hi = (wr1 / a.rep) / a.T, wt_hi = (wr1 / a.rep) % a.T;

  const KvBase kv = kv_base(a);
  // A place in the list, stepped with adds alone (the block references' products and
  // quotients, formed per block, were a third of this loop's instructions): block it, from nbp
  // on block j of the list's stream si; kb its first key and off the element offset of its
  // first K row and V^T tile in k_pfx / vt_pfx or k_hist / vt_hist
  struct Cursor {
    int it, si, j, kb;
    int64_t off;
  };
  const int64_t hoff0 = ((static_cast<int64_t>(tr.gi) * a.n_str + hs.b_lo) * a.Hkv + tr.g) * a.ldh * D;
  const int64_t hstride = static_cast<int64_t>(a.Hkv) * a.ldh * D;
  const Cursor c0 = {0, 0, 0, 0, nbp > 0 ? (static_cast<int64_t>(tr.g) * a.ldp + tr.po) * D : hoff0};
  auto step = [&](Cursor& c) {
    ++c.it;
    if (c.it < nbp || (c.it > nbp && ++c.j < (c.si == n_st - 1 ? nbh_last : nbh_full))) {
      c.kb += kWideBlock;
      c.off += kWideBlock * D;
    } else {                       // a stream's first block
      if (c.it > nbp) ++c.si;
      c.j = 0;
      c.kb = 0;
      c.off = hoff0 + c.si * hstride;
    }
  };
  auto ref = [&](const Cursor& c) {
    WideRef x;
    const bool hist = c.it >= nbp;
    const int lim = hist ? (c.si == n_st - 1 ? hlim_last : hs.hlim) : tr.pl;
    x.k0 = (hist ? kv.kh : kv.kp) + c.off;
    x.vt0 = (hist ? kv.vth : kv.vtp) + c.off;
    // the second tile only where a row of the workgroup sees a key of it: it exists then
    const bool two = c.kb + kKeyBlock < lim;
    x.k1 = two ? x.k0 + kKeyBlock * D : x.k0;
    x.vt1 = two ? x.vt0 + kKeyBlock * D : x.vt0;
    x.kb = c.kb;
    x.bb = hist ? hs.b_lo + c.si : -1;
    return x;
  };

  // Q^T fragments: the lane's row, d 16 ds + 8h ..
  bf16x8 qf[NDS];
  {
    const __bf16* qrow = a.q + (tr.tok * a.H + tr.head) * D + 8 * h;
#pragma unroll
    for (int ds = 0; ds < NDS; ++ds) {
      if (tr.vrow) {
        qf[ds] = *reinterpret_cast<const bf16x8*>(qrow + ds * 16);
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) qf[ds][e] = static_cast<__bf16>(0.0f);
      }
    }
  }
  f32x16 o[NDT];
#pragma unroll
  for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
    for (int i = 0; i < 16; ++i) o[dt][i] = 0.0f;
  float m = -INFINITY, l = 0.0f;
  const float sl2 = a.scale * kLog2e;

  // this lane's fragment addresses inside a buffer: K row r (and 32 + r), chunk (2 ds + h) ^
  // (r & 15) = (h ^ (r & 15)) ^ 2 ds; V^T row 32 dt + r, chunk (2s + h) ^ ((r >> 2) & 3)
  const int kx = h ^ (r & 15);
  const int vx = h ^ ((r >> 2) & 3);
  const int koff = r * 256;
  const int voff0 = WL::KBYTES + r * 64 + (vx << 4), voff1 = WL::KBYTES + r * 64 + ((vx ^ 2) << 4);

  u32x4 rk[WL::NCH], rv[WL::NCH];
  Cursor ca = c0, cf = c0;      // the block attended; the next one to fetch
  // n >= 1: every row sees its own key
  wide_fetch<D, NW>(ref(cf), rk, rv);
  wide_stage<D, NW>(lds, rk, rv);
  step(cf);
  if (n > 1) {
    wide_fetch<D, NW>(ref(cf), rk, rv);
    step(cf);
  }
  for (int j = 0; j < n; ++j) {
    __syncthreads();      // block j staged; block j - 1's reads of the other buffer done
    if (j + 1 < n) wide_stage<D, NW>(lds + ((j + 1) & 1) * WL::BUF, rk, rv);
    const WideRef x = ref(ca);
    step(ca);
    const BlockMask mk = block_mask(tr, x.kb, x.bb >= 0, x.bb);
    // wave-uniform skip: a history block of a stream none of the wave's rows are in, or past
    // the furthest causal limit of those that are
    bool mine = wact;
    if (x.bb >= 0) {
      const int wl = (x.bb < wb_lo || x.bb > wb_hi)
                         ? 0 : min(tr.hb + (x.bb == wb_hi ? wt_hi : a.T - 1) + 1, static_cast<int>(a.ldh));
      mine = mine && mk.kb < wl;
    }
    const char* buf = lds + (j & 1) * WL::BUF;
    f32x16 s0, s1;
    if (mine) {
#pragma unroll
      for (int i = 0; i < 16; ++i) s0[i] = s1[i] = 0.0f;
      // fragment reads run two groups of four ahead of the MFMAs that use them: a read's
      // latency hides behind the four MFMAs of the group before, not in front of its own
      bf16x8 kf[NDS / 2][4];
      auto read_k = [&](int g) {
#pragma unroll
        for (int e = 0; e < 2; ++e) {
          const char* kp = buf + koff + ((kx ^ (2 * (2 * g + e))) << 4);
          kf[g][2 * e] = *reinterpret_cast<const bf16x8*>(kp);
          kf[g][2 * e + 1] = *reinterpret_cast<const bf16x8*>(kp + 32 * 256);
        }
      };
      read_k(0);
      read_k(1);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int g = 0; g < NDS / 2; ++g) {
        if (g + 2 < NDS / 2) read_k(g + 2);
#pragma unroll
        for (int e = 0; e < 2; ++e) {
          s0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf[g][2 * e], qf[2 * g + e], s0, 0, 0, 0);
          s1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf[g][2 * e + 1], qf[2 * g + e], s1, 0, 0, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    if (j + 2 < n) {
      wide_fetch<D, NW>(ref(cf), rk, rv);
      step(cf);
    }
    if (mine) {
      // V^T fragments of k-step g = 2c + s (half-block c), all d tiles
      bf16x8 vf[4][NDT];
      auto read_v = [&](int g) {
#pragma unroll
        for (int dt = 0; dt < NDT; ++dt)
          vf[g][dt] = *reinterpret_cast<const bf16x8*>(buf + ((g & 1) ? voff1 : voff0) + (g >> 1) * WL::VTILE +
                                                       dt * 32 * 64);
      };
      // key index i of the block is visible to the lane iff i < lim - kb; the lane's keys are
      // 32c + (i & 3) + 8 (i >> 2) + 4h.  A block every lane sees whole skips the selects
      const int jhi = mk.lim - mk.kb - 4 * h;
      if (__ballot(mk.lim - mk.kb < kWideBlock) != 0) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int ki = (i & 3) + 8 * (i >> 2);
          s0[i] = ki < jhi ? s0[i] : -INFINITY;
          s1[i] = 32 + ki < jhi ? s1[i] : -INFINITY;
        }
      }
      // max(a, b) as med3(a, b, +inf): no NaN can reach here, and fmaxf would first quiet each
      // input (an instruction per score)
      auto mx = [](float x, float y) { return __builtin_amdgcn_fmed3f(x, y, INFINITY); };
      float b0 = mx(s0[0], s1[0]), b1 = mx(s0[1], s1[1]);
#pragma unroll
      for (int i = 2; i < 16; i += 2) {
        b0 = mx(b0, mx(s0[i], s1[i]));
        b1 = mx(b1, mx(s0[i + 1], s1[i + 1]));
      }
      float bm = mx(b0, b1);
      bm *= sl2;                                   // log2 units (scale > 0: the max commutes)
      {
        const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(bm), __float_as_uint(bm), false, false);
        bm = fmaxf(__uint_as_float(sw[0]), __uint_as_float(sw[1]));
      }
      // lazy rescale (attend_block's rule): ONE decision per 64-key block and wave, taken
      // before any of the block's P.V, and l and O take the same factor
      float mn = m;
      if (__ballot(bm > m + kLazyRescale) != 0) {
        mn = fmaxf(m, bm);
        const float alpha = mn == -INFINITY ? 1.0f : __builtin_amdgcn_exp2f(m - mn);
        l *= alpha;
#pragma unroll
        for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
          for (int i = 0; i < 16; ++i) o[dt][i] *= alpha;
      }
      m = mn;
      // p = 2^(s sl2 - m); a row that has seen no key yet has every s = -inf here: p = 0
      const float ms = mn == -INFINITY ? 0.0f : mn;
      float ps = 0.0f;
      bf16x8 pb[2][2];
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const float p0 = __builtin_amdgcn_exp2f(fmaf(s0[i], sl2, -ms));
        const float p1 = __builtin_amdgcn_exp2f(fmaf(s1[i], sl2, -ms));
        ps += p0 + p1;
        pb[0][i >> 3][i & 7] = static_cast<__bf16>(p0);
        pb[1][i >> 3][i & 7] = static_cast<__bf16>(p1);
      }
      l += ps;
      read_v(0);
      read_v(1);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        if (g + 2 < 4) read_v(g + 2);
#pragma unroll
        for (int dt = 0; dt < NDT; ++dt)
          o[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf[g][dt], pb[g >> 1][g & 1], o[dt], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
  }
  l += __shfl_xor(l, 32, 64);
  // store_out's rounding on the 32-wide map: register i of d tile dt is d 32 dt + 8 (i >> 2) +
  // 4h + (i & 3)
  const float inv = l > 0.0f ? 1.0f / l : 0.0f;
  // ... through the wave's own 8 KB of LDS (the key buffers are done with after the barrier),
  // so that a store instruction writes four whole 256-byte rows: the lane's 8-byte pieces of 32
  // rows left the chip as 16-byte fragments of 32 different rows per instruction
  __syncthreads();
  {
    char* img = lds + w * WL::QIMG;
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        bf16x4 v;
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = static_cast<__bf16>(o[dt][4 * g + i] * inv);
        *reinterpret_cast<bf16x4*>(img + r * 256 + (((4 * dt + g) ^ (r & 15)) << 4) + 8 * h) = v;
      }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const int64_t mine_off = tr.vrow ? (tr.tok * a.H + tr.head) * D : -1;
    const int lr = tr.lane >> 4, ch = tr.lane & 15;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int row = 4 * i + lr;
      const int64_t off = __shfl(mine_off, row, 64);      // lane row holds row row
      const u32x4 v = *reinterpret_cast<const u32x4*>(img + row * 256 + ((ch ^ (row & 15)) << 4));
      if (off >= 0) *reinterpret_cast<u32x4*>(a.out + off + ch * 8) = v;
    }
  }
}

#ifdef CS_TRACE_ATTN
// diagnostics build only (tools/attn_trace.py): wall_clock64 ticks (100 MHz) per workgroup of
// the last decode-step launch, plain stores (no atomics: those serialise and distort):
// attention [wg][0 start, 1 prologue loads in, 2 prefix loop done, 3 history loop done
// (wave 0), 4 partial stored (wave 0)], merge [wg][5 start, 6 done]
constexpr int kAttTraceWgs = 4096;
__device__ unsigned long long g_attn_ts[kAttTraceWgs][8];
#define ATT_T(...) __VA_ARGS__
__device__ __forceinline__ void att_at(int i) {
  if (blockIdx.x < kAttTraceWgs) g_attn_ts[blockIdx.x][i] = wall_clock64();
}
#else
#define ATT_T(...)
#endif

// Decode steps (a plan: few (group, head) cells, key splits): the agent's PREFIX blocks
// are shared by the workgroup's four 16-row tiles, so the split's prefix blocks (split,
// split + n_used, ...) go through CS_ATTEND_STAGED, once per workgroup for every tile (loading
// each one per tile: 4x the load instructions, 68 % issue stalls at C5); each tile's own
// streams' history blocks are then loaded per wave (hist_block, load_block).
// Every key block is attended exactly once per (query row, split).
// two waves per SIMD at every D (D = 256: no spills; 1 wave/SIMD before)
//
// ROWS (cs_prefix_attention_rows): the history is row-major for K AND V ([S][Hkv][ldh][D])
// and slot j of stream s lives in stream row hrow[s][j] -- a beam inherits its parent's
// slots through the table (cs_hist_rows_update), no K / V is copied.  A history block's 32
// V rows are gathered by LDS DMA into the wave's own 1 KB-per-16-d image [d/16][key][16 d]
// (lane l loads key l / 2, 8 d of d-tile i: one table entry per lane) and read back
// transposed (ds_read_b64_tr_b16: lane 4q + p of group h reads key 4h + q, d 16 dt + 4p) as
// the V^T operand the V^T-tile layout gives; every 32-lane half reads 8 keys x 32 B at
// 32-B key pitch: 64 distinct banks, conflict-free.
template <int D, bool ROWS = false>
__global__ __launch_bounds__(kAttnThreads, 2)
void prefix_attn_plan_lds_kernel(AttnParams a) {
  using LT = LdsTile<D>;
  constexpr int NDS = D / 32;
  constexpr int NDT = D / 16;
  constexpr int kVImg = kKeyBlock * D * 2;            // ROWS: one wave's V image of a block
  static_assert(kAttnThreads / 64 * kVImg <= LT::kBufBytes, "the V images fit the prefix buffers");
  __shared__ __attribute__((aligned(16))) char lds[LT::kBytes];

  ATT_T(if (threadIdx.x == 0) att_at(0);)
  // no plan (ROWS only): one workgroup per (group, head, query group), unsplit
  const int4 e = a.plan ? a.plan[blockIdx.x]
                        : int4{static_cast<int>(blockIdx.x) / a.n_qg, static_cast<int>(blockIdx.x) % a.n_qg,
                               1 << 8, 0};
  const int split = e.z & 255, n_used = e.z >> 8, slot = e.w;
  const TileRows tr = tile_rows(a, e.x, e.y);
  const int lane = tr.lane, w = tr.w, kw = tr.kw, ks = tr.ks;
  const int col = tr.col, h4 = tr.h4;
  const bool active = tr.active;

  const int nbp = (tr.pl + kKeyBlock - 1) / kKeyBlock;
  // this split's prefix blocks: split, split + n_used, ...  (workgroup-uniform)
  const int npi = nbp > split ? (nbp - split + n_used - 1) / n_used : 0;
  ATT_T(if (threadIdx.x == 0 && npi + tr.hb + tr.po >= 0) att_at(1);)
  // the tile's own streams' history blocks, per wave (split * kw + ks, + nslot, ...)
  const int rt0 = tr.r0 + tr.qt * 16;
  const HistBlocks hs = hist_blocks(a, tr.hb, rt0, min(rt0 + 15, tr.M - 1));
  const int n_hist = hs.n;
  const int nslot = n_used * kw;
  // ROWS: lane l's table entry (key l % 32) of history block ih; the first block's entry is
  // loaded here, its round trip hidden behind the prefix blocks, each later one during the
  // block before it
  auto hrow_of = [&](int ih) -> int32_t {
    const int64_t sg = static_cast<int64_t>(tr.gi) * a.n_str + hs.b_lo + ih / hs.nbh;
    return a.hrow[sg * a.ldh + (ih % hs.nbh) * kKeyBlock + (lane & 31)];
  };
  int32_t hcur = 0;
  if constexpr (ROWS) {
    if (active && split * kw + ks < n_hist) hcur = hrow_of(split * kw + ks);
  }

  bf16x8 qf[NDS];
  load_q<D>(a, tr, qf);
  f32x4 o[NDT];
#pragma unroll
  for (int dt = 0; dt < NDT; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m = -INFINITY, l = 0.0f;

  // ---- prefix blocks through LDS ----
  const KvBase kv = kv_base(a);
  auto ref = [&](int j) { return prefix_block<D>(a, kv, tr, split + j * n_used); };
  CS_ATTEND_STAGED(D, a, tr, lds, npi, ref, qf, o, m, l);

  ATT_T(if (threadIdx.x == 0) att_at(2);)
  if constexpr (!ROWS) {
    if (active) {
      for (int ih = split * kw + ks; ih < n_hist; ih += nslot) {
        KeyBlock<D> f;
        const BlockRef r = hist_block<D>(a, kv, tr, hs, ih);
        load_block<D>(f, r, col, h4);
        attend_block<D>(a, f, r.mask, qf, tr.kmin_pos, h4, o, m, l);
      }
    }
  } else {
    unsigned char* vimg = reinterpret_cast<unsigned char*>(lds) + w * kVImg;
    // the wave's V image of a block: key-major, key k's 2D bytes at 2D k, its 16-byte chunk c
    // at chunk c ^ sw(k) (sw even: 32-byte pairs stay whole).  A transposed read (lane 4q + p
    // of group h4: key 4 h4 + q, d 16 dt + 4 p) of one half-wave then touches 8 keys whose
    // pairs sit in 8 different 8-bank groups: conflict-free.  A DMA instruction writes KPI
    // whole keys, so only the keys the block's rows can see are gathered
    constexpr int CPK = D / 8;          // 16-byte chunks per key
    constexpr int KPI = 64 / CPK;       // keys per 1 KB DMA instruction
    const int kq = 4 * h4 + ((lane & 15) >> 2);          // this lane's vlo key (vhi: + 16)
    const uint32_t tr_base = static_cast<uint32_t>(kq * 2 * D + 8 * (lane & 3));
    const int s2 = vimg_swz<D>(kq) >> 1;
    // this lane's DMA chunk: key i KPI + lane / CPK of instruction i, chunk lane % CPK
    const int dkey = lane / CPK, dch = lane % CPK;
    typedef __attribute__((address_space(3))) bf16x4* lds_b4_ptr;
    if (active && split * kw + ks < n_hist) {
      // the image starts zeroed: a key the block's rows cannot see is not gathered, and its
      // V row must still be finite (its probability is 0; 0 x NaN is not): zeros, or an
      // earlier block's rows
#pragma unroll
      for (int i = 0; i < kVImg / 1024; ++i)
        *reinterpret_cast<u32x4*>(vimg + 1024 * i + 16 * lane) = u32x4{0u, 0u, 0u, 0u};
    }
    if (active) {
      for (int ih = split * kw + ks; ih < n_hist; ih += nslot) {
        const BlockMask mk = hist_block<D>(a, kv, tr, hs, ih).mask;
        const int kb = mk.kb;
        // keys the tile's rows can see (wave-uniform): only those are gathered
        const int nvalid = min(kKeyBlock, hs.hlim - kb);
        const int n_instr = (nvalid + KPI - 1) / KPI;
        auto row_ptr = [&](const __bf16* base, int64_t srow, int key) {
          return base + ((srow * a.Hkv + tr.g) * a.ldh + kb + key) * D;
        };
        // stream rows of keys col, 16 + col (K fragments)
        const int64_t rk0 = __shfl(hcur, col, 64), rk1 = __shfl(hcur, 16 + col, 64);
        KeyBlock<D> f;
        const __bf16* kp0 = row_ptr(a.kh, rk0, col) + 8 * h4;
        const __bf16* kp1 = row_ptr(a.kh, rk1, 16 + col) + 8 * h4;
        // K first, then the V gather (the DMA issue never waits), then the next block's
        // table entry: every load of the block in flight before the one wait
#pragma unroll
        for (int ds = 0; ds < NDS; ++ds) {
          f.k0[ds] = *reinterpret_cast<const bf16x8*>(kp0 + ds * 32);
          f.k1[ds] = *reinterpret_cast<const bf16x8*>(kp1 + ds * 32);
        }
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // the last block's reads are done
#pragma unroll 1
        for (int i = 0; i < n_instr; ++i) {
          const int k = i * KPI + dkey;
          const int64_t rv = __shfl(hcur, k, 64);
          const __bf16* vsrc = row_ptr(a.vth, rv, k) + 8 * (dch ^ vimg_swz<D>(k));
          __builtin_amdgcn_global_load_lds(vsrc, (__attribute__((address_space(3))) void*)(vimg + 1024 * i),
                                           16, 0, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
        const int ihn = ih + nslot < n_hist ? ih + nslot : ih;
        const int32_t hnext = hrow_of(ihn);
        __builtin_amdgcn_sched_barrier(0);
        // the V image landed (the compiler drains every VMEM op before an LDS read that
        // follows an LDS DMA: the next table entry, an L2 hit issued after the HBM-bound
        // gather, is in by then too)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
        for (int dt = 0; dt < NDT; ++dt) {
          const uint32_t o2 = tr_base + 32 * (((dt & 7) ^ s2) + (dt & ~7));
          f.vlo[dt] = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_b4_ptr)(vimg + o2));
          f.vhi[dt] = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_b4_ptr)(vimg + o2 + 32 * D));
        }
        attend_block<D>(a, f, mk, qf, tr.kmin_pos, h4, o, m, l);
        hcur = hnext;
      }
    }
    __syncthreads();   // every wave's V image read before the combine reuses the LDS
  }
  ATT_T(if (threadIdx.x == 0 && l >= 0.0f) att_at(3);)
  combine_waves<D>(tr, lds, o, m, l);
  if (!tr.vrow || ks != 0) return;
  if (n_used == 1) {
    store_out<D>(a, tr, o, l);
  } else {
    float* pr = a.part + (static_cast<int64_t>(slot) * kGroupRows + tr.qt * 16 + col) * LT::LDSW;
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt)
      *reinterpret_cast<f32x4*>(pr + dt * 16 + 4 * h4) = o[dt];
    if (h4 == 0) {
      pr[D] = m;
      pr[D + 1] = l;
    }
  }
  ATT_T(if (threadIdx.x == 0) { __builtin_amdgcn_s_waitcnt(0); att_at(4); })
}

#undef CS_ATTEND_STAGED

// One workgroup per merge entry (kMergeRows rows of a split (group, head, query group)),
// each wave two rows, one per 32-lane half: the half's lanes fold the splits' (m, l) into
// per-split weights, then the wave sums the weighted partial outputs (f32x4 columns).
// Fixed split order: deterministic.
template <int D>
__global__ __launch_bounds__(kAttnThreads) void attn_merge_kernel(AttnParams a) {
  constexpr int LDSW = D + 2;
  constexpr int NC = D / 4;
  __shared__ float wsm[kAttnThreads / 64][2][kMaxSplit];
  __shared__ float linv[kAttnThreads / 64][2];
  ATT_T(if (threadIdx.x == 0) att_at(5);)
  const int4 e = a.plan[a.n_attn + blockIdx.x];
  const int pg = e.x, qg = e.y, slot0 = e.z, chunk = e.w & 255, nu = e.w >> 8;
  const int gi = pg / a.Hkv, g = pg % a.Hkv;
  const int M = a.n_str * a.T * a.rep;
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int half = lane >> 5, l32 = lane & 31;
  const float* base = a.part + static_cast<int64_t>(slot0) * kGroupRows * LDSW;
  {
    const int rl = chunk * kMergeRows + 2 * w + half;
    const bool vr = qg * kGroupRows + rl < M && l32 < nu;
    float ms = -INFINITY, ls = 0.0f;
    if (vr) {
      const float* pm = base + (static_cast<int64_t>(l32) * kGroupRows + rl) * LDSW + D;
      ms = pm[0];
      ls = pm[1];
    }
    float mt = ms;
#pragma unroll
    for (int o = 16; o >= 1; o >>= 1) mt = fmaxf(mt, __shfl_xor(mt, o, 64));
    const float wt = (vr && mt != -INFINITY) ? __builtin_amdgcn_exp2f(ms - mt) : 0.0f;
    float lt = wt * ls;
#pragma unroll
    for (int o = 16; o >= 1; o >>= 1) lt += __shfl_xor(lt, o, 64);
    if (l32 < kMaxSplit) wsm[w][half][l32] = wt;
    if (l32 == 0) linv[w][half] = lt > 0.0f ? 1.0f / lt : 0.0f;
  }
  __syncthreads();
  for (int item = lane; item < 2 * NC; item += 64) {
    const int hr = item / NC, c4 = item % NC;
    const int rl = chunk * kMergeRows + 2 * w + hr;
    const int row = qg * kGroupRows + rl;
    if (row >= M) continue;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 8
    for (int sp = 0; sp < nu; ++sp) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(
          base + (static_cast<int64_t>(sp) * kGroupRows + rl) * LDSW + 4 * c4);
      acc += v * wsm[w][hr][sp];
    }
    const float inv = linv[w][hr];
    const int jh = row % a.rep, bt = row / a.rep;
    const int t = bt % a.T, b = bt / a.T;
    const int64_t tok = (static_cast<int64_t>(gi) * a.n_str + b) * a.T + t;
    bf16x4 v;
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = static_cast<__bf16>(acc[i] * inv);
    *reinterpret_cast<bf16x4*>(a.out + (tok * a.H + g * a.rep + jh) * D + 4 * c4) = v;
  }
  ATT_T(if (threadIdx.x == 0) { __builtin_amdgcn_s_waitcnt(0); att_at(6); })
}

// RoPE (half-rotation convention) + placement.  One thread per (token, head, pair i < D/2).
struct RopeParams {
  const __bf16* qkv;
  int64_t ldqkv;
  const float* part;        // rope_place_kernel<P, true>: fp32 K-split partials [splits][n_tok][ldqkv]
  int32_t splits;
  const float* inv_freq;
  const int32_t* plen;
  const int32_t* gpfx;
  const int32_t* hist_base;
  __bf16* q_out;
  __bf16* kh;
  __bf16* vth;
  int64_t ldh;
  int64_t n_tok;
  int32_t n_str, T, H, Hkv, D;
  int32_t skip_v;           // V placed by v_tile_place_kernel instead
  int32_t v_rows;           // V row-major like K ([S][Hkv][ldh][D], cs_rope_place_rows)
};

// n_split workgroups per token (kRopeItems (head, P-pair group) items each): the token's D/2
// angles' sincos into LDS, then every item of the workgroup (q, k rotated; v placed) by its
// own thread with 2P-byte loads / stores.  A decode step's few hundred tokens give over a
// thousand workgroups (one workgroup per token left most CUs with one: 18 us per C3 layer);
// a per-thread loop over the heads serialised one memory round trip per head.
constexpr int kRopeItems = 256;

// FOLD: the projection arrives as a K-split GEMM's unfolded fp32 partials (r.part), summed
// here in split order and rounded as cs_gemm_bf16's own fold would -- one launch and one
// bf16 round trip fewer per layer, bitwise the same q / K / V.  NSP splits' loads are issued
// together (surplus ones re-read the last split and are not summed): one memory round trip
// per NSP splits, not one per split.
template <int P, bool FOLD = false, int NSP = 1>
__global__ __launch_bounds__(256) void rope_place_kernel(RopeParams r, int32_t n_split) {
  typedef __bf16 vec_t __attribute__((ext_vector_type(P)));
  __shared__ float cs[128], sn[128];                // D / 2 <= 128
  const int half = r.D >> 1;
  const int nq = half / P;                          // P-pair groups per head
  const int nh = r.H + 2 * r.Hkv;
  const int64_t tok = blockIdx.x / n_split;
  const int split = static_cast<int>(blockIdx.x % n_split);
  const int64_t s = tok / r.T;
  const int t = static_cast<int>(tok % r.T);
  const int gi = static_cast<int>(s / r.n_str);
  const int p = r.gpfx ? r.gpfx[gi] : gi;
  const int slot = *r.hist_base + t;
  const float pos = static_cast<float>(r.plen[p] + slot);
  for (int i = threadIdx.x; i < half; i += 256) sincosf(pos * r.inv_freq[i], &sn[i], &cs[i]);
  __syncthreads();
  const __bf16* __restrict__ row = r.qkv + tok * r.ldqkv;
  __bf16* __restrict__ qo = r.q_out;
  __bf16* __restrict__ kh = r.kh;
  __bf16* __restrict__ vth = r.vth;
  const int lim = min(nh * nq, (split + 1) * kRopeItems);
  for (int item = split * kRopeItems + threadIdx.x; item < lim; item += 256) {
    const int hh = item / nq;
    const int i0 = P * (item - hh * nq);
    vec_t a, b;
    if constexpr (FOLD) {
      const int64_t off = tok * r.ldqkv + static_cast<int64_t>(hh) * r.D + i0;
      const int64_t sstride = r.n_tok * r.ldqkv;
      float fa[P], fb[P];
      for (int c0 = 0; c0 < r.splits; c0 += NSP) {
        f32x4 la[NSP][P / 4], lb[NSP][P / 4];
#pragma unroll
        for (int j = 0; j < NSP; ++j) {
          const int sp = min(c0 + j, r.splits - 1);
#pragma unroll
          for (int e = 0; e < P; e += 4) {
            la[j][e / 4] = *reinterpret_cast<const f32x4*>(r.part + sp * sstride + off + e);
            lb[j][e / 4] = *reinterpret_cast<const f32x4*>(r.part + sp * sstride + off + half + e);
          }
        }
        __builtin_amdgcn_sched_barrier(0);   // every load of the chunk issued before the sums
#pragma unroll
        for (int j = 0; j < NSP; ++j) {
          const bool first = c0 + j == 0, use = c0 + j < r.splits;
#pragma unroll
          for (int e = 0; e < P; e += 4)
#pragma unroll
            for (int c = 0; c < 4; ++c) {
              const float xa = la[j][e / 4][c], xb = lb[j][e / 4][c];
              fa[e + c] = first ? xa : (use ? fa[e + c] + xa : fa[e + c]);
              fb[e + c] = first ? xb : (use ? fb[e + c] + xb : fb[e + c]);
            }
        }
      }
#pragma unroll
      for (int e = 0; e < P; ++e) {
        a[e] = to_bf16(fa[e]);
        b[e] = to_bf16(fb[e]);
      }
    } else {
      const __bf16* src = row + static_cast<int64_t>(hh) * r.D + i0;
      a = *reinterpret_cast<const vec_t*>(src);
      b = *reinterpret_cast<const vec_t*>(src + half);
    }
    if (hh >= r.H + r.Hkv) {                         // v: transposed placement, no rotation
      if (r.skip_v) continue;
      const int g = hh - r.H - r.Hkv;
      if (r.v_rows) {
        __bf16* dst = vth + ((s * r.Hkv + g) * r.ldh + slot) * r.D;
        *reinterpret_cast<vec_t*>(dst + i0) = a;
        *reinterpret_cast<vec_t*>(dst + half + i0) = b;
        continue;
      }
      __bf16* dst = vth + ((s * r.Hkv + g) * r.ldh + (slot & ~31)) * r.D +
                    static_cast<int64_t>(i0) * 32 + (slot & 31);
#pragma unroll
      for (int e = 0; e < P; ++e) {
        dst[e * 32] = a[e];
        dst[(half + e) * 32] = b[e];
      }
      continue;
    }
    vec_t y1, y2;
#pragma unroll
    for (int e = 0; e < P; ++e) {
      const float x1 = static_cast<float>(a[e]), x2 = static_cast<float>(b[e]);
      y1[e] = static_cast<__bf16>(fmaf(x1, cs[i0 + e], -x2 * sn[i0 + e]));
      y2[e] = static_cast<__bf16>(fmaf(x2, cs[i0 + e], x1 * sn[i0 + e]));
    }
    __bf16* dst = hh < r.H ? qo + (tok * r.H + hh) * r.D
                           : kh + ((s * r.Hkv + (hh - r.H)) * r.ldh + slot) * r.D;
    *reinterpret_cast<vec_t*>(dst + i0) = y1;
    *reinterpret_cast<vec_t*>(dst + half + i0) = y2;
  }
}

// Multi-token streams (T >= 32: scoring chunks, prompt prefill): V placed by 32-slot tiles,
// one workgroup per (stream, K/V head, slot tile): the tile's tokens' V rows (16-byte loads)
// into LDS, then the tile's D rows of 32 slots written with 16-byte stores — the per-token
// placement of rope_place_kernel writes 2-byte pieces 64 B apart, from workgroups on every
// XCD.  Slots outside [hist_base, hist_base + T) are left as they are.
__global__ __launch_bounds__(256) void v_tile_place_kernel(RopeParams r, int32_t n_tiles) {
  __shared__ __attribute__((aligned(16))) __bf16 tile[32][256 + 8];   // [slot][d], D <= 256
  const int D = r.D;
  const int tid = threadIdx.x;
  const int c = static_cast<int>(blockIdx.x % n_tiles);
  const int64_t sg = blockIdx.x / n_tiles;            // s * Hkv + g
  const int g = static_cast<int>(sg % r.Hkv);
  const int64_t s = sg / r.Hkv;
  const int hb = *r.hist_base;
  const int slot0 = 32 * c;
  if (slot0 + 32 <= hb || slot0 >= hb + r.T) return;  // no token of this stream lands here
  const int dch = D >> 3;                              // 16-byte chunks per V row
  for (int ch = tid; ch < 32 * dch; ch += 256) {
    const int sl = ch / dch, dc = ch - sl * dch;
    const int t = slot0 + sl - hb;
    u32x4 v = {0u, 0u, 0u, 0u};
    if (t >= 0 && t < r.T)
      v = *reinterpret_cast<const u32x4*>(r.qkv + (s * r.T + t) * r.ldqkv +
                                          static_cast<int64_t>(r.H + r.Hkv + g) * D + dc * 8);
    *reinterpret_cast<u32x4*>(&tile[sl][dc * 8]) = v;
  }
  __syncthreads();
  __bf16* base = r.vth + ((s * r.Hkv + g) * r.ldh + slot0) * D;   // the tile's [D][32]
  for (int ch = tid; ch < 4 * D; ch += 256) {
    const int d = ch >> 2, q = ch & 3;
    bf16x8 v;
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = tile[q * 8 + e][d];
    const int t0 = slot0 + q * 8 - hb;
    __bf16* dst = base + d * 32 + q * 8;
    if (t0 >= 0 && t0 + 8 <= r.T) {
      *reinterpret_cast<bf16x8*>(dst) = v;
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e)
        if (t0 + e >= 0 && t0 + e < r.T) dst[e] = v[e];
    }
  }
}

// Row-layout history (cs_hist_rows_update): stream s inherits its parent's slots by table,
// dst[s][j] = src[parent[s]][j] for j < hist_base, and owns the rest (dst[s][j] = row_base +
// s: the slots this step and later ones write into its own row).  One thread per (s, j).
__global__ __launch_bounds__(256) void hist_rows_kernel(const int32_t* __restrict__ src,
                                                        int32_t* __restrict__ dst,
                                                        const int64_t* __restrict__ parent,
                                                        const int32_t* __restrict__ hist_base,
                                                        int64_t S, int32_t ldh, int64_t row_base) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (i >= S * ldh) return;
  const int64_t s = i / ldh;
  const int j = static_cast<int>(i - s * ldh);
  dst[i] = j < *hist_base ? src[parent[s] * ldh + j] : static_cast<int32_t>(row_base + s);
}

struct PlanCell {
  int32_t gi, qg, splits, per_wg;
};

}  // namespace

extern "C" {

int64_t cs_prefix_attention_plan(const int32_t* prefix_len, int32_t n_prefix,
                                 const int32_t* group_prefix, int32_t n_groups, int32_t n_str,
                                 int32_t T, int32_t H, int32_t Hkv, int32_t D, int64_t ld_hist,
                                 int32_t* plan, int64_t plan_cap, int32_t* n_attn, int32_t* n_merge,
                                 size_t* workspace_bytes) {
  if (n_attn) *n_attn = 0;
  if (n_merge) *n_merge = 0;
  if (workspace_bytes) *workspace_bytes = 0;
  if (n_groups < 0 || n_str < 0 || T < 0 || n_prefix < 0)
    return fail(CS_ERR_INVALID, "cs_prefix_attention_plan: negative size");
  if (n_groups == 0 || n_str == 0 || T == 0) return 0;
  if (!prefix_len || Hkv <= 0 || H <= 0 || H % Hkv != 0 || ld_hist <= 0 || ld_hist % kKeyBlock != 0 ||
      (D != 64 && D != 128 && D != 256))
    return fail(CS_ERR_INVALID, "cs_prefix_attention_plan: bad shape");
  const int64_t rep = H / Hkv;
  const int64_t M = static_cast<int64_t>(n_str) * T * rep;
  const int64_t n_qg = (M + kGroupRows - 1) / kGroupRows;
  const int64_t base = static_cast<int64_t>(n_groups) * Hkv * n_qg;
  // enough workgroups without key splits -- unless (single-token streams) some cells are
  // far longer than the rest: a lookahead tree level whose reference prompt lists every
  // opinion (thousands of keys) beside ~250-key agent prompts makes the reference cells
  // the launch's long pole (cells checked below)
  if (base >= kPlanMinBase && T > 1) return 0;
  const int64_t nbh_max = ld_hist / kKeyBlock;
  // every cell's key blocks per query tile (an upper bound: history at capacity)
  struct Cell { int32_t gi, qg; int64_t items, kw, nrows; };
  std::vector<Cell> cl;
  cl.reserve(static_cast<size_t>(n_groups * n_qg));
  for (int32_t gi = 0; gi < n_groups; ++gi) {
    const int32_t p = group_prefix ? group_prefix[gi] : gi;
    if (p < 0 || p >= n_prefix || prefix_len[p] < 0)
      return fail(CS_ERR_INVALID, "cs_prefix_attention_plan: group_prefix / prefix_len out of range");
    const int64_t nbp = (prefix_len[p] + kKeyBlock - 1) / kKeyBlock;
    for (int64_t qg = 0; qg < n_qg; ++qg) {
      const int64_t r0 = qg * kGroupRows;
      const int64_t nrows = std::min<int64_t>(kGroupRows, M - r0);
      const int64_t n_qt = (nrows + 15) / 16;
      const int64_t kw = n_qt == 1 ? 4 : (n_qt == 2 ? 2 : 1);
      int64_t items = 0;
      for (int64_t q = 0; q < n_qt; ++q) {
        const int64_t rt0 = r0 + 16 * q, rt1 = std::min(rt0 + 15, M - 1);
        const int64_t streams = (rt1 / rep) / T - (rt0 / rep) / T + 1;
        items = std::max(items, nbp + streams * nbh_max);
      }
      cl.push_back({gi, static_cast<int32_t>(qg), items, kw, nrows});
    }
  }
  if (base >= kPlanMinBase) {
    int64_t sum = 0, mx = 0;
    for (const Cell& c : cl) {
      sum += c.items;
      mx = std::max(mx, c.items);
    }
    if (mx * static_cast<int64_t>(cl.size()) <= kPlanImbalance * sum) return 0;
  }
  // one per-wave budget q for all cells (a cell of `items` blocks on kw waves takes
  // ceil(items / (q kw)) splits, at most kMaxSplit): the whole launch's wave-serial work
  // spread over about kPlanTargetWgs workgroups, never below kPlanMinItems blocks per
  // wave — so the split workgroups are about equally long and no cell is the long pole
  auto splits_of = [](const Cell& c, int64_t q) {
    return std::max<int64_t>(1, std::min<int64_t>(kMaxSplit, (c.items + q * c.kw - 1) / (q * c.kw)));
  };
  int64_t work = 0;
  for (const Cell& c : cl) work += (c.items + c.kw - 1) / c.kw;
  work *= Hkv;
  const int64_t q = std::max<int64_t>(kPlanMinItems, (work + kPlanTargetWgs - 1) / kPlanTargetWgs);
  std::vector<PlanCell> cells;
  cells.reserve(cl.size());
  int64_t na = 0, nm = 0, slots = 0;
  for (const Cell& c : cl) {
    const int64_t s = splits_of(c, q);
    const int64_t per = (c.items + s * c.kw - 1) / (s * c.kw);
    cells.push_back({c.gi, c.qg, static_cast<int32_t>(s), static_cast<int32_t>(per)});
    na += s * Hkv;
    if (s > 1) {
      slots += s * Hkv;
      nm += (c.nrows + kMergeRows - 1) / kMergeRows * Hkv;
    }
  }
  if (nm == 0) return 0;   // no cell splits: the plain grid
  if (na + nm > 0x7fffffffLL) return fail(CS_ERR_INVALID, "cs_prefix_attention_plan: plan too large");
  if (n_attn) *n_attn = static_cast<int32_t>(na);
  if (n_merge) *n_merge = static_cast<int32_t>(nm);
  if (workspace_bytes) *workspace_bytes = static_cast<size_t>(slots) * kGroupRows * (D + 2) * sizeof(float);
  const int64_t total = na + nm;
  if (!plan) return total;
  if (plan_cap < total) return fail(CS_ERR_INVALID, "cs_prefix_attention_plan: plan_cap too small");
  // the longest workgroups first (dispatched first: the tail of the launch is short ones)
  std::stable_sort(cells.begin(), cells.end(),
                   [](const PlanCell& x, const PlanCell& y) { return x.per_wg > y.per_wg; });
  int32_t* pa = plan;
  int32_t* pm = plan + 4 * na;
  int32_t slot = 0;
  for (const PlanCell& c : cells) {
    const int64_t r0 = static_cast<int64_t>(c.qg) * kGroupRows;
    const int64_t nrows = std::min<int64_t>(kGroupRows, M - r0);
    for (int32_t g = 0; g < Hkv; ++g) {
      const int32_t pg = c.gi * Hkv + g;
      for (int32_t sp = 0; sp < c.splits; ++sp) {
        pa[0] = pg;
        pa[1] = c.qg;
        pa[2] = sp | (c.splits << 8);
        pa[3] = c.splits > 1 ? slot + sp : 0;
        pa += 4;
      }
      if (c.splits > 1) {
        for (int32_t ch = 0; ch < (nrows + kMergeRows - 1) / kMergeRows; ++ch) {
          pm[0] = pg;
          pm[1] = c.qg;
          pm[2] = slot;
          pm[3] = ch | (c.splits << 8);
          pm += 4;
        }
        slot += c.splits;
      }
    }
  }
  return total;
}

}  // extern "C"

namespace {
// hist_rows == nullptr: cs_prefix_attention (V^T tiles); else cs_prefix_attention_rows
int prefix_attention_impl(const char* name, const void* q, const void* k_prefix, const void* vt_prefix,
                          int64_t ld_prefix, const int64_t* prefix_off, const int32_t* prefix_len,
                          int32_t max_prefix_len, const int32_t* group_prefix, int32_t n_groups,
                          const void* k_hist, const void* vt_hist, const int32_t* hist_rows,
                          int64_t ld_hist, const int32_t* hist_base, int32_t n_str, int32_t T,
                          int32_t H, int32_t Hkv, int32_t D, float scale, float softcap,
                          int32_t window, const void* plan, int32_t n_attn, int32_t n_merge,
                          void* out, void* workspace, size_t workspace_bytes, cs_stream_t stream) {
  const std::string nm(name);
  if (n_groups < 0 || n_str < 0 || T < 0) return fail(CS_ERR_INVALID, nm + ": negative size");
  if (n_groups == 0 || n_str == 0 || T == 0) return CS_OK;
  if (Hkv <= 0 || H <= 0 || H % Hkv != 0 || H / Hkv > 64)
    return fail(CS_ERR_INVALID, nm + ": H must be a multiple of Hkv (<= 64 per group)");
  if (D != 64 && D != 128 && D != 256)
    return fail(CS_ERR_INVALID, nm + ": head_dim must be 64, 128 or 256");
  if (ld_prefix <= 0 || ld_prefix % kKeyBlock != 0 || ld_hist <= 0 || ld_hist % kKeyBlock != 0)
    return fail(CS_ERR_INVALID, nm + ": ld_prefix / ld_hist must be positive multiples of 32");
  if (max_prefix_len < 0 || max_prefix_len > ld_prefix)
    return fail(CS_ERR_INVALID, nm + ": max_prefix_len outside [0, ld_prefix]");
  if (!q || !k_prefix || !vt_prefix || !prefix_off || !prefix_len || !k_hist || !vt_hist ||
      !hist_base || !out || (hist_rows == nullptr) != (nm == "cs_prefix_attention"))
    return fail(CS_ERR_INVALID, nm + ": NULL pointer");
  if (!(scale > 0.0f) || softcap < 0.0f) return fail(CS_ERR_INVALID, nm + ": bad scale / softcap");
  if (plan && (n_attn <= 0 || n_merge <= 0))
    return fail(CS_ERR_INVALID, nm + ": a plan needs n_attn > 0 and n_merge > 0");
  if (plan && !workspace)
    return fail(CS_ERR_WORKSPACE, nm + ": a plan needs the workspace cs_prefix_attention_plan() sized");
  const int64_t M = static_cast<int64_t>(n_str) * T * (H / Hkv);
  const int64_t n_qg = (M + kGroupRows - 1) / kGroupRows;
  const int64_t base = static_cast<int64_t>(n_groups) * Hkv * n_qg;
  if (n_qg > 0x7fffffff || base > 0x7fffffffLL) return fail(CS_ERR_INVALID, nm + ": too many query rows");
  AttnParams a;
  a.q = static_cast<const __bf16*>(q);
  a.kp = static_cast<const __bf16*>(k_prefix);
  a.vtp = static_cast<const __bf16*>(vt_prefix);
  a.poff = prefix_off;
  a.plen = prefix_len;
  a.gpfx = group_prefix;
  a.kh = static_cast<const __bf16*>(k_hist);
  a.vth = static_cast<const __bf16*>(vt_hist);
  a.hist_base = hist_base;
  a.hrow = hist_rows;
  a.out = static_cast<__bf16*>(out);
  a.part = static_cast<float*>(workspace);
  a.plan = static_cast<const int4*>(plan);
  a.ldp = ld_prefix;
  a.ldh = ld_hist;
  a.n_grp = n_groups;
  a.n_str = n_str;
  a.T = T;
  a.H = H;
  a.Hkv = Hkv;
  a.rep = H / Hkv;
  a.n_qg = static_cast<int32_t>(n_qg);
  a.n_attn = plan ? n_attn : 0;
  a.scale = scale;
  a.softcap = softcap;
  a.inv_softcap = softcap > 0.0f ? 1.0f / softcap : 0.0f;
  a.window = window > 0 ? window : 0;
  (void)workspace_bytes;   // sized by cs_prefix_attention_plan for this plan
  const int64_t nwg = plan ? n_attn : base;
  a.swizzle = (!plan && nwg % 8 == 0 && nwg >= 64) ? 1 : 0;
  hipStream_t st = static_cast<hipStream_t>(stream);
  // scoring chunks and prefill at D = 128 (T >= 32: the line model.forward_streams draws
  // between them and decode), no soft-cap, no window, whole tokens per 32-row tile: the wide
  // tile.  A pure function of the arguments; everything else launches as before
  if (!plan && !hist_rows && D == 128 && softcap == 0.0f && a.window == 0 && 32 % a.rep == 0 && T >= 32) {
    constexpr int kRows = 32 * kWideWaves;
    const int64_t n_wg = (M + kRows - 1) / kRows;
    const int64_t nw = static_cast<int64_t>(n_groups) * Hkv * n_wg;
    a.n_qg = static_cast<int32_t>(n_wg);
    a.swizzle = (nw % 8 == 0 && nw >= 64) ? 1 : 0;
    hipLaunchKernelGGL((prefix_attn_wide_kernel<128, kWideWaves>), dim3(static_cast<uint32_t>(nw)),
                       dim3(64 * kWideWaves), 0, st, a);
    return check_launch(name);
  }
  const dim3 grid(static_cast<uint32_t>(nwg));
  const dim3 merge_grid(static_cast<uint32_t>(plan ? n_merge : 0));
#define CS_ATTN_LAUNCH(DV)                                                              \
  do {                                                                                  \
    if (hist_rows)                                                                      \
      hipLaunchKernelGGL((prefix_attn_plan_lds_kernel<DV, true>), grid, dim3(kAttnThreads), 0, st, a); \
    else if (plan)                                                                      \
      hipLaunchKernelGGL(prefix_attn_plan_lds_kernel<DV>, grid, dim3(kAttnThreads), 0, st, a); \
    else                                                                                \
      hipLaunchKernelGGL(prefix_attn_lds_kernel<DV>, grid, dim3(kAttnThreads), 0, st, a); \
    if (plan)                                                                           \
      hipLaunchKernelGGL(attn_merge_kernel<DV>, merge_grid, dim3(kAttnThreads), 0, st, a); \
  } while (0)
  if (D == 64) {
    CS_ATTN_LAUNCH(64);
  } else if (D == 128) {
    CS_ATTN_LAUNCH(128);
  } else {
    CS_ATTN_LAUNCH(256);
  }
#undef CS_ATTN_LAUNCH
  return check_launch(name);
}
}  // namespace

extern "C" {

int cs_prefix_attention(const void* q, const void* k_prefix, const void* vt_prefix,
                        int64_t ld_prefix, const int64_t* prefix_off, const int32_t* prefix_len,
                        int32_t max_prefix_len, const int32_t* group_prefix, int32_t n_groups,
                        const void* k_hist, const void* vt_hist, int64_t ld_hist,
                        const int32_t* hist_base, int32_t n_str, int32_t T, int32_t H, int32_t Hkv,
                        int32_t D, float scale, float softcap, int32_t window, const void* plan,
                        int32_t n_attn, int32_t n_merge, void* out, void* workspace,
                        size_t workspace_bytes, cs_stream_t stream) {
  return prefix_attention_impl("cs_prefix_attention", q, k_prefix, vt_prefix, ld_prefix, prefix_off,
                               prefix_len, max_prefix_len, group_prefix, n_groups, k_hist, vt_hist,
                               nullptr, ld_hist, hist_base, n_str, T, H, Hkv, D, scale, softcap,
                               window, plan, n_attn, n_merge, out, workspace, workspace_bytes, stream);
}

int cs_prefix_attention_rows(const void* q, const void* k_prefix, const void* vt_prefix,
                             int64_t ld_prefix, const int64_t* prefix_off, const int32_t* prefix_len,
                             int32_t max_prefix_len, const int32_t* group_prefix, int32_t n_groups,
                             const void* k_hist, const void* v_hist, const int32_t* hist_rows,
                             int64_t ld_hist, const int32_t* hist_base, int32_t n_str, int32_t T,
                             int32_t H, int32_t Hkv, int32_t D, float scale, float softcap,
                             int32_t window, const void* plan, int32_t n_attn, int32_t n_merge,
                             void* out, void* workspace, size_t workspace_bytes, cs_stream_t stream) {
  if (!hist_rows) return fail(CS_ERR_INVALID, "cs_prefix_attention_rows: NULL hist_rows");
  return prefix_attention_impl("cs_prefix_attention_rows", q, k_prefix, vt_prefix, ld_prefix,
                               prefix_off, prefix_len, max_prefix_len, group_prefix, n_groups,
                               k_hist, v_hist, hist_rows, ld_hist, hist_base, n_str, T, H, Hkv, D,
                               scale, softcap, window, plan, n_attn, n_merge, out, workspace,
                               workspace_bytes, stream);
}

#ifdef CS_TRACE_ATTN
// diagnostics build only: copy the per-workgroup timestamps [kAttTraceWgs][8] and clear them
int cs_attn_trace_read(unsigned long long* out) {
  (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_attn_ts), sizeof(g_attn_ts));
  static unsigned long long zero[kAttTraceWgs][8];
  (void)hipMemcpyToSymbol(HIP_SYMBOL(g_attn_ts), zero, sizeof(zero));
  return 0;
}
#endif

int cs_hist_rows_update(const int32_t* src_rows, int32_t* dst_rows, const int64_t* parent,
                        const int32_t* hist_base, int64_t S, int32_t ld_hist, int64_t row_base,
                        int64_t n_rows, cs_stream_t stream) {
  if (S < 0 || ld_hist <= 0 || row_base < 0) return fail(CS_ERR_INVALID, "cs_hist_rows_update: bad shape");
  if (row_base + S > n_rows)
    return fail(CS_ERR_INVALID, "cs_hist_rows_update: rows row_base .. row_base + S - 1 exceed the buffer's n_rows");
  if (S == 0) return CS_OK;
  if (!src_rows || !dst_rows || !parent || !hist_base)
    return fail(CS_ERR_INVALID, "cs_hist_rows_update: NULL pointer");
  if (src_rows == dst_rows) return fail(CS_ERR_INVALID, "cs_hist_rows_update: source and destination must differ");
  if (S > 0x7fffffffLL || row_base + S > 0x7fffffffLL || (S * ld_hist + 255) / 256 > 0x7fffffffLL)
    return fail(CS_ERR_INVALID, "cs_hist_rows_update: table too large");
  hipLaunchKernelGGL(hist_rows_kernel, dim3(static_cast<uint32_t>((S * ld_hist + 255) / 256)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), src_rows, dst_rows, parent, hist_base, S, ld_hist,
                     row_base);
  return check_launch("cs_hist_rows_update");
}

}  // extern "C"

namespace {
// `name`: the entry point that was called, for the messages
int rope_place_impl(const char* name, const void* qkv, int64_t ld_qkv, const float* part,
                    int32_t splits, const float* inv_freq, const int32_t* prefix_len,
                    const int32_t* group_prefix, int32_t n_groups, const int32_t* hist_base,
                    int32_t n_str, int32_t T, int32_t H, int32_t Hkv, int32_t D, void* q_out,
                    void* k_hist, void* vt_hist, int64_t ld_hist, int32_t v_rows, cs_stream_t stream) {
  const std::string nm(name);
  if (n_groups < 0 || n_str < 0 || T < 0) return fail(CS_ERR_INVALID, nm + ": negative size");
  if (n_groups == 0 || n_str == 0 || T == 0) return CS_OK;
  if (H <= 0 || Hkv <= 0 || D <= 0 || D % 2 != 0 || ld_qkv < static_cast<int64_t>(H + 2 * Hkv) * D)
    return fail(CS_ERR_INVALID, nm + ": bad head layout");
  if (ld_hist < T) return fail(CS_ERR_INVALID, nm + ": ld_hist < T");
  if (!inv_freq || !prefix_len || !hist_base || !q_out || !k_hist || !vt_hist)
    return fail(CS_ERR_INVALID, nm + ": NULL pointer");
  // the blocked V layout is whole 32-slot tiles per head: another ld_hist would put a head's
  // last slots into the next head's first tile
  if (!v_rows && ld_hist % 32 != 0)
    return fail(CS_ERR_INVALID, nm + ": ld_hist must be a multiple of 32 (V^T tiles)");
  // 16-byte stores to the outputs; the 4-pair items' 8-byte loads of the projection
  if (reinterpret_cast<uintptr_t>(q_out) % 16 || reinterpret_cast<uintptr_t>(k_hist) % 16 ||
      reinterpret_cast<uintptr_t>(vt_hist) % 16)
    return fail(CS_ERR_INVALID, nm + ": q_out, k_hist and vt_hist must be 16-byte aligned");
  if (!part && (reinterpret_cast<uintptr_t>(qkv) % 8 || ld_qkv % 4 != 0))
    return fail(CS_ERR_INVALID, nm + ": qkv must be 8-byte aligned, ld_qkv a multiple of 4");
  RopeParams r;
  r.qkv = static_cast<const __bf16*>(qkv);
  r.ldqkv = ld_qkv;
  r.part = part;
  r.splits = splits;
  r.inv_freq = inv_freq;
  r.plen = prefix_len;
  r.gpfx = group_prefix;
  r.hist_base = hist_base;
  r.q_out = static_cast<__bf16*>(q_out);
  r.kh = static_cast<__bf16*>(k_hist);
  r.vth = static_cast<__bf16*>(vt_hist);
  r.ldh = ld_hist;
  r.v_rows = v_rows;
  r.n_tok = static_cast<int64_t>(n_groups) * n_str * T;
  r.n_str = n_str;
  r.T = T;
  r.H = H;
  r.Hkv = Hkv;
  r.D = D;
  if (D % 8 != 0 || D > 256) return fail(CS_ERR_INVALID, nm + ": head_dim must be a multiple of 8, <= 256");
  if (r.n_tok > 0x7fffffffLL) return fail(CS_ERR_INVALID, nm + ": too many tokens");
  // V by 32-slot tiles when the streams carry many tokens
  const int64_t n_tiles = ld_hist / 32;
  const int64_t n_vwg = static_cast<int64_t>(n_groups) * n_str * Hkv * n_tiles;
  r.skip_v = (!part && !v_rows && T >= 32 && ld_qkv % 8 == 0 &&
              reinterpret_cast<uintptr_t>(qkv) % 16 == 0 && n_vwg <= 0x7fffffffLL) ? 1 : 0;
  // 8-pair (16-byte) items when every head's halves are 16-byte aligned, else 4-pair
  const bool p8 = part ? true
                       : (ld_qkv % 8 == 0 && reinterpret_cast<uintptr_t>(qkv) % 16 == 0 && D % 16 == 0);
  const int64_t n_items = static_cast<int64_t>(H + 2 * Hkv) * (D / 2) / (p8 ? 8 : 4);
  const int64_t n_split = (n_items + kRopeItems - 1) / kRopeItems;
  if (r.n_tok * n_split > 0x7fffffffLL) return fail(CS_ERR_INVALID, nm + ": too many tokens");
  const dim3 grid(static_cast<uint32_t>(r.n_tok * n_split));
  if (part && splits <= 2)
    hipLaunchKernelGGL((rope_place_kernel<8, true, 2>), grid, dim3(256), 0, static_cast<hipStream_t>(stream),
                       r, static_cast<int32_t>(n_split));
  else if (part && splits <= 4)
    hipLaunchKernelGGL((rope_place_kernel<8, true, 4>), grid, dim3(256), 0, static_cast<hipStream_t>(stream),
                       r, static_cast<int32_t>(n_split));
  else if (part)
    hipLaunchKernelGGL((rope_place_kernel<8, true, 8>), grid, dim3(256), 0, static_cast<hipStream_t>(stream),
                       r, static_cast<int32_t>(n_split));
  else if (p8)
    hipLaunchKernelGGL(rope_place_kernel<8>, grid, dim3(256), 0, static_cast<hipStream_t>(stream), r,
                       static_cast<int32_t>(n_split));
  else
    hipLaunchKernelGGL(rope_place_kernel<4>, grid, dim3(256), 0, static_cast<hipStream_t>(stream), r,
                       static_cast<int32_t>(n_split));
  if (r.skip_v)
    hipLaunchKernelGGL(v_tile_place_kernel, dim3(static_cast<uint32_t>(n_vwg)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), r, static_cast<int32_t>(n_tiles));
  return check_launch(name);
}

// the checks the two split-K entry points share (`name`: the entry point's, for the messages)
int rope_place_splitk_impl(const char* name, const float* part, int32_t splits, const float* inv_freq,
                           const int32_t* prefix_len, const int32_t* group_prefix, int32_t n_groups,
                           const int32_t* hist_base, int32_t n_str, int32_t T, int32_t H, int32_t Hkv,
                           int32_t D, void* q_out, void* k_hist, void* vt_hist, int64_t ld_hist,
                           int32_t v_rows, cs_stream_t stream) {
  const std::string nm(name);
  if (!part || splits < 1) return fail(CS_ERR_INVALID, nm + ": need partials, splits >= 1");
  if (T >= 32) return fail(CS_ERR_INVALID, nm + ": T < 32 only (fold first for chunks)");
  if (reinterpret_cast<uintptr_t>(part) % 16 || D % 16)
    return fail(CS_ERR_INVALID, nm + ": partials 16-byte aligned, head_dim % 16 == 0");
  return rope_place_impl(name, nullptr, static_cast<int64_t>(H + 2 * Hkv) * D, part, splits, inv_freq,
                         prefix_len, group_prefix, n_groups, hist_base, n_str, T, H, Hkv, D, q_out,
                         k_hist, vt_hist, ld_hist, v_rows, stream);
}
}  // namespace

extern "C" {

int cs_rope_place(const void* qkv, int64_t ld_qkv, const float* inv_freq, const int32_t* prefix_len,
                  const int32_t* group_prefix, int32_t n_groups, const int32_t* hist_base,
                  int32_t n_str, int32_t T, int32_t H, int32_t Hkv, int32_t D, void* q_out,
                  void* k_hist, void* vt_hist, int64_t ld_hist, cs_stream_t stream) {
  if (!qkv) return fail(CS_ERR_INVALID, "cs_rope_place: NULL pointer");
  return rope_place_impl("cs_rope_place", qkv, ld_qkv, nullptr, 1, inv_freq, prefix_len, group_prefix,
                         n_groups, hist_base, n_str, T, H, Hkv, D, q_out, k_hist, vt_hist, ld_hist, 0,
                         stream);
}

int cs_rope_place_rows(const void* qkv, int64_t ld_qkv, const float* inv_freq,
                       const int32_t* prefix_len, const int32_t* group_prefix, int32_t n_groups,
                       const int32_t* hist_base, int32_t n_str, int32_t T, int32_t H, int32_t Hkv,
                       int32_t D, void* q_out, void* k_hist, void* v_hist, int64_t ld_hist,
                       cs_stream_t stream) {
  if (!qkv) return fail(CS_ERR_INVALID, "cs_rope_place_rows: NULL pointer");
  return rope_place_impl("cs_rope_place_rows", qkv, ld_qkv, nullptr, 1, inv_freq, prefix_len,
                         group_prefix, n_groups, hist_base, n_str, T, H, Hkv, D, q_out, k_hist, v_hist,
                         ld_hist, 1, stream);
}

int cs_rope_place_splitk(const float* part, int32_t splits, const float* inv_freq,
                         const int32_t* prefix_len, const int32_t* group_prefix, int32_t n_groups,
                         const int32_t* hist_base, int32_t n_str, int32_t T, int32_t H,
                         int32_t Hkv, int32_t D, void* q_out, void* k_hist, void* vt_hist,
                         int64_t ld_hist, cs_stream_t stream) {
  return rope_place_splitk_impl("cs_rope_place_splitk", part, splits, inv_freq, prefix_len,
                                group_prefix, n_groups, hist_base, n_str, T, H, Hkv, D, q_out,
                                k_hist, vt_hist, ld_hist, 0, stream);
}

int cs_rope_place_splitk_rows(const float* part, int32_t splits, const float* inv_freq,
                              const int32_t* prefix_len, const int32_t* group_prefix,
                              int32_t n_groups, const int32_t* hist_base, int32_t n_str, int32_t T,
                              int32_t H, int32_t Hkv, int32_t D, void* q_out, void* k_hist,
                              void* v_hist, int64_t ld_hist, cs_stream_t stream) {
  return rope_place_splitk_impl("cs_rope_place_splitk_rows", part, splits, inv_freq, prefix_len,
                                group_prefix, n_groups, hist_base, n_str, T, H, Hkv, D, q_out,
                                k_hist, v_hist, ld_hist, 1, stream);
}

}  // extern "C"

// ---------------------------------------------------------------------------------------
// encoder_attn_kernel -- bidirectional softmax attention of the text encoder (encoder.hip)
// over a ragged batch: text t is tokens cu[t] .. cu[t + 1] - 1 of the fused projection
// qkv [n_tok][3 H 64] (q | k | v, each [H][64], K AND V row-major as in the rows route), and
// a token sees every key of its own text and none of another's.  One workgroup per (text,
// head, 64-query tile) walks the text's 32-key blocks, each staged through LDS once for the
// workgroup's four 16-query tiles, double-buffered as CS_ATTEND_STAGED does it.
//
// From the shared pieces: LdsTile (the padded K / V^T buffers), mine_staged, attend_staged
// (so attend_block: the arithmetic, mask and lazy rescale are the decoders'), combine_waves
// (a text of <= 32 queries gives its tile's key blocks to 2 or 4 waves) and store_out.  Its
// own: the TileRows it fills (tile_rows derives a row from the group / stream / GQA layout,
// a ragged text has none), the Q load (load_q takes q [n_tok][H][D]; here Q sits inside the
// fused row at another pitch) and the staging (fetch_chunks / stage_chunks copy a block that
// is contiguous, whole, and already V^T; here the rows are 3 H 64 apart, the keys past the
// text's end are another text's and must not be read -- they are staged as zeros, so the
// output cannot depend on a neighbour, NaN included -- and V is transposed on its way in).
namespace {

struct EncAttnParams {
  const __bf16* qkv;
  int64_t ldqkv;
  const int32_t* cu;
  __bf16* out;
  int64_t n_tok;
  int32_t n_text, H, n_qt, max_len;   // n_qt: 64-query tiles of the longest text
  float scale;
};

constexpr int kEncD = 64;

// this thread's 16-byte chunk of key block kb: key tid / 8, d 8 (tid % 8) .. + 7 of K and of V
// (zeros past the text's end)
__device__ __forceinline__ void enc_fetch(const __bf16* kbase, int64_t ld, int kb, int len, u32x4& rk,
                                          u32x4& rv, int H) {
  const int key = kb + (static_cast<int>(threadIdx.x) >> 3);
  if (key < len) {
    const __bf16* p = kbase + key * ld + 8 * (threadIdx.x & 7);
    rk = *reinterpret_cast<const u32x4*>(p);
    rv = *reinterpret_cast<const u32x4*>(p + H * kEncD);
  } else {
    rk = u32x4{0u, 0u, 0u, 0u};
    rv = u32x4{0u, 0u, 0u, 0u};
  }
}

// ... into block j's buffer: the K chunk as it is, the V chunk's 8 d as 8 V^T rows
__device__ __forceinline__ void enc_stage(__bf16* buf, int j, const u32x4& rk, const u32x4& rv) {
  using LT = LdsTile<kEncD>;
  __bf16* kd = buf + (j & 1) * LT::ELEMS;
  uint16_t* vd = reinterpret_cast<uint16_t*>(kd + LT::KELEMS);
  const int key = static_cast<int>(threadIdx.x) >> 3, ch = threadIdx.x & 7;
  *reinterpret_cast<u32x4*>(kd + key * LT::KROW + 8 * ch) = rk;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const uint32_t wv = rv[e >> 1];
    vd[(8 * ch + e) * LT::VROW + key] = static_cast<uint16_t>((e & 1) ? (wv >> 16) : (wv & 0xffffu));
  }
}

__global__ __launch_bounds__(kAttnThreads, 2)
void encoder_attn_kernel(EncAttnParams e) {
  constexpr int D = kEncD;
  using LT = LdsTile<D>;
  __shared__ __attribute__((aligned(16))) char lds[LT::kBytes];
  const int bid = blockIdx.x;
  const int qtile = bid % e.n_qt;
  const int h = (bid / e.n_qt) % e.H;
  const int t = bid / (e.n_qt * e.H);
  const int64_t t0 = e.cu[t];
  const int64_t t1 = e.cu[t + 1];
  // a malformed cu_seqlens reads and writes nothing (workgroup-uniform, before any barrier)
  if (t0 < 0 || t1 <= t0 || t1 > e.n_tok || t1 - t0 > e.max_len) return;
  const int len = static_cast<int>(t1 - t0);
  const int q0 = qtile * kGroupRows;
  if (q0 >= len) return;

  AttnParams a = {};
  a.out = e.out;
  a.H = e.H;
  a.scale = e.scale;
  a.softcap = 0.0f;
  a.inv_softcap = 0.0f;

  TileRows tr = {};
  tr.M = len;
  tr.r0 = q0;
  tr.nrows = min(kGroupRows, len - q0);
  tr.n_qt = (tr.nrows + 15) >> 4;
  tr.kw = tr.n_qt == 1 ? 4 : (tr.n_qt == 2 ? 2 : 1);
  tr.w = threadIdx.x >> 6;
  tr.lane = threadIdx.x & 63;
  tr.qt = tr.w % tr.n_qt;
  tr.ks = tr.w / tr.n_qt;
  tr.active = tr.ks < tr.kw;
  tr.col = tr.lane & 15;
  tr.h4 = tr.lane >> 4;
  const int row = q0 + tr.qt * 16 + tr.col;
  tr.vrow = tr.active && row < len;
  tr.tok = t0 + (row < len ? row : len - 1);
  tr.head = h;
  tr.kmin_pos = INT32_MIN;

  bf16x8 qf[D / 32];
  {
    const __bf16* qrow = e.qkv + tr.tok * e.ldqkv + h * D + 8 * tr.h4;
#pragma unroll
    for (int ds = 0; ds < D / 32; ++ds) {
      if (tr.vrow) {
        qf[ds] = *reinterpret_cast<const bf16x8*>(qrow + ds * 32);
      } else {
#pragma unroll
        for (int i = 0; i < 8; ++i) qf[ds][i] = static_cast<__bf16>(0.0f);
      }
    }
  }
  f32x4 o[D / 16];
#pragma unroll
  for (int dt = 0; dt < D / 16; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m = -INFINITY, l = 0.0f;

  const int lim = tr.vrow ? len : 0;
  auto ref = [&](int j) {
    BlockRef r;
    r.k = nullptr;
    r.vt = nullptr;
    r.mask = BlockMask{j * kKeyBlock, lim, 0};
    return r;
  };
  const __bf16* kbase = e.qkv + t0 * e.ldqkv + (e.H + h) * D;
  const int n = (len + kKeyBlock - 1) / kKeyBlock;
  __bf16* buf = reinterpret_cast<__bf16*>(lds);
  u32x4 rk, rv;
  enc_fetch(kbase, e.ldqkv, 0, len, rk, rv, e.H);
  enc_stage(buf, 0, rk, rv);
  __syncthreads();
  for (int j = 0; j < n; ++j) {
    const bool more = j + 1 < n;
    if (more) enc_fetch(kbase, e.ldqkv, (j + 1) * kKeyBlock, len, rk, rv, e.H);
    if (mine_staged(tr, j)) attend_staged<D>(a, tr, buf, j, ref, qf, o, m, l);
    if (more) enc_stage(buf, j + 1, rk, rv);
    __syncthreads();
  }
  combine_waves<D>(tr, lds, o, m, l);
  if (tr.vrow && tr.ks == 0) store_out<D>(a, tr, o, l);
}

}  // namespace

extern "C" {

int cs_encoder_attention(const void* qkv, int64_t ld_qkv, const int32_t* cu_seqlens, int32_t n_text,
                         int64_t n_tok, int32_t max_seqlen, int32_t H, int32_t D, float scale,
                         void* out, cs_stream_t stream) {
  const std::string nm = "cs_encoder_attention";
  if (n_text < 0 || n_tok < 0 || max_seqlen < 0) return fail(CS_ERR_INVALID, nm + ": negative size");
  if (D != kEncD) return fail(CS_ERR_INVALID, nm + ": head_dim must be 64");
  if (H <= 0 || H > 1024) return fail(CS_ERR_INVALID, nm + ": H must be in 1 .. 1024");
  if (max_seqlen > 512) return fail(CS_ERR_INVALID, nm + ": texts of 1 .. 512 tokens");
  if (ld_qkv < static_cast<int64_t>(3) * H * D || ld_qkv % 8 != 0)
    return fail(CS_ERR_INVALID, nm + ": ld_qkv must be >= 3 H D and a multiple of 8");
  if (!(scale > 0.0f) || std::isinf(scale)) return fail(CS_ERR_INVALID, nm + ": bad scale");
  if (n_text == 0 || n_tok == 0 || max_seqlen == 0) return CS_OK;
  if (!qkv || !cu_seqlens || !out) return fail(CS_ERR_INVALID, nm + ": NULL pointer");
  if (reinterpret_cast<uintptr_t>(qkv) % 16 || reinterpret_cast<uintptr_t>(out) % 16)
    return fail(CS_ERR_INVALID, nm + ": qkv and out must be 16-byte aligned");
  if (n_tok > 0x7fffffffLL) return fail(CS_ERR_INVALID, nm + ": too many tokens");
  EncAttnParams e;
  e.qkv = static_cast<const __bf16*>(qkv);
  e.ldqkv = ld_qkv;
  e.cu = cu_seqlens;
  e.out = static_cast<__bf16*>(out);
  e.n_tok = n_tok;
  e.n_text = n_text;
  e.H = H;
  e.n_qt = (max_seqlen + kGroupRows - 1) / kGroupRows;
  e.max_len = max_seqlen;
  e.scale = scale;
  const int64_t nwg = static_cast<int64_t>(n_text) * H * e.n_qt;
  if (nwg > 0x7fffffffLL) return fail(CS_ERR_INVALID, nm + ": grid too large");
  hipLaunchKernelGGL(encoder_attn_kernel, dim3(static_cast<uint32_t>(nwg)), dim3(kAttnThreads), 0,
                     static_cast<hipStream_t>(stream), e);
  return check_launch("cs_encoder_attention");
}

}  // extern "C"
