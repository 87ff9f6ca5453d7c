// stream.hip — vocab-wide log-softmax + target gather (cs_logsoftmax_gather).
#include "cs_kernels.cuh"

namespace {

// Work items (row, split) are walked grid-stride so a capped grid also works.
template <int DT, bool CAP, bool FIXED, int BLOCK, int UNROLL>
__global__ __launch_bounds__(BLOCK, BLOCK >= 1024 ? 8 : 1) void lsg_stream_kernel(
    const char* __restrict__ logits, int64_t n_items, int64_t vocab, int64_t ld_bytes,
    int32_t nsplit, int64_t split_len, const int32_t* __restrict__ tgt, int32_t k, float cap,
    float inv_cap, float* __restrict__ out_tok, float* __restrict__ out_lse,
    float2* __restrict__ part) {
  __shared__ float sm_m[BLOCK / 64];
  __shared__ float sm_s[BLOCK / 64];
  __shared__ float sm_lse;
  constexpr bool TAB = CapTable<DT, CAP, FIXED>::kOn;
  __shared__ float ctab[TAB ? kCapTab : 1];
  const int tid = threadIdx.x;
  if constexpr (TAB) {
    build_cap_table<BLOCK>(ctab, cap, inv_cap);
    __syncthreads();
  }

  for (int64_t bid = blockIdx.x; bid < n_items; bid += gridDim.x) {
    const int64_t row = bid / nsplit;
    const int32_t split = static_cast<int32_t>(bid - row * nsplit);
    const char* rp = logits + row * ld_bytes;
    const int64_t v0 = static_cast<int64_t>(split) * split_len;
    const int64_t v1 = min(vocab, v0 + split_len);
    const float2 ms =
        block_lse_partial<DT, CAP, FIXED, BLOCK, UNROLL>(rp, v0, v1 - v0, cap, inv_cap, sm_m, sm_s,
                                                         ctab);
    if (tid == 0) {
      if (nsplit > 1) {
        part[bid] = ms;
      } else {
        const float lse = ms.x + logf(ms.y);
        sm_lse = lse;
        if (out_lse) out_lse[row] = lse;
      }
    }
    __syncthreads();
    if (nsplit == 1 && k > 0)
      gather_targets(rp, vocab, sm_lse, tgt + row * k, k, out_tok + row * k, CAP, cap, inv_cap,
                     DT, tid, BLOCK);
    __syncthreads();  // sm_* are reused by the next work item
  }
}

// Split rows in the canonical split arithmetic (split_partial, cs_kernels.cuh): BLOCK / 256
// splits per workgroup, each split's (m, s) to part[row * nsplit + split] for lsg_merge_kernel.
template <int DT, bool CAP, bool FIXED, int BLOCK>
__global__ __launch_bounds__(BLOCK, BLOCK >= 1024 ? 8 : 1) void lsg_split_kernel(
    const char* __restrict__ logits, int64_t n_items, int64_t vocab, int64_t ld_bytes,
    int32_t nsplit, int64_t split_len, float cap, float inv_cap, float2* __restrict__ part) {
  __shared__ float sm_m[BLOCK / 64];
  __shared__ float sm_s[BLOCK / 64];
  constexpr bool TAB = CapTable<DT, CAP, FIXED>::kOn;
  __shared__ float ctab[TAB ? kCapTab : 1];
  if constexpr (TAB) {
    build_cap_table<BLOCK>(ctab, cap, inv_cap);
    __syncthreads();
  }
  const int32_t per_row = split_items(nsplit, BLOCK);
  for (int64_t bid = blockIdx.x; bid < n_items; bid += gridDim.x) {
    const int64_t row = bid / per_row;
    const int32_t item = static_cast<int32_t>(bid - row * per_row);
    int32_t split;
    bool valid;
    const float2 ms = split_partial<DT, CAP, FIXED, BLOCK>(logits + row * ld_bytes, item, nsplit,
                                                          split_len, vocab, cap, inv_cap, sm_m,
                                                          sm_s, ctab, split, valid);
    if (valid && threadIdx.x % kSplitSub == 0) part[row * nsplit + split] = ms;
    __syncthreads();  // sm_* are reused by the next work item
  }
}

// split-V finish: merge the (m, s) partials of one row in split order, then gather.
template <int DT, bool CAP>
__global__ __launch_bounds__(kMergeBlock) void lsg_merge_kernel(
    const char* __restrict__ logits, int64_t vocab, int64_t ld_bytes, int32_t nsplit,
    const float2* __restrict__ part, const int32_t* __restrict__ tgt, int32_t k, float cap,
    float inv_cap, float* __restrict__ out_tok, float* __restrict__ out_lse) {
  const int64_t row = blockIdx.x;
  const int lane = threadIdx.x;
  float m = -INFINITY, s = 0.0f;
  for (int j = lane; j < nsplit; j += kMergeBlock) {
    const float2 p = part[row * nsplit + j];
    lse_merge(m, s, p.x, p.y);
  }
  wave_lse_reduce(m, s);
  const float lse = m + logf(s);
  if (lane == 0 && out_lse) out_lse[row] = lse;
  if (k > 0)
    gather_targets(logits + row * ld_bytes, vocab, lse, tgt + row * k, k, out_tok + row * k, CAP,
                   cap, inv_cap, DT, lane, kMergeBlock);
}

// Streaming-kernel shapes, from the A/B on the bench's data (profiles/r01_lsg_variants.jsonl):
//   single pass (rows >= 2048): 1024 threads x 2 vectors in flight  (C2: 7.25 TB/s, 90.6 %)
//   split-V (fewer rows):        the canonical split arithmetic (split_partial, cs_kernels.cuh):
//                                256-thread sub-blocks x 2 vectors, 4 splits per 1024 threads
template <int DT, bool CAP, bool FIXED>
void launch_lsg(const void* logits, int64_t rows, int64_t vocab, int64_t ld_bytes,
                const SplitPlan& plan, const int32_t* tgt, int32_t k, float cap, float* out_tok,
                float* out_lse, float2* part, hipStream_t st) {
  const float inv_cap = CAP ? 1.0f / cap : 0.0f;
  const char* lg = static_cast<const char*>(logits);
  if (plan.nsplit == 1) {
    hipLaunchKernelGGL((lsg_stream_kernel<DT, CAP, FIXED, 1024, 2>), dim3(static_cast<uint32_t>(rows)),
                       dim3(1024), 0, st, lg, rows, vocab, ld_bytes, plan.nsplit, plan.split_len, tgt,
                       k, cap, inv_cap, out_tok, out_lse, part);
    return;
  }
  // the canonical split arithmetic, four splits per 1024-thread workgroup
  const int64_t n_items = rows * split_items(plan.nsplit, 1024);
  hipLaunchKernelGGL((lsg_split_kernel<DT, CAP, FIXED, 1024>), dim3(static_cast<uint32_t>(n_items)),
                     dim3(1024), 0, st, lg, n_items, vocab, ld_bytes, plan.nsplit, plan.split_len, cap,
                     inv_cap, part);
  hipLaunchKernelGGL((lsg_merge_kernel<DT, CAP>), dim3(static_cast<uint32_t>(rows)), dim3(kMergeBlock),
                     0, st, lg, vocab, ld_bytes, plan.nsplit, part, tgt, k, cap, inv_cap, out_tok,
                     out_lse);
}

}  // namespace

extern "C" {

const char* cs_version(void) { return "consensus_scoring 0.1.0 (gfx950)"; }

const char* cs_last_error(void) { return cs_g_last_error.c_str(); }

size_t cs_workspace_size(int64_t rows, int64_t vocab, int32_t k) {
  (void)k;
  const SplitPlan p = plan_split(rows, vocab, CS_BF16);
  const SplitPlan q = plan_split(rows, vocab, CS_F32);
  const int32_t ns = p.nsplit > q.nsplit ? p.nsplit : q.nsplit;
  if (ns <= 1) return 0;
  return static_cast<size_t>(rows) * static_cast<size_t>(ns) * sizeof(float2);
}

int cs_logsoftmax_gather(const void* logits, int dtype, int64_t rows, int64_t vocab, int64_t ld,
                         const int32_t* target_ids, int32_t k, float softcap, float* out_tok_lp,
                         float* out_row_lse, void* workspace, size_t workspace_bytes,
                         cs_stream_t stream) {
  const char* fn = "cs_logsoftmax_gather";
  if (int rc = check_logits(fn, dtype, vocab, ld)) return rc;
  if (rows < 0 || k < 0) return fail(CS_ERR_INVALID, std::string(fn) + ": need rows >= 0 and k >= 0");
  if (rows > 0x7fffffffLL) return fail(CS_ERR_INVALID, std::string(fn) + ": rows exceeds 2^31-1");
  if (rows == 0) return CS_OK;
  if (!logits) return fail(CS_ERR_INVALID, std::string(fn) + ": logits is NULL");
  if (k > 0 && (!target_ids || !out_tok_lp))
    return fail(CS_ERR_INVALID, std::string(fn) + ": k > 0 needs target_ids and out_tok_lp");
  if (int rc = check_softcap(fn, softcap)) return rc;
  if (int rc = check_elt_aligned(fn, logits, dtype)) return rc;
  const SplitPlan plan = plan_split(rows, vocab, dtype);
  if (int rc = check_grid(fn, rows * plan.nsplit)) return rc;
  float2* part = nullptr;
  if (plan.nsplit > 1) {
    const size_t need = static_cast<size_t>(rows) * plan.nsplit * sizeof(float2);
    if (int rc = check_workspace(fn, workspace, workspace_bytes, need)) return rc;
    part = static_cast<float2*>(workspace);
  }
  const int64_t ld_bytes = ld * elt_size(dtype);
  dispatch_dtype_cap_fixed(dtype, softcap, [&](auto dt, auto cap, auto fixed) {
    launch_lsg<decltype(dt)::value, decltype(cap)::value, decltype(fixed)::value>(
        logits, rows, vocab, ld_bytes, plan, target_ids, k, softcap, out_tok_lp, out_row_lse, part,
        static_cast<hipStream_t>(stream));
  });
  return check_launch("cs_logsoftmax_gather");
}

}  // extern "C"
