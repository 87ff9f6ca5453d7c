/*
 * consensus_scoring.h — C-ABI of the MI355X (gfx950) agent x candidate scoring path.
 *
 * The reference (cartgr/Generating-Fair-Consensus-Statements-with-Social-Choice-on-Token-Level-MDPs)
 * has no native code and no FFI: every log-probability comes back from a remote
 * HTTPS call (`get_prompt_logprobs`, src/utils.py:201-281) and is folded into
 * per-agent utilities and welfare by serial Python loops.  This header is the
 * boundary that replaces those loops.  Each entry point names the reference code
 * it replaces (file:line, relative to the reference root).
 *
 * Conventions
 *   - All data pointers are caller-owned DEVICE buffers (e.g. torch tensors'
 *     data_ptr()).  The library never allocates on the hot path; the only scratch
 *     is the caller-provided workspace sized by cs_workspace_size().
 *   - Every call is asynchronous and stream-ordered on `stream` (a hipStream_t
 *     passed as an opaque pointer; NULL = the default stream).  No host sync.
 *   - Return value: CS_OK (0) on success, a negative cs_status otherwise; the
 *     message is available from cs_last_error() (thread-local).
 *   - Kernels are re-entrant: no global mutable device state.
 *   - Results are deterministic run-to-run: no float atomics, fixed reduction order.
 */
#ifndef CONSENSUS_SCORING_H
#define CONSENSUS_SCORING_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* cs_stream_t; /* hipStream_t */

/* element type of the logits buffer */
enum cs_dtype { CS_F32 = 0, CS_BF16 = 1, CS_F16 = 2 };

/* welfare over agents (applied per candidate column) */
enum cs_welfare {
  CS_WELFARE_MIN = 0,    /* egalitarian: min_a u[a,c]                                  */
  CS_WELFARE_SUM = 1,    /* utilitarian: sum_a u[a,c]                                  */
  CS_WELFARE_SUMLOG = 2, /* log-Nash:    sum_a log(max(u[a,c], eps))                   */
  CS_WELFARE_MAX = 3     /* max_a u[a,c] (egalitarian over a cost, e.g. perplexity)    */
};

/* what cs_welfare_reduce does with a non-finite utility */
enum cs_nonfinite {
  CS_NONFINITE_SKIP = 0,   /* drop it (src/evaluation.py:316-319, `np.isfinite` filter)        */
  CS_NONFINITE_REPLACE = 1 /* nan_to_num(nan, posinf, neginf) (src/methods/best_of_n.py:384-389) */
};

enum cs_status {
  CS_OK = 0,
  CS_ERR_INVALID = -1,   /* bad argument (shape, dtype, null pointer)          */
  CS_ERR_WORKSPACE = -2, /* workspace missing or smaller than cs_workspace_size */
  CS_ERR_HIP = -3        /* a HIP launch failed                                 */
};

/* Library identification and last error (thread-local, never NULL). */
const char* cs_version(void);
const char* cs_last_error(void);

/* Bytes of device workspace cs_logsoftmax_gather needs for this shape (0 when the
 * single-pass path is used).  Pure host function. */
size_t cs_workspace_size(int64_t rows, int64_t vocab, int32_t k);

/*
 * cs_logsoftmax_gather — fused vocab-wide log-softmax + candidate-token gather.
 *
 * For every row r of logits[rows][ld] (first `vocab` columns used):
 *     x'       = softcap > 0 ? softcap * tanh(x / softcap) : x
 *     lse[r]   = log(sum_v exp(x'[r,v]))
 *     out_tok_lp[r*k + j] = x'[r, target_ids[r*k + j]] - lse[r]      (j < k)
 * A target id outside [0, vocab) yields NaN (the reference's `None` log-prob,
 * src/utils.py:262-263, which every caller filters).
 * One HBM pass over the logits; fp32 accumulation.
 *
 * Non-finite rows.  A row with a NaN anywhere in its first `vocab` columns has NaN
 * lse and NaN out_tok_lp at every j, in every dtype, soft-cap mode and split plan
 * (as the fp64 oracle, oracle_logsoftmax_gather).  A row whose first `vocab` columns
 * are all -inf (softcap = 0) has lse = -inf and NaN out_tok_lp, like torch.logsumexp;
 * the fp64 oracle returns NaN for the lse of such a row as well.  The same holds for
 * the agent rows of cs_beam_step and cs_beam_decode_step, which share this stream.
 *
 * Replaces: the remote log-softmax + gather behind get_prompt_logprobs
 *   (src/utils.py:249-263, echo=True prompt log-probs), the per-token read in
 *   _get_agent_token_logprob (src/methods/beam_search.py:389-390; one row per
 *   (agent, beam) gathered at k candidate tokens), and core.log_softmax_rows +
 *   gather (core.py:64-68, 88-90).
 *
 * out_row_lse may be NULL.  workspace may be NULL iff cs_workspace_size() == 0.
 */
int cs_logsoftmax_gather(const void* logits, int dtype, int64_t rows, int64_t vocab, int64_t ld,
                         const int32_t* target_ids, int32_t k, float softcap, float* out_tok_lp,
                         float* out_row_lse, void* workspace, size_t workspace_bytes,
                         cs_stream_t stream);

/*
 * cs_segment_reduce — per-candidate folding of token log-probs.
 *
 * Segment s covers tok_lp[seg_offsets[s] .. seg_offsets[s+1]) (CSR, non-decreasing).
 * NaN entries (None log-probs) are skipped.  Sums are accumulated in fp64 in a
 * fixed order.  Outputs (any may be NULL):
 *     out_sum_lp[s] = sum lp        out_sum_p[s] = sum exp(lp)
 *     out_count[s]  = #non-NaN      out_last[s]  = tok_lp[seg_offsets[s+1]-1] (NaN if empty)
 *
 * Replaces: mean of valid log-probs (src/methods/best_of_n.py:303-305),
 *   np.mean(logprobs[-len(path):]) (src/methods/finite_lookahead.py:508-520),
 *   avg_logprob / avg_prob (src/evaluation.py:203-213), sum(full_logprobs[-1:])
 *   (src/methods/beam_search.py:389-390), logu[:, j] += ls[:, a_t] (core.py:90).
 */
int cs_segment_reduce(const float* tok_lp, int64_t n, const int32_t* seg_offsets, int64_t n_seg,
                      float* out_sum_lp, float* out_sum_p, int32_t* out_count, float* out_last,
                      cs_stream_t stream);

/*
 * cs_welfare_reduce — welfare across agents for every candidate.
 *
 * U is [A][C] with row stride ldu (agent-major, agent order = dict order of
 * agent_opinions).  W[c] = welfare_kind over a of U[a*ldu + c], folded in agent
 * order in fp64.  Non-finite utilities are skipped or replaced (cs_nonfinite);
 * a column with no usable utility gives NaN.
 *
 * Replaces: min over agents (src/methods/beam_search.py:558-560,
 *   src/methods/best_of_n.py:401-408, src/methods/finite_lookahead.py:527);
 *   utilitarian / log-Nash welfare (src/evaluation.py:337-349, 367-381);
 *   F_val at a point-mass lottery (core.py:108-113); utilitarian column sums
 *   (core.py:374).
 */
int cs_welfare_reduce(const float* U, int32_t A, int32_t C, int64_t ldu, int kind, float eps,
                      int nonfinite, float nan_val, float posinf_val, float neginf_val, float* W,
                      cs_stream_t stream);

/*
 * cs_segmented_topk — stable descending top-k inside each segment.
 *
 * Segment s is W[s*ld .. s*ld + seg_len).  out_idx[s*k + r] is the index (within
 * the segment) of the element of rank r, ranks ordered by (value desc, index asc);
 * NaN ranks below every number.  out_val may be NULL.  k <= seg_len <= 16384.
 *
 * Replaces: sorted(candidates, key=min(rewards), reverse=True) — stable, so ties
 *   keep insertion order (src/methods/beam_search.py:558-560, 646-648);
 *   np.argmax, first max wins (src/methods/best_of_n.py:198, core.py:374);
 *   max(range, key=...) (src/methods/finite_lookahead.py:527).
 */
int cs_segmented_topk(const float* W, int32_t n_seg, int32_t seg_len, int64_t ld, int32_t k,
                      int32_t* out_idx, float* out_val, cs_stream_t stream);

/*
 * cs_beam_step — one scoring step of token-level beam search after the LM head, in ONE
 * launch (one workgroup per (agent row, vocab split); the last workgroup of each row
 * finishes that row, the last row folds the welfare and sorts).
 *
 * logits holds the agent rows [A*B][ld] (row a*B + b = agent a's prompt + beam b);
 * targets [B][K] are the candidate tokens of beam b, shared by every agent (an id
 * outside [0, vocab) is padding and yields NaN); rewards_in [A][B] is each agent's
 * cumulative reward of each beam.  With C = B*K and c = b*K + j:
 *     lp           = x'[a*B+b, targets[c]] - lse[a*B+b]           (as cs_logsoftmax_gather)
 *     out_U[a*C+c] = rewards_in[a*B+b] + lp                      (fp32 add)
 *     out_W[c]     = welfare_kind over a of out_U[a*C+c]         (as cs_welfare_reduce, SKIP)
 *     out_order[r] = index of rank r by (W desc, index asc), NaN last, r < n_order
 *                    (as cs_segmented_topk); out_order_val (nullable) = W at that index.
 *     out_kept[a*n_order + r] (nullable) = out_U[a*C + out_order[r]]: the cumulative
 *                    rewards of the kept beams when the first n_order ranks are kept
 *                    (needs n_order > 0 and B*K <= 1024).
 * n_order <= 256 selects the n_order best (radix-select threshold + rank counting, the
 * exact stable order) without sorting the rest.
 * Bit-identical to cs_logsoftmax_gather + cs_welfare_reduce + cs_segmented_topk on the
 * same inputs.  n_order = 0 skips the sort (agent-sharded runs all-reduce out_W
 * first, then call cs_segmented_topk).  B*K <= 16384 (a second launch sorts when
 * B*K > 1024).
 *
 * WORKSPACE: cs_beam_step_workspace_size() bytes, zero-filled before the first call and
 * used by one stream at a time.  It holds arrival counters that every call leaves at
 * zero, so it is reused without a memset (and inside captured graphs).
 *
 * Replaces: the per-(beam, token, agent) scoring loop, cumulative rewards and the
 *   stable sort by min over agents of src/methods/beam_search.py:495-560
 *   (_get_agent_token_logprob :335-404 per candidate).
 */
size_t cs_beam_step_workspace_size(int64_t rows, int64_t vocab);
int cs_beam_step(const void* logits, int dtype, int32_t A, int32_t B, int64_t vocab, int64_t ld,
                 const int32_t* targets, int32_t K, const float* rewards_in, float softcap,
                 int welfare_kind, float eps, float* out_U, float* out_W, int32_t n_order,
                 int32_t* out_order, float* out_order_val, float* out_kept, void* workspace,
                 size_t workspace_bytes, cs_stream_t stream);

/*
 * cs_beam_decode_step — one whole beam-search decode step after the LM head in ONE
 * launch: cs_vocab_topk on the B reference-policy rows (ref_logits [B][ld_ref]) proposes
 * K candidate tokens per beam (out_ids [B][K], value desc / id asc), and cs_beam_step
 * scores them under the agent rows (logits [A*B][ld]) — out_U, out_W, out_order,
 * out_order_val, out_kept exactly as cs_beam_step with targets = out_ids.  The proposer
 * workgroups run beside the agent-row stream; per beam the last of its A + 1 arrivals
 * gathers the beam's candidates.  Bit-identical to cs_vocab_topk + cs_beam_step.
 * Limits: K <= min(256, vocab), B*K <= 16384, A*B <= 65536, B <= 4096.
 *
 * WORKSPACE: cs_beam_decode_workspace_size() bytes, zero-filled before the first call,
 * used by one stream at a time, left zeroed by every call (graph-replayable).
 *
 * Replaces: the reference's per-step loop of beam_search.py:439-560 — unique-token
 *   sampling per beam (:199-333), per (beam, token, agent) scoring (:335-404, 495-538),
 *   cumulative rewards and the stable sort by min over agents (:534-560).
 */
size_t cs_beam_decode_workspace_size(int32_t A, int32_t B, int64_t vocab, int32_t K);
int cs_beam_decode_step(const void* ref_logits, int64_t ld_ref, const void* logits, int64_t ld,
                        int dtype, int32_t A, int32_t B, int64_t vocab, int32_t K, float softcap,
                        const float* rewards_in, int welfare_kind, float eps, int32_t* out_ids,
                        float* out_U, float* out_W, int32_t n_order, int32_t* out_order,
                        float* out_order_val, float* out_kept, void* workspace,
                        size_t workspace_bytes, cs_stream_t stream);

/*
 * cs_beam_select — the selection half of an agent-sharded beam step, after the welfare
 * all-reduce: out_order[r] = index of rank r of W by (W desc, index asc), NaN last,
 * r < n_order (as cs_segmented_topk); out_order_val (nullable) = W there; out_kept
 * (nullable) [A][n_order] = U[a*C + out_order[r]] for this rank's A agents (U [A][C],
 * the out_U of its cs_beam_decode_step / cs_beam_step); out_W (nullable) = W after
 * unfill.  unfill: CS_UNFILL_POSINF turns +inf back into NaN (the MIN combine fills
 * columns without a usable utility with +inf before the all-reduce, parallel.py),
 * CS_UNFILL_NEGINF does the same for -inf (MAX), CS_UNFILL_NONE leaves W as is.
 * One workgroup, one launch; C <= 1024, 0 < n_order <= C.  Bit-identical to
 * cs_segmented_topk + the column gather.
 *
 * Replaces: the stable sort by min over agents and the keep of the first beam_width of
 *   src/methods/beam_search.py:558-593 on a rank that holds a subset of the agents.
 */
#define CS_UNFILL_NONE 0
#define CS_UNFILL_POSINF 1
#define CS_UNFILL_NEGINF 2
int cs_beam_select(const float* W, int32_t C, int unfill, const float* U, int32_t A,
                   int32_t n_order, float* out_W, int32_t* out_order, float* out_order_val,
                   float* out_kept, cs_stream_t stream);

/*
 * cs_vocab_topk — deterministic candidate proposer: the k largest (soft-capped)
 * logits of every row, ordered by (value desc, token id asc).
 *
 * Replaces the serial unique-token sampling loop of the reference's beam search
 * (_sample_next_tokens, src/methods/beam_search.py:199-333: up to
 * max_sampling_attempts remote completions per beam) with one HBM pass per step;
 * k is the build's deterministic "top-k tokens per beam" (BASELINE configs).
 * Logit-bias masking (beam_search.py:236-251) is applied by the caller to the
 * logits rows before the call.  k <= 256 and ceil(vocab/4096)*k <= 16384.
 * out_vals may be NULL.
 */
size_t cs_vocab_topk_workspace_size(int64_t rows, int64_t vocab, int32_t k);
int cs_vocab_topk(const void* logits, int dtype, int64_t rows, int64_t vocab, int64_t ld, int32_t k,
                  float softcap, int32_t* out_ids, float* out_vals, void* workspace,
                  size_t workspace_bytes, cs_stream_t stream);

/*
 * cs_vocab_sample — seeded Gumbel-max sampling, n_draw independent draws per row.
 *
 * Draw d of row r returns argmax_v ( x'[r,v] / temperature + g(seeds[r*n_draw+d], v) ),
 * ties to the lowest id, with g = -log(-log(u)) and u the counter-based uniform
 * documented in oracle/oracle.py (splitmix64 of (seed, v), top 23 bits + 0.5, scaled by 2^-23).
 * out_lp (nullable) receives the drawn token's log-probability under
 * softmax(x'/temperature).  n_draw <= 16.
 * A token whose x' is -inf or NaN is never drawn; any NaN logit in the row makes the
 * row's log-probabilities NaN.  A row with no finite logit yields id -1 and NaN, which
 * callers must filter, like the NaN of an out-of-range target.  (What is judged is x':
 * a soft-cap maps a -inf logit to -softcap, an ordinary token.)
 *
 * Replaces the remote one-token samplers: client.completions.create(max_tokens=1,
 * seed=base_seed+attempt, logit_bias) (src/methods/beam_search.py:253-297),
 * generate_text(max_tokens=1, temperature=1, seed) in the lookahead tree
 * (src/methods/finite_lookahead.py:310-334) and the per-token draws of the
 * Best-of-N candidate generation (src/methods/best_of_n.py:104-118).
 */
size_t cs_vocab_sample_workspace_size(int64_t rows, int64_t vocab, int32_t n_draw);
int cs_vocab_sample(const void* logits, int dtype, int64_t rows, int64_t vocab, int64_t ld,
                    float temperature, float softcap, const uint64_t* seeds, int32_t n_draw,
                    int32_t* out_ids, float* out_lp, void* workspace, size_t workspace_bytes,
                    cs_stream_t stream);

/*
 * cs_sample_step — one generation step of S independent streams after the LM head: the
 * seeded draw, the stop test, the append and the next step's input token.  Everything that
 * changes between steps is read from device memory, so a captured graph replays the call
 * with no new argument and no memset between replays.
 *
 * With t = *step (device, int32), for stream s:
 *   done[s] != 0: next_tok[s] = pad_id, nothing else of the stream is written and its logits
 *     row is not read.
 *   otherwise: id, lp = the one draw of cs_vocab_sample with seed
 *     (base_seeds[s] * 1000003 + t) mod 2^64 (runtime.draw_seed) on the row
 *     x[v] = float(logits[s][v]) + (v listed in bias_ids ? bias_value : 0), the bias added in
 *     fp32 before the soft-cap, once per token however often it is listed, ids outside
 *     [0, vocab) ignored.  Bit for bit cs_vocab_sample(rows = S, n_draw = 1) on that fp32 row.
 *     id == -1 (no drawable logit) or id in stop_ids: done[s] = 1, nothing appended.
 *     else: out_tokens[s][out_len[s]] = id, out_lp[s][out_len[s]] = lp (out_lp nullable),
 *       out_len[s] += 1, and done[s] = 1 once out_len[s] == max_tokens.  (A stream handed
 *       over with out_len outside [0, max_tokens) is ended without an append.)
 *     next_tok[s] (int64, the layout of DecodeState.tok) = id while the stream is unfinished
 *       after the step, else pad_id.
 *   n_alive[0] = number of streams with done == 0 after the call.
 * Limits: n_bias <= 1024, n_stop <= 16, max_tokens >= 1, 0 <= pad_id < vocab, and with
 * n_bias > 0 at most 2^19 tokens per row slice (vocab / the split count of the plan).
 * S = 0 is CS_OK and writes nothing.
 *
 * WORKSPACE: cs_sample_step_workspace_size() bytes, zero-filled before the first call, used
 * by one stream at a time, left zeroed where it counts (one arrival word) by every call.
 *
 * Replaces: the remote completion loop behind generate_text (src/utils.py:69-118) for many
 *   prompts at once, as the Best-of-N candidates (src/methods/best_of_n.py:104-118) and the
 *   Habermas Machine's per-agent prompts need it.
 */
size_t cs_sample_step_workspace_size(int64_t S, int64_t vocab);
int cs_sample_step(const void* logits, int dtype, int64_t S, int64_t vocab, int64_t ld,
                   float temperature, float softcap, const uint64_t* base_seeds,
                   const int32_t* step, const int32_t* bias_ids, int32_t n_bias, float bias_value,
                   const int32_t* stop_ids, int32_t n_stop, int32_t max_tokens, int32_t pad_id,
                   int32_t* done, int32_t* out_len, int32_t* out_tokens, float* out_lp,
                   int64_t* next_tok, int32_t* n_alive, void* workspace, size_t workspace_bytes,
                   cs_stream_t stream);

/*
 * cs_vocab_sample_ex — cs_vocab_sample with a logit bias, a repetition penalty and greedy
 * decoding, all inside the one pass over the row.
 *
 * The row that is drawn from, in fp32, for token v of row r:
 *   x = float(logits[r][v]) + (v listed in bias_ids ? bias_value : 0), then the soft-cap
 *     (cs_sample_step's biased row: once per token however often listed, ids outside
 *     [0, vocab) ignored);
 *   if repetition_penalty != 1 and v is in seen_ids[seen_off[r] : seen_off[r+1]] (int32,
 *     device, seen_off [rows + 1]; both NULL: no list): x = x < 0 ? x * penalty : x / penalty,
 *     a correctly rounded fp32 division: transformers' RepetitionPenaltyLogitsProcessor on the
 *     model's final logits, before the temperature.  Ids outside [0, vocab) are ignored,
 *     duplicates count once, -inf stays -inf and NaN stays NaN.
 * temperature > 0: cs_vocab_sample's Gumbel-max draws on x / temperature.
 * temperature == 0: greedy.  Every draw is the argmax of x, ties to the lowest id; seeds is
 *   not read (may be NULL); out_lp is the token's log-probability under softmax(x).
 * The never-drawn and poisoned-row rules of cs_vocab_sample hold on x.
 * With temperature > 0, no bias and no penalty (penalty 1 or no list) the call IS
 * cs_vocab_sample: same kernels, same bits.
 * Limits: those of cs_vocab_sample, n_bias <= 1024, penalty finite and > 0, and at most 2^19
 * tokens per row slice (two LDS bitmaps over the slice).
 */
size_t cs_vocab_sample_ex_workspace_size(int64_t rows, int64_t vocab, int32_t n_draw);
int cs_vocab_sample_ex(const void* logits, int dtype, int64_t rows, int64_t vocab, int64_t ld,
                       float temperature, float softcap, const uint64_t* seeds, int32_t n_draw,
                       const int32_t* bias_ids, int32_t n_bias, float bias_value,
                       float repetition_penalty, const int32_t* seen_ids, const int32_t* seen_off,
                       int32_t* out_ids, float* out_lp, void* workspace, size_t workspace_bytes,
                       cs_stream_t stream);

/*
 * cs_sample_step_ex — cs_sample_step with greedy decoding, a repetition penalty and stop
 * strings; still two launches, and still replayable from a captured graph with no new
 * argument.
 *
 * For an unfinished stream s, id and lp are bit for bit cs_vocab_sample_ex(rows = S,
 * n_draw = 1) with the seed of cs_sample_step, on the same bias and with the seen set
 *   seen_ids[seen_off[s] : seen_off[s+1]] (the stream's prompt tokens; seen_off [S + 1])
 *   plus out_tokens[s][0 : out_len[s]] as they stand when the call starts,
 * so the set grows from step to step by itself.  temperature == 0 is greedy: base_seeds and
 * the step's value are not used for the draw.
 * The state update is cs_sample_step's, and then, if the token was appended and
 * n_stop_seq > 0: with the window tail[s][0 : tail_len[s]] ++ bytes(id), where bytes(v) =
 * tok_bytes[tok_off[v] : tok_off[v+1]] (uint8 / int32 [vocab + 1], device), done[s] = 1 if
 * one of the stop strings occurs in the window ending inside the new token's bytes (the token
 * stays appended, so a host that cuts the text sees the whole occurrence; next_tok[s] =
 * pad_id).  The new tail is the last min(31, length) bytes of the window.  A token with no
 * bytes (a special token) changes nothing.  tail is uint8 [S][32], tail_len int32 [S], both
 * device memory, zero before a stream's first step.
 * The stop strings are HOST memory, copied into the launch: string k is
 * stop_bytes[stop_off[k] : stop_off[k+1]], stop_off[0] = 0, n_stop_seq <= 8 strings of 1 to
 * 32 bytes.  With n_stop_seq == 0 none of tok_bytes, tok_off, stop_bytes, stop_off, tail and
 * tail_len is read.
 * With temperature > 0, penalty 1 and n_stop_seq == 0 the call IS cs_sample_step: same
 * kernels, same bits.
 * Limits and workspace: those of cs_sample_step (the same size), penalty finite and > 0, and
 * at most 2^19 tokens per row slice whether or not a bias is given.
 *
 * Replaces: temperature=0, repetition_penalty and stop of the remote completion call behind
 *   generate_text (src/utils.py:77-198), as the Habermas Machine's ranking prediction
 *   (src/methods/habermas_machine.py:948) and the evaluator's judges use them.
 */
size_t cs_sample_step_ex_workspace_size(int64_t S, int64_t vocab);
int cs_sample_step_ex(const void* logits, int dtype, int64_t S, int64_t vocab, int64_t ld,
                      float temperature, float softcap, const uint64_t* base_seeds,
                      const int32_t* step, const int32_t* bias_ids, int32_t n_bias, float bias_value,
                      float repetition_penalty, const int32_t* seen_ids, const int32_t* seen_off,
                      const int32_t* stop_ids, int32_t n_stop, const uint8_t* tok_bytes,
                      const int32_t* tok_off, const uint8_t* stop_bytes, const int32_t* stop_off,
                      int32_t n_stop_seq, uint8_t* tail, int32_t* tail_len, int32_t max_tokens,
                      int32_t pad_id, int32_t* done, int32_t* out_len, int32_t* out_tokens,
                      float* out_lp, int64_t* next_tok, int32_t* n_alive, void* workspace,
                      size_t workspace_bytes, cs_stream_t stream);

/*
 * cs_dfa_token_masks — which tokens a byte-level automaton lets a stream draw, per state.
 *
 * trans is int16 [n_states][256] (the next state on a byte, -1: dead), accept uint8 [n_states],
 * token v's bytes are tok_bytes[tok_off[v] : tok_off[v+1]] (the table of cs_sample_step_ex),
 * all device memory.  masks is uint32 [n_states][ceil(vocab / 32)]; bit v & 31 of word
 * masks[q][v >> 5] is set iff
 *   v is listed in stop_ids (n_stop <= 16): accept[q] != 0 (the text may end here);
 *   otherwise: token v has at least one byte and walking its bytes from q never reaches -1
 *     (nor a value >= n_states, which counts as dead).
 * Bits past vocab are 0.  One launch, every word written; n_states * vocab / 8 bytes.
 * 1 <= n_states <= 1024, 0 < vocab < 2^31.
 */
int cs_dfa_token_masks(const int16_t* trans, const uint8_t* accept, int32_t n_states,
                       const uint8_t* tok_bytes, const int32_t* tok_off, int64_t vocab,
                       const int32_t* stop_ids, int32_t n_stop, uint32_t* masks,
                       cs_stream_t stream);

/*
 * cs_vocab_sample_dfa — cs_vocab_sample_ex on rows constrained by an automaton.
 *
 * Row r is in state dfa_state[r] (int32, device).  After bias, soft-cap and penalty, a token
 * whose bit is clear in masks[dfa_state[r] * mask_words + ...] (the layout of
 * cs_dfa_token_masks with row stride mask_words >= ceil(vocab / 32)) has x = -inf: it is out
 * of the log-sum-exp, so out_lp is the log-probability under the constrained distribution, and
 * by the never-drawn rule it is never drawn; a NaN logit under a clear bit does not poison the
 * row.  A state outside [0, n_states) allows nothing: id -1, NaN.  The bits are read from
 * global memory (the two LDS bitmaps of cs_vocab_sample_ex stay as they are, so the limits do).
 * masks == NULL: the call IS cs_vocab_sample_ex (same kernels, same bits; mask_words,
 * n_states and dfa_state are not looked at).  Otherwise 1 <= n_states <= 1024.
 */
size_t cs_vocab_sample_dfa_workspace_size(int64_t rows, int64_t vocab, int32_t n_draw);
int cs_vocab_sample_dfa(const void* logits, int dtype, int64_t rows, int64_t vocab, int64_t ld,
                        float temperature, float softcap, const uint64_t* seeds, int32_t n_draw,
                        const int32_t* bias_ids, int32_t n_bias, float bias_value,
                        float repetition_penalty, const int32_t* seen_ids, const int32_t* seen_off,
                        const uint32_t* masks, int64_t mask_words, int32_t n_states,
                        const int32_t* dfa_state, int32_t* out_ids, float* out_lp, void* workspace,
                        size_t workspace_bytes, cs_stream_t stream);

/*
 * cs_sample_step_dfa — cs_sample_step_ex with every stream held to an automaton; still two
 * launches, and still replayable from a captured graph with no new argument.
 *
 * For an unfinished stream s the draw is cs_vocab_sample_dfa's in state dfa_state[s], and the
 * state update is cs_sample_step_ex's.  Then, if the token was appended, its bytes
 * (tok_bytes / tok_off, needed here whether or not stop strings are given) are walked from
 * dfa_state[s] through trans (int16 [n_states][256]) and dfa_state[s] becomes the state
 * reached (-1 if the walk dies, which a set mask bit rules out); a token with no bytes leaves
 * it.  A state with no drawable token gives id -1, which ends the stream like any row without
 * a drawable logit; a stop id is drawable in accepting states only (cs_dfa_token_masks) and
 * ends the stream as before.
 * masks == NULL: the call IS cs_sample_step_ex (same kernels, same bits).
 * Limits and workspace: those of cs_sample_step_ex, 1 <= n_states <= 1024.
 *
 * Replaces: response_format={"type": "json_object"} of the evaluator's judges
 *   (src/evaluation.py:413-893) and the answer format the Habermas Machine parses
 *   (src/methods/habermas_machine.py), which the hosted endpoint enforces or the caller
 *   re-parses.
 */
size_t cs_sample_step_dfa_workspace_size(int64_t S, int64_t vocab);
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
                       cs_stream_t stream);

/*
 * cs_prefix_attention — cascade attention of many candidate streams over SHARED
 * per-agent prefix K/V (bf16 in / bf16 out, fp32 online softmax, bf16 MFMA).
 *
 * n_groups groups of n_str streams each; group i uses prefix group_prefix[i] (NULL =
 * identity).  Stream s = i*n_str + b carries T query tokens; token t of stream s is
 * q[(s*T + t)][H][D] and sees
 *     prefix keys  [0, prefix_len[pfx])   k_prefix  [Hkv][ld_prefix][D]
 *                                         vt_prefix [Hkv][ld_prefix/32][D][32]
 *                                         prefix p's key j is row prefix_off[p] + j (ragged
 *                                         prefixes in one buffer; prefix_off[p] % 32 == 0,
 *                                         rows up to the next multiple of 32 readable)
 *     its history  [0, *hist_base + t]    k_hist  [S][Hkv][ld_hist][D]
 *                                         vt_hist [S][Hkv][ld_hist/32][D][32]
 * V is stored transposed in 32-key tiles: keys 32c .. 32c+31 are the tile
 * vt[..][c][0..D)[0..32), key-contiguous rows of 64 B.  ld_prefix, ld_hist multiples of 32;
 * key slots past the visible range must hold finite values.  out [(s*T + t)][H][D].
 * Query head h uses K/V head h / (H / Hkv).  scores = q.k * scale, then
 * softcap * tanh(./softcap) when softcap > 0 (Gemma-2 attention soft-cap), softmax over the
 * visible keys; window > 0 also hides keys more than window - 1 positions behind the query
 * (Gemma-2's sliding window; prefix key j sits at position j, history slot j at
 * prefix_len + j).  D in {64, 128, 256}.  hist_base lives in device memory so that a
 * captured decode step replays with a growing history.  max_prefix_len (host) bounds
 * prefix_len.  One workgroup holds all query rows of (group, K/V head) (64 per workgroup),
 * so a prefix key block is read once for every candidate of that agent.
 *
 * Work plan: when few (group, head, query group) cells would leave the chip idle (decode
 * steps), each cell's keys are split over several workgroups and the splits merged in a
 * second launch.  cs_prefix_attention_plan (host) sizes the splits per cell from host
 * bounds of the prefix lengths (prefix_len[p] >= the device length; the split count is a
 * performance choice only) and the history capacity, and writes int32 x 4 entries:
 *     plan == NULL:  returns the entry count (0 = no plan needed: pass plan = NULL, no
 *                    workspace), n_attn / n_merge / workspace_bytes through the pointers;
 *     plan != NULL:  fills up to plan_cap entries.
 * The caller copies the entries to device memory once per prefix set and passes them with
 * n_attn, n_merge and a workspace of workspace_bytes.  Results are deterministic (fixed-order
 * split merge), and equal for every plan up to fp32 reassociation.
 *
 * Replaces: the per-(agent, candidate) re-encoding of the agent's whole prompt behind
 *   every get_prompt_logprobs call (src/utils.py:249-259; driven per candidate at
 *   src/methods/beam_search.py:495-538, best_of_n.py:266-321,
 *   finite_lookahead.py:464-524, src/evaluation.py:177-230).
 */
int64_t cs_prefix_attention_plan(const int32_t* prefix_len, int32_t n_prefix,
                                 const int32_t* group_prefix, int32_t n_groups, int32_t n_str,
                                 int32_t T, int32_t H, int32_t Hkv, int32_t D, int64_t ld_hist,
                                 int32_t* plan, int64_t plan_cap, int32_t* n_attn, int32_t* n_merge,
                                 size_t* workspace_bytes);
int cs_prefix_attention(const void* q, const void* k_prefix, const void* vt_prefix,
                        int64_t ld_prefix, const int64_t* prefix_off, const int32_t* prefix_len,
                        int32_t max_prefix_len, const int32_t* group_prefix, int32_t n_groups,
                        const void* k_hist, const void* vt_hist, int64_t ld_hist,
                        const int32_t* hist_base, int32_t n_str, int32_t T, int32_t H, int32_t Hkv,
                        int32_t D, float scale, float softcap, int32_t window, const void* plan,
                        int32_t n_attn, int32_t n_merge, void* out, void* workspace,
                        size_t workspace_bytes, cs_stream_t stream);

/*
 * cs_prefix_attention_rows — cs_prefix_attention over a ROW-LAYOUT history reached through a
 * slot table, for beam decoding without history copies:
 *     k_hist, v_hist  [S][Hkv][ld_hist][D] (V row-major like K, not in 32-key V^T tiles)
 *     hist_rows       [S][ld_hist] int32: slot j of stream s is row hist_rows[s][j] of k_hist /
 *                     v_hist (every entry a row of the buffers, which may hold more than the
 *                     S query streams: a token tree's earlier levels)
 * so a beam's inherited slots stay where its ancestor wrote them (cs_hist_rows_update builds
 * the next step's table; cs_rope_place_rows writes the step's K / V into the stream's own row).
 * Same arguments, plan and results otherwise (plan may be NULL with no workspace: one
 * workgroup per (group, K/V head, query group)).  Every result equals cs_prefix_attention on
 * the copied history the table describes, up to fp32 reassociation (the same block order:
 * bitwise in practice).
 *
 * Replaces: as cs_prefix_attention; the beam's history is the reference's beam text
 *   (src/methods/beam_search.py:491-538), re-encoded in full by every call there.
 */
int cs_prefix_attention_rows(const void* q, const void* k_prefix, const void* vt_prefix,
                             int64_t ld_prefix, const int64_t* prefix_off, const int32_t* prefix_len,
                             int32_t max_prefix_len, const int32_t* group_prefix, int32_t n_groups,
                             const void* k_hist, const void* v_hist, const int32_t* hist_rows,
                             int64_t ld_hist, const int32_t* hist_base, int32_t n_str, int32_t T,
                             int32_t H, int32_t Hkv, int32_t D, float scale, float softcap,
                             int32_t window, const void* plan, int32_t n_attn, int32_t n_merge,
                             void* out, void* workspace, size_t workspace_bytes, cs_stream_t stream);

/*
 * cs_rope_place — rotary embedding (half-rotation convention, angle = position *
 * inv_freq[i]) of the fused projection qkv [(s*T + t)][ld_qkv] = [q (H*D) | k (Hkv*D) |
 * v (Hkv*D)] and placement into the cs_prefix_attention layouts: q_out [(s*T+t)][H][D],
 * k_hist[s][g][j][:] (rotated), vt_hist[s][g][j/32][:][j%32], j = *hist_base + t.  The
 * position of token t of stream s (group i) is prefix_len[group_prefix[i]] + *hist_base + t.
 * bf16 in / out, fp32 rotation.
 * Refused (CS_ERR_INVALID, nothing launched): ld_hist not a multiple of 32 (the V^T tiles of a
 * head are whole; the _rows entry points take any ld_hist >= T); q_out, k_hist or vt_hist not
 * 16-byte aligned; qkv not 8-byte aligned or ld_qkv not a multiple of 4 (head_dim is a
 * multiple of 8, <= 256).  *hist_base + T <= ld_hist is the caller's to keep: the host does
 * not read hist_base.
 *
 * Replaces: the per-call re-encoding of the reference's prompts (src/utils.py:249-259):
 *   a candidate token's K/V is computed once and kept for every later step of its stream.
 */
int cs_rope_place(const void* qkv, int64_t ld_qkv, const float* inv_freq, const int32_t* prefix_len,
                  const int32_t* group_prefix, int32_t n_groups, const int32_t* hist_base,
                  int32_t n_str, int32_t T, int32_t H, int32_t Hkv, int32_t D, void* q_out,
                  void* k_hist, void* vt_hist, int64_t ld_hist, cs_stream_t stream);

/*
 * cs_rope_place_splitk — cs_rope_place on a K-split projection's unfolded fp32 partials
 * part [splits][n_tok][(H + 2 Hkv) D] (cs_gemm_bf16 with y = NULL): each element is summed in
 * split order and rounded to bf16 exactly as cs_gemm_bf16's own fold would, then rotated and
 * placed -- bitwise cs_gemm_bf16 (folded) followed by cs_rope_place, one launch fewer.
 * T < 32, head_dim % 16 == 0, part 16-byte aligned.
 *
 * Replaces: as cs_rope_place (src/utils.py:249-259).
 */
int cs_rope_place_splitk(const float* part, int32_t splits, const float* inv_freq,
                         const int32_t* prefix_len, const int32_t* group_prefix, int32_t n_groups,
                         const int32_t* hist_base, int32_t n_str, int32_t T, int32_t H,
                         int32_t Hkv, int32_t D, void* q_out, void* k_hist, void* vt_hist,
                         int64_t ld_hist, cs_stream_t stream);

/*
 * cs_rope_place_rows / cs_rope_place_splitk_rows — cs_rope_place / cs_rope_place_splitk with
 * V placed row-major like K: v_hist[s][g][j][:] (the cs_prefix_attention_rows layout), in the
 * stream's own row s.
 *
 * Replaces: as cs_rope_place (src/utils.py:249-259).
 */
int cs_rope_place_rows(const void* qkv, int64_t ld_qkv, const float* inv_freq,
                       const int32_t* prefix_len, const int32_t* group_prefix, int32_t n_groups,
                       const int32_t* hist_base, int32_t n_str, int32_t T, int32_t H, int32_t Hkv,
                       int32_t D, void* q_out, void* k_hist, void* v_hist, int64_t ld_hist,
                       cs_stream_t stream);
int cs_rope_place_splitk_rows(const float* part, int32_t splits, const float* inv_freq,
                              const int32_t* prefix_len, const int32_t* group_prefix,
                              int32_t n_groups, const int32_t* hist_base, int32_t n_str, int32_t T,
                              int32_t H, int32_t Hkv, int32_t D, void* q_out, void* k_hist,
                              void* v_hist, int64_t ld_hist, cs_stream_t stream);

/*
 * cs_hist_rows_update — the beam (or token-tree) step of a row-layout history
 * (cs_prefix_attention_rows):
 *     dst_rows[s][j] = src_rows[parent[s]][j]   j < *hist_base   (inherited slots, by table)
 *     dst_rows[s][j] = row_base + s             j >= *hist_base  (written by this and later steps)
 * dst [S][ld_hist] int32; src [any][ld_hist] (the parents' table: the previous beam step's,
 * or a token tree's parent level's), distinct from dst.  Beams: one buffer of S rows,
 * row_base 0, a ping-pong pair of tables so a queued step can be undone; a token tree: one
 * buffer for every level's streams, a level's streams at rows row_base .. row_base + S - 1.
 * n_rows: the K / V buffer's row count; row_base + S > n_rows is rejected (CS_ERR_INVALID),
 * so a table can never name a row past the buffer it indexes.  No K / V moves.  hist_base
 * in device memory (graph replays).
 *
 * Replaces: the reference's beams and lookahead paths are strings that every scoring call
 *   re-encodes in full (src/methods/beam_search.py:491-538, src/methods/finite_lookahead.py:
 *   297-399 through src/utils.py:249-259); here a kept beam or a tree node inherits its
 *   parent's K / V by table, without any copy.
 */
int cs_hist_rows_update(const int32_t* src_rows, int32_t* dst_rows, const int64_t* parent,
                        const int32_t* hist_base, int64_t S, int32_t ld_hist, int64_t row_base,
                        int64_t n_rows, cs_stream_t stream);

/*
 * cs_add_rms_norm — residual add + RMSNorm of bf16 rows in one pass:
 *     b' = b, or with b_weight: b' = b * rsqrt(mean(b^2) + eps) * g_b (rounded to bf16; the
 *          branch's own norm, Gemma-2's post-attention / post-MLP norm, bitwise as a
 *          separate cs_add_rms_norm over b alone)
 *     s = a + b' (rounded to bf16; b NULL = none), written to s_out when non-NULL (may alias a)
 *     y = s * rsqrt(mean(s^2) + eps) * g,  g = weight (plus_one = 0, Llama-3) or
 *         1 + weight (plus_one = 1, Gemma-2; also g_b); fp32 statistics, one rounding.
 * d a multiple of 8 (<= 32768), leading dimensions multiples of 8.
 *
 * Replaces: part of the remote forward behind every get_prompt_logprobs call
 *   (src/utils.py:249-259) — the per-layer residual + normalisation of each new token.
 */
int cs_add_rms_norm(const void* a, int64_t lda, const void* b, int64_t ldb, const void* b_weight,
                    void* s_out, int64_t lds, const void* weight, int64_t rows, int64_t d,
                    float eps, int plus_one, void* y, int64_t ldy, cs_stream_t stream);

/*
 * cs_add_rms_norm_splitk — cs_add_rms_norm whose branch b is the K-split partials of a
 * cs_gemm_bf16 called with y = NULL: partials [splits][rows][d] fp32 (contiguous, 16-byte
 * aligned, 1 <= splits <= 16, d <= 8192) are folded in split order and rounded to bf16 exactly as cs_gemm_bf16's own fold,
 * so the result is bitwise cs_gemm_bf16(y) followed by cs_add_rms_norm(b = y) — one launch
 * and one bf16 round trip fewer (a decode step's down projection + the residual add).
 */
int cs_add_rms_norm_splitk(const void* a, int64_t lda, const float* partials, int32_t splits,
                           const void* b_weight, void* s_out, int64_t lds, const void* weight,
                           int64_t rows, int64_t d, float eps, int plus_one, void* y, int64_t ldy,
                           cs_stream_t stream);

/*
 * cs_gated_act — the gated MLP activation of bf16 rows: out = act(gate) * up with act =
 * SiLU (act = 0, Llama-3) or tanh-GeLU (act = 1, Gemma-2), the activation rounded to bf16
 * before the product.  F and leading dimensions multiples of 8.
 *
 * Replaces: part of the remote forward behind every get_prompt_logprobs call
 *   (src/utils.py:249-259).
 */
int cs_gated_act(const void* gate, int64_t ld_gate, const void* up, int64_t ld_up, int64_t rows,
                 int64_t F, int act, void* out, int64_t ld_out, cs_stream_t stream);

/*
 * cs_gemm_bf16 — a decode step's projection GEMM, Y[M, N] = X[M, K] * W[N, K]^T, bf16 in
 * and out, fp32 accumulation (v_mfma_f32_16x16x32_bf16), for the few hundred rows one step
 * of all (agent, beam) streams has.  W (the streamed operand, read once) is [N, K] row-major
 * (a torch Linear weight); X [M, K]; Y [M, N] (gated = 0).  gated = 1: W is the fused
 * gate|up weight [2F, K] (gate rows first) and Y [M, F] = act(gate) * up with the rounding
 * of cs_gated_act (act 0 SiLU, 1 tanh-GeLU).  splits > 1 divides K over workgroups and
 * folds the fp32 partials in split order (workspace: splits * M * N floats); splits <= 0
 * takes cs_gemm_splits; y = NULL with splits > 1 leaves the partials [splits][M][N] in the
 * workspace unfolded (cs_add_rms_norm_splitk folds them).  variant: 0 = the library's choice, 1 = 2 x 4 wave grid (128 columns x
 * up to 288 rows per workgroup), 2 = column-only wave split, 256 columns, LDS-DMA X,
 * 3 = as 2 with 128 columns (gated: 4 waves, 64 features per workgroup, two workgroups per
 * CU; N a multiple of 128), 4 = as 2 with at most 144 rows per workgroup (row blocks of a
 * column tile paired on one XCD); 5-7 = the thin form for M <= 80 (no K split: every wave
 * of a workgroup streams its own K slice into registers, no barrier until the final fold;
 * 5: 16 features x 8 waves, 6: 32 x 8, 7: 16 x 16).  The variants' tile shapes, with what the
 * gated forms change, are the table kGemmVariants and gemm_form beside it in csrc/gemm.hip;
 * N % 256 != 0 sends variants 2 and 4 to 3 (gated: to 1).  N a multiple of 128, K of 64 * splits;
 * ldx, ldw multiples of 8, ldy of 4; X, W 16-byte aligned.  Deterministic (no atomics).
 *
 * Replaces: part of the remote forward behind every get_prompt_logprobs call
 *   (src/utils.py:249-259) — the per-layer q|k|v, output, gate|up and down projections of
 *   each new token (the gated form also replaces cs_gated_act on that path).
 */
int cs_gemm_bf16(const void* x, int64_t ldx, const void* w, int64_t ldw, void* y, int64_t ldy,
                 int64_t M, int64_t N, int64_t K, int splits, int gated, int act, int variant,
                 float* workspace, cs_stream_t stream);

/* cs_gemm_splits — the K split cs_gemm_bf16 takes for splits <= 0 (>= 1; 0 on a bad shape:
 * M, N or K <= 0, or N % 128 != 0).  1 for every other call that cs_gemm_bf16 rejects: a
 * variant outside 0..7, K % 64 != 0, a thin variant with M > 80. */
int64_t cs_gemm_splits(int64_t M, int64_t N, int64_t K, int gated, int variant);

/*
 * cs_gemm_pack — W [N, K] (row stride ldw) into the fragment-major layout of
 * cs_gemm_bf16_packed: 16-row tile T, 64-deep K step s, half h (k 32h .. 32h + 31) is 1 KB at
 * element ((T * K / 64 + s) * 2 + h) * 512, lane-linear (lane l's 8 elements = row 16T + l % 16,
 * k 64s + 32h + 8 (l / 16) .. + 7).  A pure permutation (N * K elements out); N % 16 == 0,
 * K % 64 == 0, 16-byte aligned.  Done once per weight, at model load.
 *
 * cs_gemm_bf16_packed — cs_gemm_bf16 (variants 0, 2, 3, 4; same splits, gated, act, workspace
 * rules) on a packed W: every weight-fragment load is one contiguous 1 KB and each wave's W
 * stream one sequential run, instead of 16 rows x 64 B.  Bitwise equal to cs_gemm_bf16 on the
 * unpacked W.
 *
 * Replaces: the same projections of the remote forward as cs_gemm_bf16
 *   (src/utils.py:249-259).
 */
int cs_gemm_pack(const void* w, int64_t ldw, int64_t N, int64_t K, void* w_packed,
                 cs_stream_t stream);

int cs_gemm_bf16_packed(const void* x, int64_t ldx, const void* w_packed, void* y, int64_t ldy,
                        int64_t M, int64_t N, int64_t K, int splits, int gated, int act,
                        int variant, float* workspace, cs_stream_t stream);

/*
 * cs_gemm_w8_pack — W [N, K] bf16 (row stride ldw) quantised to OCP e4m3fn codes (bias 7,
 * largest finite value 448, no infinities, NaN at 0x7f / 0xff; not the fnuz form) with one
 * power-of-two scale per row:
 *   row_exp[n] = the smallest integer e with amax_n * 2^-e <= 448 (an all-zero row: 0), int8
 *   code[n][k] = e4m3_rne(w[n][k] * 2^-row_exp[n])   (subnormal codes kept, NaN never produced)
 *   twin[n][k] = value(code[n][k]) * 2^row_exp[n]    (exactly a bf16 number)
 * codes_packed (N * K bytes) is fragment-major: the 16-row tile T's 64-deep K step s is 1 KB at
 * byte (T * K / 64 + s) * 1024, lane-linear (lane l's 16 bytes = row 16T + l % 16; byte 8h + j
 * of them = k 64s + 32h + 8 (l / 16) + j, h = 0, 1, j = 0..7):
 *   codes_packed[(T * K / 64 + s) * 1024 + 16 l + 8 h + j] = code[16T + l % 16][64s + 32h + 8 (l / 16) + j]
 * twin (row stride ldt) may be NULL, or w itself (in place).  status (device int32) is set to 0,
 * or to 1 (an input is Inf or NaN) | 2 (a row's exponent leaves int8, or one of its twin values
 * is no bf16 number: it overflows or falls below bf16's subnormal grid); when it is not 0,
 * codes_packed, row_exp and twin are left untouched.  N % 16 == 0, K % 64 == 0, ldw and ldt
 * multiples of 8, 16-byte aligned.  No host sync.  Done once per weight, at model load.
 *
 * cs_gemm_w8_pack_codes — the same permutation of given codes [N, K] (row-major bytes).
 *
 * cs_gemm_bf16_w8 — cs_gemm_bf16_packed on such a weight:
 *   Y[m][n] = bf16_rne(2^row_exp[n] * sum_k X[m][k] * value(code[n][k])),
 * codes converted to bf16 in registers, v_mfma_f32_16x16x32_bf16 accumulation in fp32, the scale
 * applied to the fp32 sum (to each K split's partial) before any rounding.  Same rules: N a
 * multiple of 128, K of 64 * splits; splits > 1 (at most 16) folds fp32 partials
 * [splits][M][N] (workspace) in split order, y = NULL leaves them unfolded for
 * cs_rope_place_splitk / cs_add_rms_norm_splitk; splits <= 0 takes cs_gemm_w8_splits; gated = 1
 * pairs gate row f with up row N / 2 + f (each with its own exponent) and writes act(gate) * up
 * with cs_gated_act's roundings (no K split).  M <= cs_gemm_w8_max_rows() (80: the decode
 * steps, where a projection is a weight stream); above it CS_ERR_INVALID, nothing launched.
 * ldx a multiple of 8, ldy of 4; x and the codes 16-byte aligned, row_exp 4-byte.
 * Deterministic (no atomics), no host sync.
 *
 * cs_gemm_bf16_w8_add — the residual form (not gated): h [M, N] (row stride ldh) is read and
 * rewritten in place, h[m][n] = bf16_rne(h[m][n] + 2^row_exp[n] * sum_k ...): the fp32 product is
 * added to the residual before the ONE rounding, as a BLAS epilogue with beta = 1 adds it (a
 * K split adds in its fold).  Same shape, split, alignment and M rules as cs_gemm_bf16_w8 with
 * y = h.
 *
 * Replaces: the same projections of the remote forward as cs_gemm_bf16
 *   (src/utils.py:249-259), on a 1-byte weight stream.
 */
int cs_gemm_w8_pack(const void* w, int64_t ldw, int64_t N, int64_t K, void* codes_packed,
                    int8_t* row_exp, void* twin, int64_t ldt, int32_t* status, cs_stream_t stream);

int cs_gemm_w8_pack_codes(const void* codes, int64_t N, int64_t K, void* codes_packed,
                          cs_stream_t stream);

int cs_gemm_bf16_w8(const void* x, int64_t ldx, const void* codes_packed, const int8_t* row_exp,
                    void* y, int64_t ldy, int64_t M, int64_t N, int64_t K, int splits, int gated,
                    int act, float* workspace, cs_stream_t stream);

int cs_gemm_bf16_w8_add(const void* x, int64_t ldx, const void* codes_packed, const int8_t* row_exp,
                        void* h, int64_t ldh, int64_t M, int64_t N, int64_t K, int splits,
                        float* workspace, cs_stream_t stream);

/* cs_gemm_w8_splits — the K split cs_gemm_bf16_w8 takes for splits <= 0 (>= 1; 0 on a shape it
 * rejects: M, N or K <= 0, N % 128 or K % 64 != 0).  cs_gemm_w8_max_rows — its largest M. */
int64_t cs_gemm_w8_splits(int64_t M, int64_t N, int64_t K, int gated);
int64_t cs_gemm_w8_max_rows(void);

/*
 * cs_nash_lottery — the lottery over m complete statements that maximises Nash welfare
 * F(p) = sum_i log(U_i . p), for P independent problems in one launch, one workgroup each:
 * Frank-Wolfe towards the vertex e_j* of largest gradient g_j = sum_i U[i,j] / a_i (a = U p,
 * agents in index order, lowest j on ties) with a golden-section search of the step gamma in
 * [0, 1] (at most 80 rounds, until the bracket is under 1e-9, gamma* its midpoint), from
 * p = 1/m.  An iteration adopts p <- (1 - gamma*) p + gamma* e_j* and then stops when F grew by
 * less than tol; max_iters = 0 returns the uniform lottery.  All fp64 (utilities reach down to
 * 1e-300); a is carried as a <- (1 - gamma*) a + gamma* U[:,j*] between iterations.
 *
 * U: P problems of [A][ldu] fp64 (first m columns used), problem stride ldp_problem (elements;
 * problems must not overlap), 8-byte aligned.  1 <= A <= 64, 1 <= m <= 16384, ldu >= m,
 * P >= 0, max_iters >= 0, tol finite.
 * variant: 0 = the library's choice, 1 = the problem's U is staged in LDS once (invalid when
 * A * m * 8 exceeds the 147456 bytes the kernel may take), 2 = U is read from global memory
 * every iteration.  Same arithmetic in the same order: the variants' outputs are bitwise equal.
 *
 * out_p [P][m] the lottery; nullable: out_a [P][A] = U p, out_F [P] = sum_i log a_i,
 * out_gap [P] = max_j g_j - A (the Frank-Wolfe certificate: F* - F(p) <= gap by concavity),
 * all three recomputed from the p written; out_iters [P] the iterations run.
 * A problem that holds a negative or non-finite utility, or an agent whose row is all zero,
 * gets out_iters = -1 and NaN in its other outputs; the rest of the batch is unaffected.
 * Deterministic (no atomics), no host sync, no allocation.
 *
 * Replaces: FW_nash_welfare (core.py:116-168) and F_val at its result (core.py:108-113), called
 *   once per (seed, rho) by the reference's sweep (core.py:365-369).
 */
int cs_nash_lottery(const double* U, int32_t P, int32_t A, int32_t m, int64_t ldu,
                    int64_t ldp_problem, int32_t max_iters, double tol, int variant, double* out_p,
                    double* out_a, double* out_F, double* out_gap, int32_t* out_iters,
                    cs_stream_t stream);

/*
 * cs_maximin_lottery — the maximin (egalitarian) lottery and the coalition-improvement factor,
 * for P problems x C coalitions in one launch, one workgroup per (problem, coalition).  For a
 * coalition S and base > 0 let M[i][j] = U[i][j] / base[i], i in S.  The workgroup solves the
 * matrix game value(M) = max_{q in simplex} min_{i in S} (M q)_i and returns
 *   out_alpha = |S| / A * value(M),
 * which is the optimum of the reference's LP "maximise alpha s.t. U_i . p' >= alpha * base_i
 * (i in S), sum p' = |S| / A, p' >= 0" (substitute p' = |S| / A * q); with S = all agents and
 * base = 1 it is the egalitarian LP and q the maximin lottery.
 *
 * Method: with x = q / value the game is min 1.x s.t. M x >= 1, x >= 0, dual-feasible from the
 * all-slack basis, solved by a revised dual simplex: leaving row the most negative basic value;
 * entering column the smallest ratio (reduced cost) / -(pivot-row entry) over the negative
 * entries of the pivot row; lowest index on every tie (the m lottery columns before the
 * slacks).  Only the |S| x |S| basis inverse is carried; the pivot row and the reduced costs
 * are formed from M every pivot.  All fp64.  A one-column problem (m = 1) has one lottery and is
 * answered without a pivot.  There is no fallback rule against cycling: max_pivots bounds the
 * work.  CS_MAXIMIN_MAX_PIVOTS is the default cap: every pivot visits a basis, the most seen
 * over the 1,713 LPs of the recorded 6 x 81 sweep problems was 19 and 259 for a 64 x 300 problem
 * with all 64 agents, so 4096 is generous but finite.
 *
 * U, P, A, m, ldu, ldp_problem: as for cs_nash_lottery (1 <= A <= 64, 1 <= m <= 16384).
 * base [P][A]: nullable = all ones.
 * masks_host / masks: the same C 64-bit coalition masks (bit i = agent i), shared by all
 * problems, once in HOST memory (checked here: an empty mask or a bit at or above A is
 * CS_ERR_INVALID) and once in DEVICE memory (read by the kernel, which ignores bits at or above
 * A and gives an empty mask status -1, so a device copy that differs cannot read out of bounds).
 * Both NULL: one coalition of all agents (C = 1).  P * C <= 2^31 - 1.
 *
 * LDS: the basis inverse (A * (A | 1) * 8 bytes) always; M is staged too when both fit the
 * 147456 bytes the kernel may take, (A * (A | 1) + A * m) * 8 <= 147456.  Above that the kernel
 * reads U from global memory (L2) and divides by base at every use: the same operations in the
 * same order, so the result does not depend on which path ran.  Workgroups of 64 threads up to
 * m = 128, 256 up to m = 4096, 1024 above.
 *
 * out_alpha [P][C]; nullable out_q [P][C][m] (>= 0, sums to 1, exact zeros off the basis);
 * nullable out_lambda [P][C][A], the dual weights (>= 0, zero outside S, sum to 1):
 * min_{i in S} (M q)_i <= value <= max_j (lambda M)_j certifies the result by weak duality;
 * out_pivots [P][C] the pivots taken.
 * out_pivots = -1 and NaN in the other outputs of that (problem, coalition): the problem holds
 * a negative or non-finite utility; a member's base is not finite and positive (the reference's
 * LP is then unbounded and the coalition skipped); a member's row of M is all zero or
 * overflowed.  out_pivots = -2 and NaN: max_pivots exhausted (max_pivots = 0 gives -2 whenever a
 * pivot is needed), or rounding left no column to enter or no positive sum.  The rest of the
 * batch is unaffected.  Deterministic (no atomics): a (problem, coalition) gets the bits it
 * gets alone.  No host sync, no allocation.
 *
 * Replaces: the HiGHS LPs of egalitarian_lottery (core.py:171-206) and of every coalition of
 *   max_coalition_improvement (core.py:214-279), 2^n - 1 per call, three calls per (seed, rho)
 *   of the reference's sweep (core.py:379-381).
 */
#define CS_MAXIMIN_MAX_PIVOTS 4096
int cs_maximin_lottery(const double* U, int32_t P, int32_t A, int32_t m, int64_t ldu,
                       int64_t ldp_problem, const double* base, const uint64_t* masks_host,
                       const uint64_t* masks, int32_t C, int32_t max_pivots, double* out_alpha,
                       double* out_q, double* out_lambda, int32_t* out_pivots, cs_stream_t stream);

/*
 * cs_lottery_policy — the token-level policy a lottery over the m = B^L leaves of a B-ary tree
 * of depth L induces: pi(b | s) = mass(s + b) / mass(s), where mass(s) is the lottery's weight
 * on the contiguous block of leaves under prefix s (leaves in lexicographic order); a prefix of
 * mass <= 0 gets the uniform 1/B.  Masses are summed bottom-up in action order, fp64.
 * p [P][m] contiguous; out_policy [P][sum_{t=1..L} B^t]: per problem the levels t = 0..L-1
 * concatenated, level t holding [B^t prefixes][B actions].  One workgroup per problem.
 * B >= 1, L >= 1, B^L <= 16384 (and L <= 64, which only binds at B = 1).
 *
 * Replaces: the prefix masses and per-step action probabilities of induced_policy_rollout
 *   (core.py:303-325, over build_prefix_index's table, core.py:287-294).
 */
int cs_lottery_policy(const double* p, int32_t P, int32_t B, int32_t L, double* out_policy,
                      cs_stream_t stream);

/*
 * cs_policy_rollout — leaves of the B-ary tree of depth L sampled step by step from a token
 * policy, for P problems at once, with exactly the draws of the reference's
 * ``rng = default_rng(seed)`` and ``rng.choice(B, p=probs)`` per step, and a count per leaf.
 *
 * The draw rule (numpy's Generator.choice with a scalar result): per row of B probabilities
 * cdf = the running sum in action order (fp64, sequential), every entry then divided by the
 * last; u = the next double of the stream; a = the number of cdf entries <= u (searchsorted,
 * side "right").  A zero-probability action has a cdf entry equal to its predecessor's and is
 * never chosen, action 0 at u = 0.0 included; the last entry is exactly 1.0 > u, so a <= B - 1.
 * A walk starts at s = 0 and takes s <- s * B + a for L levels; s is then the leaf's index.
 * The stream is PCG64: state <- state * 0x2360ED051FC65DA44385DF649FCCF645 + inc (mod 2^128),
 * then x = (high word ^ low word) rotated right by state >> 122, u = (x >> 11) * 2^-53.
 * One draw is one step, so a thread reaches its own samples with an O(log) jump-ahead and no
 * uniforms are made or uploaded by the host.
 *
 * policy [P][sum_{t=1..L} B^t]: per-level tables in cs_lottery_policy's output layout (any
 * token policy on the tree, not only a lottery-induced one).
 * rng [P][4]: per problem the PCG64 state's high and low word and the increment's high and low
 * word, the two 128-bit integers of np.random.PCG64(seed).state["state"].
 * Sample i of the whole rollout takes the draws i * L .. i * L + L - 1 of its problem's stream;
 * this call does the samples first_sample .. first_sample + num_samples - 1, so a rollout split
 * over several calls gives the counts of one call.
 * cdf_work: scratch of policy's size (the cdf tables).
 * out_counts [P][B^L] int64 is ADDED TO: the caller zeroes it, split calls accumulate.
 * out_leaf: nullable, [P][num_samples] int32, the leaf each sample of this call reached.
 * out_status [P]: 0 done; -1 the problem's policy holds a negative or non-finite entry, or a row
 * whose sum is further than 2^-26 (1.49e-8, numpy's sqrt(eps) check, where the reference would
 * raise) from 1: its counts and leaves are left untouched, the rest of the batch is unaffected.
 *
 * B >= 1, 1 <= L <= 64, B^L <= 16384, P >= 0, first_sample >= 0, num_samples >= 0,
 * (first_sample + num_samples) * L < 2^62, P * num_samples <= 2^31 - 1 when out_leaf is given;
 * pointers non-NULL and 8-byte aligned (out_leaf, out_status: 4).  P = 0 or num_samples = 0
 * returns CS_OK, launches nothing and writes nothing.
 * Two kernels on the stream: the cdf tables and statuses (one workgroup per problem), then the
 * walk (one workgroup per problem and 4096 samples, 16 consecutive samples per thread).  Counts
 * go through an int32 histogram in LDS (B^L * 4 bytes) and reach out_counts by integer atomic
 * adds: the sums do not depend on the order, so the result is deterministic and a problem gets
 * the counts it gets alone.  No host sync, no allocation.
 *
 * Replaces: the sampling loop of induced_policy_rollout (core.py:313-332), num_samples * L
 *   rng.choice calls on the host, run by the reference for one lottery (core.py:437-444).
 */
int cs_policy_rollout(const double* policy, int32_t P, int32_t B, int32_t L, const uint64_t* rng,
                      int64_t first_sample, int64_t num_samples, double* cdf_work,
                      int64_t* out_counts, int32_t* out_leaf, int32_t* out_status,
                      cs_stream_t stream);

/*
 * cs_schulze — Schulze rank aggregation of E independent elections in one launch, one
 * workgroup per election: R voters' rankings of C candidates become pairwise defeats,
 * strongest-path strengths, a (possibly tied) social ranking, a ranking untied by a ballot, and
 * a winner.  Integer arithmetic throughout: the result is the reference's bit for bit.
 *
 * in_kind selects the stage at which the data enters:
 *   CS_SCHULZE_RANKINGS   in = int32 [E][R][C] ranks, lower is better, ties allowed
 *   CS_SCHULZE_SCORES     in = float [E][R][C] scores, higher is better
 *   CS_SCHULZE_DEFEATS    in = int32 [E][C][C] pairwise defeats (skips stage 1)
 *   CS_SCHULZE_STRENGTHS  in = int32 [E][C][C] path strengths (skips stages 1 and 2)
 * R, valid and out_defeats are ignored where stage 1 is skipped, out_strengths where stage 2 is.
 *
 * Stage 1: d[i][j] = the number of counted voters r with rank[r][i] < rank[r][j] (scores:
 *   score[r][i] > score[r][j]; a NaN compares false both ways, infinities as usual); diagonal 0.
 *   valid [E][R] (nullable = all; bytes, any alignment): voter r counts iff valid[r] != 0.
 * Stage 2: p[i][j] = d[i][j] > d[j][i] ? d[i][j] : 0, diagonal 0; then for every pivot k in
 *   ascending order and all (j, l), j != k, l != k, j != l:
 *   p[j][l] = max(p[j][l], min(p[j][k], p[k][l])).  A pivot reads only row k and column k and
 *   writes neither, so its updates run in parallel with one barrier per pivot and give the
 *   sequential loop's result.  The entries may be any integers (kind DEFEATS).
 * Stage 3: count[i] = #{j : p[i][j] >= p[j][i]} (j = i included); out_ranking[i] = the number
 *   of distinct counts greater than count[i] (np.unique(-count, return_inverse=True)).
 * Tie-break (ballot [E][C] given; any int32 values, repeats allowed): nb[i] = the number of
 *   distinct ballot values below ballot[i], key[i] = out_ranking[i] * C + nb[i],
 *   out_untied[i] = the number of distinct keys below key[i].
 * out_winner[e] = the lowest index of rank 0 in the untied ranking when a ballot is given, else
 *   in out_ranking.
 * out_status[e]: 0 solved; -1 malformed (a counted voter's rank outside [0, C - 1], or a nonzero
 *   diagonal in a DEFEATS / STRENGTHS input: the reference's ValueErrors); -2 valid leaves no
 *   voter.  Every other output of such an election is filled with -1; the rest of the batch is
 *   unaffected.
 *
 * 1 <= C <= 128, 1 <= R <= 65536, E >= 0 (E = 0 returns CS_OK and launches nothing).  in,
 * out_ranking and out_status are required, the other pointers nullable; out_untied needs
 * ballot; all but valid 4-byte aligned.
 * LDS: the C x C matrix with row stride C | 1, one tile of 32 voters and five vectors of C,
 * 84,992 bytes at C = 128; the voters stream through the tile, so R does not grow it.  One wave
 * per workgroup up to C = 16, four above.  Deterministic (no atomics), no host sync, no
 * allocation.
 *
 * Replaces: _schulze_compute_pairwise_defeats, _schulze_compute_strongest_path_strengths,
 *   _schulze_rank_candidates, _hm_untie_ranking_with_ballot and the winner's selection
 *   (src/methods/habermas_machine.py:992-1024, 1048-1160), three nested Python loops per stage.
 */
enum cs_schulze_kind {
  CS_SCHULZE_RANKINGS = 0,
  CS_SCHULZE_SCORES = 1,
  CS_SCHULZE_DEFEATS = 2,
  CS_SCHULZE_STRENGTHS = 3
};
int cs_schulze(const void* in, int in_kind, int32_t E, int32_t R, int32_t C, const uint8_t* valid,
               const int32_t* ballot, int32_t* out_defeats, int32_t* out_strengths,
               int32_t* out_ranking, int32_t* out_untied, int32_t* out_winner, int32_t* out_status,
               cs_stream_t stream);

/*
 * Text encoder (BERT-style, post-LayerNorm: BAAI/bge-large-en-v1.5 and bge-base-en-v1.5) over
 * a RAGGED batch with no padding: text t is tokens cu_seqlens[t] .. cu_seqlens[t + 1] - 1 of
 * the n_tok rows (cu_seqlens int32 [n_text + 1], rising, from 0 to n_tok).  All activations and
 * weights bf16, 16-byte aligned, leading dimensions multiples of 8; the projections between
 * these launches are the caller's GEMMs.
 *
 * Replaces: the hosted embedding call get_embedding (src/utils.py:376-407), a forward pass of
 *   the encoder, and the similarity / welfare arithmetic of src/evaluation.py:232-307.
 *
 * cs_embed_layer_norm — y[tok] = LayerNorm(word_emb[ids[tok]] + pos_emb[tok - cu_seqlens[t]] +
 *   type_emb[0]) * weight + bias, summed and normalised in fp32 (mean, then the variance about
 *   it), rounded once to bf16.  d % 8 == 0, d <= 2048.  max_seqlen (the host's longest text)
 *   above n_pos returns CS_ERR_INVALID without a launch.  The ids live on the device, so what
 *   only they can show is reported there: a token with an id outside [0, vocab), a position
 *   >= n_pos or outside every text gets a zero row and *status = CS_ERR_INVALID (-1); the
 *   caller zeroes *status (device int32) before the call and reads it when it next synchronises.
 * cs_add_layer_norm — y = LayerNorm(x + residual) * weight + bias (residual nullable), the sum
 *   in fp32 and never rounded on its own; y may alias x or residual.  Post-LN with a bias and
 *   a mean, not cs_add_rms_norm.
 * cs_gelu — y = 0.5 x (1 + erf(x / sqrt 2)) in fp32 on bf16 rows [rows][F], F % 8 == 0; y may
 *   alias x.
 * cs_encoder_attention — bidirectional softmax attention: out[tok][h] = softmax_k(scale q.k) v
 *   over the keys of tok's own text only.  qkv [n_tok][ld_qkv >= 3 H D] is the fused projection
 *   read in place (q | k | v, each [H][D], V row-major), out [n_tok][H D] contiguous.  D = 64,
 *   1 <= text length <= max_seqlen <= 512.  bf16 MFMA 16x16x32, fp32 online softmax; one
 *   workgroup per (text, head, 64-query tile), key blocks of 32; a text's output depends on no
 *   byte of any other text.  A text whose cu_seqlens entries are not 0 < length <= max_seqlen
 *   inside [0, n_tok] is skipped (nothing of it read or written).
 */
int cs_embed_layer_norm(const int32_t* ids, const int32_t* cu_seqlens, int32_t n_text, int64_t n_tok,
                        int32_t max_seqlen, const void* word_emb, int32_t vocab, const void* pos_emb,
                        int32_t n_pos, const void* type_emb, const void* weight, const void* bias,
                        int64_t d, float eps, void* y, int64_t ldy, int32_t* status,
                        cs_stream_t stream);
int cs_add_layer_norm(const void* x, int64_t ldx, const void* residual, int64_t ldr,
                      const void* weight, const void* bias, int64_t rows, int64_t d, float eps,
                      void* y, int64_t ldy, cs_stream_t stream);
int cs_gelu(const void* x, int64_t ldx, int64_t rows, int64_t F, void* y, int64_t ldy,
            cs_stream_t stream);
int cs_encoder_attention(const void* qkv, int64_t ld_qkv, const int32_t* cu_seqlens, int32_t n_text,
                         int64_t n_tok, int32_t max_seqlen, int32_t H, int32_t D, float scale,
                         void* out, cs_stream_t stream);

/*
 * cs_cosine_welfare — the evaluator's embedding utilities in one launch, all arithmetic fp64.
 *
 * E_s [S][ld_s], E_a [A][ld_a] fp32 embeddings of the statements and of the agents' opinions
 * (first d columns); valid_s [S], valid_a [A] bytes (nullable: all valid; 0 = the embedding is
 * missing, the reference's None).
 *   out_cos[a][s]  = 1 - clip(1 - u.v / sqrt(u.u v.v), 0, 2)   (1 - scipy.spatial.distance.cosine)
 *                    0.0 if u.u == 0 or v.v == 0; NaN if either is missing or the value is
 *                    not finite (the reference's None)
 *   out_welfare[0][s] = min, [1][s] = sum, [2][s] = sum log(max(c, eps)) over the FINITE
 *                    out_cos[.][s], agents in order (Python's left-to-right sums); NaN when
 *                    none is finite.
 * out_cos [A][S], out_welfare [3][S] fp64.  One workgroup per statement; deterministic.
 *
 * Replaces: src/evaluation.py:239-307 (per agent, per statement, in Python).
 */
int cs_cosine_welfare(const float* E_s, int64_t ld_s, const float* E_a, int64_t ld_a,
                      const uint8_t* valid_s, const uint8_t* valid_a, int32_t S, int32_t A, int64_t d,
                      double eps, double* out_cos, double* out_welfare, cs_stream_t stream);

/*
 * Clustering of embeddings: StandardScaler, KMeans and the row nearest each centre, scikit-learn's
 * decisions restated, all arithmetic fp64 (csrc/cluster.hip).  Matrices are row-major doubles with
 * a leading dimension >= d, 8-byte aligned.  Kernel boundaries are the only grid-wide
 * synchronisation; every sum over points is folded in a fixed order (per-tile partials, then the
 * tiles in order) and there is no floating-point atomic, so two runs are bitwise equal.
 *
 * Limits (CSError / CS_ERR_INVALID above them): k <= 64, d <= 4096, n <= 2^20, R <= 1024.
 *
 * cs_standardize — Z = (X - mean) / scale per column.  mean = sum / n; var = (sum (x - mean)^2 -
 *   (sum (x - mean))^2 / n) / n (ddof 0); scale = sqrt(var), or 1 for a constant feature:
 *   var <= n eps var + (n mean eps)^2, eps = 2^-52.  Z may alias X.
 *
 * cs_kmeans_seed — k-means++ for R restarts at once.  Z is centred by the caller.  first [R]
 *   int32 rows, u [R][k - 1][T] doubles in [0, 1), T = 2 + int(log k): the draws of
 *   numpy's RandomState, made by the caller.  Both are given twice: on the host (checked here,
 *   before any launch) and on the device (read by the kernels).  Per restart: the first centre is
 *   Z[first]; closest[i] the squared distance of row i to it, pot = sum closest; for
 *   c = 1 .. k - 1 the candidates are min(searchsorted(cumsum(closest), u pot, side=left), n - 1),
 *   the one with the smallest sum of min(closest, dist^2(candidate, .)) is kept (first on ties)
 *   and closest, pot become its.  centers [R][k][d], indices [R][k].
 *
 * cs_kmeans_init — labels = -1, state = running, and tol_abs = mean(var(Z, axis 0)) * tol in the
 *   workspace.  state is int32 [2 R + 1]: done [R] (0 running, 1 the labels repeated, 2 the
 *   tolerance or max_iter ended it), n_iter [R], live (the number of restarts still running).
 *
 * cs_kmeans_iterate — n_steps Lloyd iterations of every running restart; the workgroups of a
 *   finished restart exit, so the host enqueues steps blindly and polls `live`.  One iteration:
 *   label = the first lowest squared distance to the old centres; per-cluster sums and counts;
 *   empty clusters, in increasing id, take the points farthest from their assigned old centre,
 *   farthest first, the lower index among equal distances (sum[o] -= z, sum[e] = z, count[e] = 1,
 *   count[o] -= 1; labels unchanged; nothing moves if that largest distance is 0);
 *   centre = sum * (1 / count), a cluster still empty takes the first largest cluster's row;
 *   shift = sum_c |new_c - old_c|^2.  Done if the labels equal the previous iteration's (1), else
 *   if shift <= tol_abs or n_iter == max_iter (2).  centers [R][k][d] is updated in place.
 *
 * cs_kmeans_finish — restarts not done by repeated labels are labelled once more against their
 *   final centres; inertia[r] = sum_i |z_i - c_label(i)|^2; per group of n_init consecutive
 *   restarts (R % n_init == 0), restart r replaces the incumbent if its inertia is lower and its
 *   labels are not the incumbent's partition renamed.  out_best [R / n_init] (index within the
 *   group), out_labels [R / n_init][n], out_centers [R / n_init][k][d] (mean [d], nullable, added
 *   back), out_inertia [R], out_n_iter [R].
 *
 * cs_nearest_rows — for each of q rows of Q the index of the nearest of X's n rows (squared
 *   distance, the first lowest index on ties) and the Euclidean distance.
 *
 * The three cs_kmeans_* calls of one fit share one workspace of cs_kmeans_workspace_size bytes,
 * 16-byte aligned; nothing else may touch it between them.
 *
 * Replaces: sklearn's StandardScaler, KMeans(n_init, random_state) and
 *   pairwise_distances_argmin_min as data/cluster_habermas_issues.py:118-160 calls them.
 */
#define CS_KMEANS_MAX_K 64
#define CS_KMEANS_MAX_D 4096
#define CS_KMEANS_MAX_N 1048576
#define CS_KMEANS_MAX_R 1024
size_t cs_standardize_workspace_size(int32_t n, int32_t d);
int cs_standardize(const double* X, int64_t ldx, int32_t n, int32_t d, double* Z, int64_t ldz,
                   double* mean, double* scale, void* workspace, size_t workspace_bytes,
                   cs_stream_t stream);
size_t cs_kmeans_workspace_size(int32_t n, int32_t d, int32_t k, int32_t R);
int cs_kmeans_seed(const double* Z, int64_t ldz, int32_t n, int32_t d, int32_t k, int32_t R,
                   int32_t T, const int32_t* first_host, const double* u_host, const int32_t* first,
                   const double* u, double* centers, int32_t* indices, void* workspace,
                   size_t workspace_bytes, cs_stream_t stream);
int cs_kmeans_init(const double* Z, int64_t ldz, int32_t n, int32_t d, int32_t k, int32_t R,
                   double tol, int32_t* state, void* workspace, size_t workspace_bytes,
                   cs_stream_t stream);
int cs_kmeans_iterate(const double* Z, int64_t ldz, int32_t n, int32_t d, int32_t k, int32_t R,
                      double* centers, int32_t* state, int32_t n_steps, int32_t max_iter,
                      void* workspace, size_t workspace_bytes, cs_stream_t stream);
int cs_kmeans_finish(const double* Z, int64_t ldz, int32_t n, int32_t d, int32_t k, int32_t R,
                     int32_t n_init, const double* centers, const double* mean, const int32_t* state,
                     int32_t* out_best, int32_t* out_labels, double* out_centers, double* out_inertia,
                     int32_t* out_n_iter, void* workspace, size_t workspace_bytes,
                     cs_stream_t stream);
size_t cs_nearest_rows_workspace_size(int32_t q, int32_t n);
int cs_nearest_rows(const double* Q, int64_t ldq, int32_t q, const double* X, int64_t ldx, int32_t n,
                    int32_t d, int32_t* out_index, double* out_dist, void* workspace,
                    size_t workspace_bytes, cs_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* CONSENSUS_SCORING_H */
