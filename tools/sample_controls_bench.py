#!/usr/bin/env python3
"""What the sampling controls cost and save, at the Best-of-N generation shape of BASELINE C2
(64 streams, 150 tokens, the 128,256-token vocabulary).

  kernel    one cs_sample_step_ex call with the repetition penalty on (a 300-token prompt and
            150 generated tokens in every stream's seen set) against cs_sample_step on the
            same bf16 logits.  The two alternate in one process; a timed window is --calls
            calls between two device events, replayed from captured graphs of 200 calls (so no
            host time per call is in it), each call preceded by the two small fills that
            put the streams' state back (out_len = 150, done = 0), and a window of the fills
            alone is timed beside them and subtracted.  Median, min and max over --rounds
            windows; the min-to-max range of cs_sample_step's own windows is the run-to-run
            spread on this box.
  steps     utils.generate_texts' device loop (runtime.generate_streams on the prompt
            generate_texts renders) with an ASCII terminator, with the device's stop-string
            test and without it (what the loop did before it had one): decode steps that ran,
            tokens decoded over all streams, and how many cut texts are equal.  The plain loop
            runs twice (are two runs of one call equal?) and the stop test runs once more with
            a string no token holds (cs_sample_step_ex on every step, no stream ending early:
            are the two kernels' draws equal?), so that a difference between the paths can be
            told from a difference that ending streams early makes to their neighbours.
            Counts, not times.

Writes one JSON line:

  python tools/sample_controls_bench.py [--out profiles/sample_controls_bench.jsonl]
"""
import argparse
import importlib
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
PKG = "generating-fair-consensus-statements-with-social-choice-on-token-level-mdps_amd"

S, V, T, PROMPT = 64, 128256, 150, 300       # BASELINE C2's candidate generation
PRESET = "llama-3.1-8b"
A = 8


def kernel_times(torch, ops, dev, calls, rounds):
    g = torch.Generator().manual_seed(0)
    logits = (torch.randn(S, V, generator=g) * 3.0).to(torch.bfloat16).to(dev)
    base = torch.arange(1, S + 1, dtype=torch.int64, device=dev)
    step = torch.zeros(1, dtype=torch.int32, device=dev)
    done = torch.zeros(S, dtype=torch.int32, device=dev)
    out_len = torch.full((S,), T, dtype=torch.int32, device=dev)
    out_tok = torch.randint(0, V, (S, T + 1), generator=g).to(torch.int32).to(dev)
    next_tok = torch.zeros(S, dtype=torch.int64, device=dev)
    n_alive = torch.zeros(1, dtype=torch.int32, device=dev)
    seen_ids = torch.randint(0, V, (S * PROMPT,), generator=g).to(torch.int32).to(dev)
    seen_off = (torch.arange(S + 1, dtype=torch.int32) * PROMPT).to(dev)
    ws = ops.Workspace(zeroed=True)
    state = (logits, base, step, done, out_len, out_tok, next_tok, n_alive)

    def reset():
        out_len.fill_(T)
        done.zero_()

    def parent():
        reset()
        ops.sample_step(*state, pad_id=0, workspace=ws)

    def penalised():
        reset()
        ops.sample_step_ex(*state, pad_id=0, workspace=ws, repetition_penalty=1.3,
                           seen_ids=seen_ids, seen_off=seen_off)

    paths = {"fills": reset, "sample_step": parent, "sample_step_ex_penalty": penalised}
    graphs = {}
    per_graph = 200                               # calls captured per graph: no host time per call
    replays = max(1, calls // per_graph)
    for name, fn in paths.items():
        fn()                                      # eager once: the workspace exists before capture
        torch.cuda.synchronize()
        graphs[name] = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graphs[name]):
            for _ in range(per_graph):
                fn()
    us = {k: [] for k in paths}
    for rnd in range(rounds + 1):                 # round 0 warms every path
        for name in paths:
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(replays):
                graphs[name].replay()
            t1.record()
            t1.synchronize()
            if rnd:
                us[name].append(t0.elapsed_time(t1) * 1e3 / (replays * per_graph))
    res = {"S": S, "V": V, "dtype": "bf16", "prompt_tokens_seen": PROMPT, "generated_tokens_seen": T,
           "calls_per_window": replays * per_graph, "calls_per_graph": per_graph, "windows": rounds,
           "warmup_windows": 1}
    for name, v in us.items():
        res[name + "_us"] = {"median": round(statistics.median(v), 2), "min": round(min(v), 2),
                             "max": round(max(v), 2)}
    f = res["fills_us"]["median"]
    res["sample_step_us_less_fills"] = round(res["sample_step_us"]["median"] - f, 2)
    res["sample_step_ex_penalty_us_less_fills"] = round(
        res["sample_step_ex_penalty_us"]["median"] - f, 2)
    res["penalty_extra_us"] = round(res["sample_step_ex_penalty_us"]["median"]
                                    - res["sample_step_us"]["median"], 2)
    res["sample_step_spread_us"] = round(res["sample_step_us"]["max"] - res["sample_step_us"]["min"], 2)
    return res


def decode_steps(torch, R, dev, preset, n, max_tokens, terminator):
    import bench
    bon = importlib.import_module(PKG + ".methods.best_of_n")
    eng, tok = R.random_engine(preset, dev, reuse_caches=0, tokenizer_dir=bench.BPE_FIXTURE)
    user = bon.BON["ref_user"].format(issue=bench.SCENARIO_ISSUE,
                                      opinions_text=bon.opinions_text(bench.synthetic_opinions(A)))
    ids, _ = tok.render_chat(bon.BON["ref_system"], user)
    seeds = [1 + i for i in range(n)]
    res = {"preset": preset, "prompt_tokens": len(ids), "n": n, "max_tokens": max_tokens,
           "terminator": terminator, "token_bytes_table": tok.token_bytes() is not None,
           "early_stop_strings": [s.decode() for s in R.early_stop_strings((terminator,))]}
    texts, toks = {}, {}
    E = importlib.import_module(PKG + ".engine")
    keep, advance, advances = R.early_stop_strings, E.DecodeState.advance_device, []
    E.DecodeState.advance_device = lambda self, post=None: (advances.append(1),
                                                            advance(self, post=post))[1]
    # the loop without the stop test runs twice: whether two runs of the SAME call draw the same
    # tokens on this model is what a difference between the two paths has to be read against
    # and once with a stop string that no token holds: cs_sample_step_ex on every step, but no
    # stream ends early, so its tokens against the plain run's are the two kernels' draws alone
    never = "\x01\x02"
    for name, on, term in (("device_stop", True, terminator), ("no_device_stop", False, terminator),
                           ("no_device_stop_again", False, terminator),
                           ("device_stop_never_matching", True, never)):
        # without the stop test: the loop as it was, no stop string reaches the step
        R.early_stop_strings = keep if on else (lambda strings: [])
        advances.clear()
        try:
            outs = R.generate_streams(eng, tok, [ids], seeds, max_tokens, 1.0, stop_strings=(term,))
        finally:
            R.early_stop_strings = keep
        steps = 1 + len(advances)               # the first draw, then one per advance
        toks[name] = outs[0]
        res[name] = {"decode_steps": steps, "tokens_decoded": sum(len(o) for o in outs[0])}
        texts[name] = []
        for o in outs[0]:
            t = tok.decode(o)
            texts[name].append(t[:t.find(terminator)] if terminator in t else t)
    full, cut = toks["no_device_stop"], toks["device_stop"]
    table = R.stop_token_table(tok, eng.model.cfg.vocab)
    stops = R.early_stop_strings((terminator,))

    def stop_len(seq):
        tail = b""
        for k, v in enumerate(seq):
            hit, tail = R.stop_window_push(tail, table[v], stops)
            if hit:
                return k + 1
        return len(seq)

    res["streams_equal_between_the_two_plain_runs"] = sum(
        a == b for a, b in zip(full, toks["no_device_stop_again"]))
    res["streams_equal_with_a_never_matching_stop_string"] = sum(
        a == b for a, b in zip(full, toks["device_stop_never_matching"]))
    first = [next((k for k, (x, y) in enumerate(zip(f, c)) if x != y), None) for f, c in zip(full, cut)]
    res["first_differing_step_per_stopped_stream"] = first
    res["stop_step_per_stream_in_the_plain_run"] = [stop_len(f) for f in full]
    res["stopped_streams_that_are_prefixes_of_the_plain_run"] = sum(
        f[:len(c)] == c for f, c in zip(full, cut))
    res["stopped_streams_ending_where_the_host_rule_ends_them"] = sum(
        len(c) == stop_len(c) for c in cut)
    res["prefix_streams_ending_where_the_plain_run_completes_the_terminator"] = sum(
        len(c) == stop_len(f) for f, c in zip(full, cut) if f[:len(c)] == c)
    res["cut_texts_equal"] = sum(a == b for a, b in zip(texts["device_stop"], texts["no_device_stop"]))
    res["cut_texts_equal_between_the_two_plain_runs"] = sum(
        a == b for a, b in zip(texts["no_device_stop"], texts["no_device_stop_again"]))
    res["streams_with_terminator"] = sum(
        len(a) < len(tok.decode(o)) for a, o in zip(texts["no_device_stop"], full))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "sample_controls_bench.jsonl"))
    ap.add_argument("--calls", type=int, default=10000)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--preset", default=PRESET)
    ap.add_argument("--n", type=int, default=S)
    ap.add_argument("--max-tokens", type=int, default=T)
    ap.add_argument("--terminator", default="e")
    ap.add_argument("--skip-steps", action="store_true")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("sample_controls_bench needs the GPU (no CPU path)")
    ops = importlib.import_module(PKG + ".ops")
    R = importlib.import_module(PKG + ".runtime")
    dev = torch.device("cuda", torch.cuda.current_device())
    line = {"bench": "sample_controls", "gpu": torch.cuda.get_device_name(dev),
            "kernel": kernel_times(torch, ops, dev, args.calls, args.rounds)}
    if not args.skip_steps:
        line["steps"] = decode_steps(torch, R, dev, args.preset, args.n, args.max_tokens,
                                     args.terminator)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(line) + "\n")
    print(json.dumps(line))


if __name__ == "__main__":
    main()
