"""Measure the FP8 weight stream of the decode-step projections (csrc/gemm_w8.hip) against the
bf16 route of the same twin weights, on this MI355X, and record the quantisation error of the
format.

Per shape, in one process, interleaved: A = ops.linear on the bf16 twin exactly as the
dispatch table routes that (M, N, K) (cs_gemm_bf16, packed where the table packs, else
hipBLASLt + cs_gated_act, with the committed TunableOp selection as bench.py uses it);
B = ops.linear with the Fp8Weight.  Distinct weight copies are rotated so every call streams
from HBM, not from the 256 MB Infinity Cache.  A sample is the device-event time of one batch
of calls; a round's figure is the median of its samples; the reported time is the median over
rounds and the spread is the range of A's (and B's) round medians.  One json line per shape
goes to profiles/w8_bench.jsonl; the shapes where B is not faster by more than A's spread go
to tuned/gemm_w8_mi355x.json with --install, the list ops.linear reads to keep them on bf16.

Also: one captured decode step (DecodeState + LM head, 48 streams) of random:llama-3.1-8b
against random:llama-3.1-8b@fp8, and max / mean |delta log-prob| of get_prompt_logprobs
between an engine on the original weights and its @fp8 engine (a property of the format, not
of the kernel; recorded, no threshold) on the trace fixtures' tiny-llama architecture and on
random:llama-3.1-8b.

    python tools/w8_bench.py [--out profiles/w8_bench.jsonl] [--install] [--quick]
"""
import argparse
import importlib
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
PKG = "generating-fair-consensus-statements-with-social-choice-on-token-level-mdps_amd"
rt = importlib.import_module(PKG + ".runtime")
ops = importlib.import_module(PKG + ".ops")
engine = importlib.import_module(PKG + ".engine")
utils = importlib.import_module(PKG + ".utils")

# Llama-3.1-8B's projections (q|k|v, output, gate|up, down, LM head) and the per-rank 70B gate|up
SHAPES = [(6144, 4096, False), (4096, 4096, False), (28672, 4096, True), (4096, 14336, False),
          (128256, 4096, False), (57344, 8192, True)]
ROWS = (20, 48, 72, 144)
REQUIRED = {(48, 28672, 4096, True), (48, 4096, 14336, False)}
ROTATE_BYTES = 800 << 20          # bf16 bytes of distinct weights a route cycles through


def _time_batch(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(n):
        fn(i)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / n          # us per call


def ab(fa, fb, iters, rounds=5, samples=5):
    """(A's round medians, B's round medians) in us, A and B alternating sample by sample."""
    for f in (fa, fb):
        _time_batch(f, iters)                    # warm-up: code objects, hipBLASLt's choice
    ra, rb = [], []
    for _ in range(rounds):
        sa, sb = [], []
        for _ in range(samples):
            sa.append(_time_batch(fa, iters))
            sb.append(_time_batch(fb, iters))
        ra.append(statistics.median(sa))
        rb.append(statistics.median(sb))
    return ra, rb


def bench_shape(M, N, K, gated, dev, quick):
    g = torch.Generator(device=dev).manual_seed(N + K + M)
    nbuf = max(2, -(-ROTATE_BYTES // (N * K * 2)))
    if quick:
        nbuf = 2
    key = f"{M},{N},{K},{int(gated)}"
    ch = ops.gemm_choice(M, N, K, gated, packed=True)
    packs = ch is not None and ch["packed"]
    if ch is None and gated:                     # the gated fall-back: the plain product + cs_gated_act
        chp = ops.gemm_choice(M, N, K, False, packed=True)
        packs = chp is not None and chp["packed"]
    ws, pws, fws = [], [], []
    for _ in range(nbuf):
        w = (torch.randn(N, K, generator=g, device=dev) * 0.02).to(torch.bfloat16)
        fws.append(ops.gemm_w8_pack(w, twin_out=w))          # w is now the twin
        ws.append(w)
        pws.append(ops.gemm_pack(w) if packs else None)
    x = torch.randn(M, K, generator=g, device=dev).to(torch.bfloat16)
    n_out = N // 2 if gated else N
    ya = torch.empty(M, n_out, dtype=torch.bfloat16, device=dev)
    yb = torch.empty_like(ya)
    served = ops.gemm_w8_serves(M, N, K, gated)

    def fa(i):
        ops.linear(x, ws[i % nbuf], gated=gated, out=ya, packed=pws[i % nbuf])

    def fb(i):
        ops.linear(x, ws[i % nbuf], gated=gated, out=yb, packed=fws[i % nbuf])

    fa(0)
    fb(0)
    torch.cuda.synchronize()
    ref = ya.float()
    tol = ref.abs() * 2.0 ** -7 + 1e-3 * ref.abs().max()
    err = float(((yb.float() - ref).abs() / tol).max())
    iters = max(nbuf, 20) if not quick else 4
    ra, rb = ab(fa, fb, iters, rounds=2 if quick else 5, samples=3 if quick else 5)
    ta, tb = statistics.median(ra), statistics.median(rb)
    act = (M * K + M * n_out) * 2
    rec = {"kind": "gemm", "key": key, "M": M, "N": N, "K": K, "gated": gated,
           "a_route": ("cs_gemm_bf16 v%d s%d%s" % (ch["variant"], ch["splits"], " packed" if ch["packed"] else "")
                       if ch is not None else "hipBLASLt" + (" + cs_gated_act" if gated else "")),
           "b_served": served, "weight_copies": nbuf, "calls_per_sample": iters,
           "a_us": round(ta, 2), "b_us": round(tb, 2),
           "a_round_medians_us": [round(v, 2) for v in ra], "b_round_medians_us": [round(v, 2) for v in rb],
           "a_spread_us": round(max(ra) - min(ra), 2), "b_spread_us": round(max(rb) - min(rb), 2),
           "a_bytes_per_s": round((N * K * 2 + act) / ta * 1e6), "b_bytes_per_s": round((N * K + N + act) / tb * 1e6),
           "ratio_a_over_b": round(ta / tb, 3), "max_err_over_bound": round(err, 3),
           "b_faster_beyond_a_spread": bool(ta - tb > max(ra) - min(ra))}
    del ws, pws, fws
    torch.cuda.empty_cache()
    return rec


def decode_step(ident, steps, dev):
    """us per captured step (DecodeState + LM head) of 48 streams: 6 prefixes x 8 beams."""
    eng, _ = rt.get_engine(ident)
    g = torch.Generator().manual_seed(7)
    V = eng.model.cfg.vocab
    prefixes = [torch.randint(5, V - 5, (256,), generator=g).tolist() for _ in range(6)]
    with rt.device_lock(dev):
        st = engine.DecodeState(eng, eng.prefill(prefixes), n_prefix=6, n_beams=8, max_steps=steps + 8)
        logits = torch.empty(48, V, dtype=torch.bfloat16, device=dev)

        def post():
            eng.model.lm_head(st.hidden, out=logits)

        def run(n):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(n):
                st.advance(list(range(8)), [11] * 8, post=post)
            b.record()
            b.synchronize()
            return a.elapsed_time(b) * 1e3 / n

        run(4)                                   # the eager step and both parities' captures
        return st, run


def quant_error(base, dev):
    """max and mean |delta log-prob| of get_prompt_logprobs, original weights vs the @fp8 engine"""
    users = ["Should the city spend more on public transport or on road repairs? " * 3,
             "What is a fair way to share the cost of a new community centre among residents? " * 3]
    d = []
    for u in users:
        a = utils.get_prompt_logprobs(base, "You are a careful assistant.", u)
        b = utils.get_prompt_logprobs(base + rt.FP8_SUFFIX, "You are a careful assistant.", u)
        assert a[0] == b[0] and len(a[1]) > 8
        d += [abs(p - q) for p, q in zip(a[1], b[1]) if p is not None and q is not None]
    return {"kind": "quant_error", "model": base, "positions": len(d), "max_abs_dlogprob": max(d),
            "mean_abs_dlogprob": sum(d) / len(d)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "w8_bench.jsonl"))
    ap.add_argument("--install", action="store_true", help="write tuned/gemm_w8_mi355x.json")
    ap.add_argument("--quick", action="store_true", help="two small shapes, few samples (a rehearsal)")
    ap.add_argument("--no-model", action="store_true", help="skip the 8B decode step and error runs")
    ap.add_argument("--from", dest="src", help="no measurement: --install from this run's records")
    args = ap.parse_args()
    if args.src:
        with open(args.src) as f:
            install([json.loads(line) for line in f if line.strip()])
        return
    if not torch.cuda.is_available():
        sys.exit("w8_bench needs the GPU: nothing is measured without one")
    dev = torch.device("cuda", torch.cuda.current_device())
    rt.use_gemm_tuning()
    ops.gemm_w8_serves(1, 128, 64)               # loads the exclusion list ...
    ops._w8_excluded = frozenset()               # ... and measures every shape regardless of it
    shapes = [(512, 1024, False), (1024, 512, True)] if args.quick else SHAPES
    recs = []
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        def emit(rec):
            recs.append(rec)
            f.write(json.dumps(rec) + "\n")
            f.flush()
            print(json.dumps(rec), flush=True)

        for N, K, gated in shapes:
            for M in ROWS:
                if M > ops.gemm_w8_max_rows():
                    continue                     # not served: both routes would be the same call
                emit(bench_shape(M, N, K, gated, dev, args.quick))
        emit(quant_error("random:tiny-llama", dev))
        if not args.no_model and not args.quick:
            ops._w8_excluded = None              # the decode step runs with the installed exclusion list
            base = "random:llama-3.1-8b"
            emit(quant_error(base, dev))
            steps = 60
            sa, ra = decode_step(base, 6 * steps, dev)
            sb, rb = decode_step(base + rt.FP8_SUFFIX, 6 * steps, dev)
            ta, tb = [], []
            for _ in range(5):
                ta.append(ra(steps))
                tb.append(rb(steps))
            emit({"kind": "decode_step", "model": base, "streams": 48, "prefix_tokens": 256,
                  "steps_per_sample": steps, "bf16_step_us": round(statistics.median(ta), 1),
                  "fp8_step_us": round(statistics.median(tb), 1),
                  "bf16_samples_us": [round(v, 1) for v in ta], "fp8_samples_us": [round(v, 1) for v in tb]})
            sa.release()
            sb.release()
    if args.install:
        install(recs)


def install(recs):
    """tuned/gemm_w8_mi355x.json: the measured shapes where B is not faster beyond A's spread."""
    slow = [r["key"] for r in recs if r["kind"] == "gemm" and not r["b_faster_beyond_a_spread"]]
    missed = [r["key"] for r in recs if r["kind"] == "gemm" and r["key"] in slow and
              (r["M"], r["N"], r["K"], r["gated"]) in REQUIRED]
    if missed:
        sys.exit(f"FP8 is not faster beyond A's spread at the required shapes {missed}: "
                 "not writing a table that excludes them")
    path = os.path.join(REPO, PKG, "tuned", "gemm_w8_mi355x.json")
    with open(path, "w") as f:
        json.dump({"about": "M,N,K,gated shapes tools/w8_bench.py measured no faster on cs_gemm_bf16_w8 "
                            "than on the bf16 route of the twin (beyond the spread of the bf16 route's "
                            "repeated medians): ops.linear keeps them on bf16",
                   "exclude": sorted(slow)}, f, indent=1)
        f.write("\n")
    print("wrote", path)


if __name__ == "__main__":
    main()
